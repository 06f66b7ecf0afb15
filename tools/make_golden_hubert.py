"""Writes tests/golden/hubert_fe_*.npz: for each case of ``hubert_cases.GOLDEN`` the seeded input ``x`` [B, N] float32 and the output ``y``
[B, 512, L] float64 of transformers' ``HubertFeatureEncoder`` in float64 holding the seeded weights of tests/hubert_cases.py (weights are
rebuilt from the seed by whoever reads the file; only the input and the expected output are stored).

    python tools/make_golden_hubert.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hubert_cases as hc  # noqa: E402


def main():
    import transformers

    for name, c in sorted(hc.GOLDEN.items()):
        x = hc.inputs(c)
        fe = hc.hf_module(hc.weights(c.seed, c.wgain), torch.float64)
        with torch.no_grad():
            y = fe(torch.from_numpy(x.copy()).double()).numpy()
        path = os.path.join(hc.GOLDEN_DIR, name + ".npz")
        np.savez(path, x=x, y=y, seed=np.int64(c.seed), transformers_version=np.str_(transformers.__version__))
        print("%s: x %s y %s, %d bytes" % (path, x.shape, y.shape, os.path.getsize(path)))


if __name__ == "__main__":
    main()
