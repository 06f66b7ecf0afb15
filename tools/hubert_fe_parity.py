"""Records how far ``HubertFrontHIP`` is from the fp32 feature extractor, as a fraction of how far torch's own ``.half()`` module is (what the
reference runs with ``is_half``), on the seeded weights of tests/hubert_cases.py; and its error against the fp64 oracle next to the bars.

    python tools/hubert_fe_parity.py --out profiles/hubert_fe_parity.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import hubert_cases as hc  # noqa: E402

CASES = (hc.Case(1, 16000, 14), hc.Case(3, 5040, 41), hc.Case(1, 5040, 51, True, 2.5), hc.Case(2, 16000, 55, False, 1.0, "dc"),
         hc.Case(1, 5040, 54, True, 1.0, "small"), hc.Case(1, 41040, 21))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_fe_parity.json"))
    a = ap.parse_args()
    import rvc_amd

    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "cases": [],
           "method": "seeded weights; reference = transformers HubertFeatureEncoder fp32 on the GPU; torch_half = the same module .half(); "
                     "oracle = tests/hubert_cases.py fp64 with the kernel's fp16 rounding points; errors are (RMS, max-abs)"}
    for c in CASES:
        w = hc.weights(c.seed, c.wgain)
        x = torch.from_numpy(hc.inputs(c).copy()).to(dev)
        fe32 = hc.hf_module(w, torch.float32).to(dev)
        fe16 = hc.hf_module(w, torch.float32).to(dev).half()
        hip = rvc_amd.HubertFrontHIP.from_module(fe32)
        with torch.no_grad():
            ref = fe32(x).double().cpu().numpy()
            t16 = fe16(x.half()).double().cpu().numpy()
            got = hip(x.half() if c.half else x).double().cpu().numpy()
        e_t, e_h = hc.err(t16, ref), hc.err(got, ref)
        b = hc.bars(c)
        e_o = hc.err(got, b["y"])
        row = {"case": hc.case_id(c), "max_abs_ref": float(np.abs(ref).max()), "torch_half_vs_fp32": e_t, "hip_vs_fp32": e_h,
               "hip_over_torch_half_rms": e_h[0] / e_t[0] if e_t[0] else None, "hip_over_torch_half_max": e_h[1] / e_t[1] if e_t[1] else None,
               "hip_vs_oracle": e_o, "bar_rms": float(b["bar_rms"]), "bar_max": float(b["bar_max"]), "floor_rms": b["floor_rms"], "floor_max": b["floor_max"]}
        res["cases"].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
