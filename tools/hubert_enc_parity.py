"""Records how far twelve swapped HuBERT-base layers (``HubertLayerHIP``, csrc/hubert_enc.hip) are from the same layers in fp64, as a fraction of
how far torch's own ``.half()`` layers are (what the reference runs with ``is_half``), on the seeded weights of tests/hubert_enc_cases.py.

    python tools/hubert_enc_parity.py --out profiles/hubert_enc_parity.json
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

import hubert_enc_cases as hc  # noqa: E402

FRAMES = (137, 599)
LAYERS, SEED = 12, 90


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_enc_parity.json"))
    a = ap.parse_args()
    import rvc_amd

    dev = torch.device("cuda:0")
    ws = hc.weights("base", SEED, 1.0, LAYERS)
    res = {"device": torch.cuda.get_device_name(0), "layers": LAYERS, "cases": [],
           "method": "seeded HuBERT-base layers (d 768, 12 heads, FFN 3072); reference = the fairseq-shaped torch layers of tests/hubert_enc_cases.py in "
                     "fp64 on the GPU; torch_half = the same layers .half() on an fp16 input; hip = the same .half() model after "
                     "accelerate_hubert_layers; after_layers = 9 (the v1 output layer) and 12; errors are (RMS, max-abs) against fp64"}
    m64 = hc.fs_model(ws, "base").double().to(dev)
    m16 = hc.fs_model(ws, "base").half().to(dev)
    for T in FRAMES:
        x = torch.from_numpy(np.random.default_rng(SEED + T).standard_normal((1, T, 768)).astype(np.float32)).half().to(dev)
        for n in (9, LAYERS):
            def run(model, xin):
                kept = list(model.encoder.layers)
                try:
                    model.encoder.layers = torch.nn.ModuleList(kept[:n])
                    with torch.no_grad():
                        return model(xin).double().cpu().numpy()
                finally:
                    model.encoder.layers = torch.nn.ModuleList(kept)

            ref = run(m64, x.double())
            t16 = run(m16, x)
            assert rvc_amd.accelerate_hubert_layers(m16) == LAYERS
            got = run(m16, x)
            assert rvc_amd.restore_hubert_layers(m16) == LAYERS
            e_t, e_h = hc.err(t16, ref), hc.err(got, ref)
            row = {"frames": T, "after_layers": n, "max_abs_ref": float(np.abs(ref).max()), "rms_ref": float(np.sqrt(np.mean(ref * ref))),
                   "torch_half_vs_fp64": e_t, "hip_vs_fp64": e_h, "hip_over_torch_half_rms": e_h[0] / e_t[0], "hip_over_torch_half_max": e_h[1] / e_t[1]}
            res["cases"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
