"""csrc/unet.hip layer by layer against the fp16-operand fp64 oracle (oracle/unet_oracle.py), teacher-forced, over the sweep case of
tests/unet_cases.py, once:

    python tools/unet_layer_parity.py --out profiles/unet_layer_parity.json

Per primitive and per pass (``ksplit=0``: the forward's own K split at this size, ``ksplit=1``: the fused epilogue) the share of elements
``rvcmi_unet_debug_op`` stores that are not fp16(y), the elements outside the elementwise bound, and the largest
(|got - y| - spacing16 / 2) / A -- how far the accumulation must have moved y, in units of the sum of magnitudes A.  Beside them the CPU
floors: the same figures for the oracle evaluated in float32, in torch's summation order and in the kernel's chunked / split order permuted
(there ``raw`` is |y32 - y| / A before the fp16 store, which the GPU's output no longer shows).  Then the whole network and its skip tensors
against the rounded oracle at the bars of tests/unet_cases.py.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import unet_cases as uc  # noqa: E402
from oracle import unet_oracle as uo  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    layers = []
    top = {"ksplit0": {"flips": 0.0, "excess": 0.0, "violations": 0}, "ksplit1": {"flips": 0.0, "excess": 0.0, "violations": 0},
           "cpu_f32": {"flips": 0.0, "raw": 0.0}, "cpu_permuted": {"flips": 0.0, "raw": 0.0}}
    for r in uc.sweep_trace():
        B, Cin, H, W = r["x0"].shape
        Cin += r["x1"].shape[1] if r["x1"] is not None else 0
        rec = {"layer": r["name"], "kind": r["kind"], "shape": list(r["y"].shape), "Cin": Cin,
               "forward_ksplit": uo.forward_ksplit(r["kind"], Cin, r["y"].shape[1], B * H * W)}
        for ks in (0, 1):
            ck = uc.prim_check(uc.run_record(dev, r, ks), r)
            rec["ksplit%d" % ks] = {k: ck[k] for k in ("flips", "violations", "excess")}
            t = top["ksplit%d" % ks]
            t["flips"], t["excess"], t["violations"] = max(t["flips"], ck["flips"]), max(t["excess"], ck["excess"]), t["violations"] + ck["violations"]
        for tag, kw in (("cpu_f32", {}), ("cpu_permuted", dict(perturb=dict(seed=5, split=True)))):
            y32 = uo.eval_prim(r, "f32", **kw)
            ck = uc.prim_check(y32.double() if r["kind"] == uo.K_HEAD else y32.half().double(), r)
            raw = float(((y32.double() - r["y"]).abs() / r["A"].clamp_min(1e-300)).max())
            rec[tag] = {"flips": ck["flips"], "violations": ck["violations"], "excess": ck["excess"], "raw": raw}
            top[tag]["flips"], top[tag]["raw"] = max(top[tag]["flips"], ck["flips"]), max(top[tag]["raw"], raw)
        print(json.dumps(rec), flush=True)
        layers.append(rec)
    whole = []
    for c in uc.WHOLE:
        want, got = uc.whole_case(c), uc.run_whole(dev, c)
        for k in sorted(want):
            b = want[k]
            rms, mx = uc.err(got[k], b["y"])
            rec = {"case": uc.case_id(c), "stage": k, "floor_rms": b["floor_rms"], "floor_max": b["floor_max"], "bar_rms": b["bar_rms"], "bar_max": b["bar_max"],
                   "hip_rms": rms, "hip_max": mx, "within_bars": bool(rms <= b["bar_rms"] and mx <= b["bar_max"])}
            print(json.dumps(rec), flush=True)
            whole.append(rec)
    out = {"reference": "oracle/unet_oracle.forward, float64, the rounding points of csrc/unet_kernels.hpp; every primitive fed the oracle's own fp16 operands",
           "sweep_case": uc.case_id(uc.SWEEP), "gamma": uc.GAMMA, "flip_cap": uc.FLIP_CAP,
           "bound": "|got - y| <= spacing16(max(|got|, |y|)) / 2 + gamma * A; at most flip_cap of a primitive's elements differ from fp16(y)",
           "largest": top, "layers": layers,
           "whole": {"bars": "bar_rms = %.1f * floor_rms + ulp16(max |y|) / sqrt(n), bar_max = %.1f * floor_max + ulp16(max |y|)" % (uc.F_RMS, uc.F_MAX),
                     "stages": whole}}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("largest:", json.dumps(top))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
