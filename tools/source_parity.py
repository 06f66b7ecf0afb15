"""The generator's excitation and realtime resampling against oracle/source_oracle.py over the case table of tests/source_cases.py, once:

    python tools/source_parity.py --out profiles/source_parity.json

Per "har" case: how many samples lie outside the interval, the worst distance from its centre in float32 ulps and the item, frame and sample where it occurs (and the
first samples outside, should there be any: where ``har`` differs).  Per n_res case: the share of interpolated samples bit-equal to each admissible rounding of the
source index and to torch's float32 F.interpolate.  Per z case: the "pre" tap against the oracle on each candidate.  Records for a later reader -- is 4 ulp generous,
which rounding does the compiler emit for interp_linear_at -- no bar is taken from them.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import source_cases as sc  # noqa: E402
from oracle import source_oracle as so  # noqa: E402


def _short(v):
    if isinstance(v, float):
        return float("%.4g" % v)
    if isinstance(v, dict):
        return {k: _short(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_short(x) for x in v]
    return v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {"har": [], "har_n_res": [], "z_n_res": []}
    for c in sc.HAR_CASES:
        out["har"].append(_short(sc.device_har_case(c, dev)[0]))
        print(json.dumps(out["har"][-1]), flush=True)
    for c in sc.INTERP_CASES + sc.INTERP_IDENTITY:
        out["har_n_res"].append(_short(sc.device_interp_case(c, dev)[0]))
        print(json.dumps(out["har_n_res"][-1]), flush=True)
    for c in sc.INTERP_Z_CASES:
        out["z_n_res"].append(_short(sc.device_z_case(c, dev)))
        print(json.dumps(out["z_n_res"][-1]), flush=True)
    worst = max(out["har"], key=lambda r: r["worst_ulp"])
    head = {"device": torch.cuda.get_device_name(dev),
            "har": "debug_tap('har') of the fp16-operand handle against source_oracle.har_interval: sinf +-%d ulp, tanhf +-%d ulp, the phase and every other step bit-determined; "
                   "worst_ulp = the largest |har - centre| in float32 ulps of the centre" % (so.L_SIN, so.L_TANH),
            "har_n_res": "debug_tap('har', n_res=) against source_oracle.interp_admissible of the device's own plain tap; equal_<index> = share of samples bit-equal to that rounding "
                         "of the source index with the output rounded once",
            "z_n_res": "debug_tap('pre', n_res=) of the fp32-operand handle against the fp64 conv_pre + cond on each admissible interpolation of z, bars of tests/nsf_cases.py",
            "samples_outside_any_interval": sum(r["outside"] for r in out["har"]), "samples_outside_any_band": sum(r.get("outside", 0) for r in out["har_n_res"]),
            "worst_ulp_from_centre": {"ulp": worst["worst_ulp"], "case": worst["case"], "at": worst["worst_at"]}}
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(_short(v))) for k, v in head.items()))
        for k, recs in out.items():
            f.write(',\n %s: [\n' % json.dumps(k + "_cases") + ",\n".join("  " + json.dumps(r) for r in recs) + "\n ]")
        f.write("\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
