"""The generator's kernels against the per-layer fp16-operand fp64 oracle (oracle/nsf_layer_oracle.py) over the case table of tests/nsf_cases.py, once:

    python tools/nsf_parity.py --out profiles/nsf_parity.json

Per case: the ResBlock path every stage ran on (``paths``, with ``plan`` the forward's own report of it: ``gen.last_plan()``), and per layer the error of the device's tap against the oracle applied
to the device's previous tap, the floor (the oracle's float32 evaluation against float64 on the same input), the bars and the ratios.  Needs a GPU.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nsf_cases as nc  # noqa: E402


def _short(v):
    """floats to 4 significant digits (the file holds some 500 layer records)"""
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
    cases = []
    for c, items in [(c, False) for c in nc.TABLE] + [(c, True) for c in nc.BATCH_CASES]:
        rec = _short(nc.device_case(c, dev, items=items)[0])
        print(json.dumps(rec), flush=True)
        cases.append(rec)
    worst = {}
    for rec in cases:
        for e in rec["layers"]:
            k = nc.kind_of(e["layer"])
            for key in ("rms", "max"):
                share = e[key] / e["bar_" + key]
                if share > worst.get((k, key), (0.0, None))[0]:
                    worst[(k, key)] = (share, "%s %s" % (rec["case"], e["layer"]))
    out = {"paths": "as the compared forward reported them (plan: rvcmi_nsf_last_plan); FULL<n>: k_rb_full with n-row tiles; the profiler's kernel names agree",
           "reference": "oracle/nsf_layer_oracle.Layers, float64, operands and streams rounded where the kernels round; each layer fed the device's own previous tap",
           "floor": "the same layer in float32 against float64 on the same input; bar = FACTOR * floor + one ulp (fp16 or fp32, as the tap is stored) at max |y| "
                    "(over sqrt(n) for RMS); FACTOR = %s" % json.dumps(nc.FACTOR),
           "largest_share_of_a_bar": {"%s_%s" % k: {"share": v[0], "where": v[1]} for k, v in sorted(worst.items())},
           "all_within_bars": all(e["within_bars"] for rec in cases for e in rec["layers"]), "cases": cases}
    with open(args.out, "w") as f:
        f.write("{\n" + ",\n".join(' %s: %s' % (json.dumps(k), json.dumps(_short(v))) for k, v in out.items() if k != "cases"))
        f.write(',\n "cases": [\n' + ",\n".join("  " + json.dumps(rec) for rec in cases) + "\n ]\n}\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
