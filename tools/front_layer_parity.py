"""The front in its default arithmetic, segment by segment against the rounded float64 oracle, measured on the GPU: every case of
tests/front_layer_cases.py (the table of tests/test_gpu_front_layers.py), and per case, segment and launch form the error, the floor (the input's own and
the one the bar is built on), the bars and the forms observed.

    python tools/front_layer_parity.py --out profiles/front_layer_parity.json

A case whose checks fail is recorded with the message and the run goes on; any other error (a HIP error among them) ends the run at once.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


COLUMNS = ("segment", "rms", "max", "floor_rms", "floor_max", "eff_rms", "eff_max", "bar_rms", "bar_max", "ties", "ties_flipped")


def sig4(v):
    return float("%.4g" % v) if isinstance(v, float) else v


def write(res, path):
    """One case per line, a segment as one row of ``COLUMNS`` (floor_* = the input's own floor, eff_* = the floor the bar is built on, ties / ties_flipped =
    layer<i>'s near-ties of the hidden activation and how many the device rounded away from nearest), figures to 4 digits."""
    cases = res.pop("cases")
    head = {**res, "columns": list(COLUMNS), "all_within_bars": all(s["within_bars"] for c in cases for s in c.get("segments", ())) and
            not any("failed_check" in c for c in cases)}
    with open(path, "w") as f:
        f.write("{\n")
        for k, v in head.items():
            f.write(" %s: %s,\n" % (json.dumps(k), json.dumps(json.loads(json.dumps(v), parse_float=lambda t: sig4(float(t))))))
        f.write(' "cases": [\n')
        for i, c in enumerate(cases):
            row = {k: v for k, v in c.items() if k not in ("segments", "kernels")}
            row["outside_bars"] = [s["segment"] for s in c.get("segments", ()) if not s["within_bars"]]
            row["segments"] = [[sig4(s[k]) for k in COLUMNS] for s in c.get("segments", ())]
            f.write("  %s%s\n" % (json.dumps(row), "," if i + 1 < len(cases) else ""))
        f.write(" ]\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "front_layer_parity.json"))
    ap.add_argument("--only", default="", help="substring of the case names to run")
    a = ap.parse_args()
    import front_layer_cases as fc

    assert torch.cuda.is_available(), "this tool measures on the GPU"
    gpu = torch.device("cuda:0")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    res = {"device": torch.cuda.get_device_name(0), "factor": fc.FACTOR, "perturb_worst_cpu": fc.PERTURB_WORST, "cases": []}
    worst = {}
    for c in fc.TABLE + fc.BATCH_CASES:
        if a.only not in c.name:
            continue
        try:
            rec = fc.device_case(c, gpu)[0]
        except AssertionError as e:
            rec = {"case": c.name, "failed_check": str(e)}
        res["cases"].append(rec)
        for s in rec.get("segments", ()):
            k = fc.kind_of(s["segment"])
            w = worst.setdefault(k, {"rms_ratio": 0.0, "max_ratio": 0.0, "bar_share": 0.0, "outside_bars": []})
            w["rms_ratio"] = max(w["rms_ratio"], s["rms_ratio"] or 0.0)
            w["max_ratio"] = max(w["max_ratio"], s["max_ratio"] or 0.0)
            w["bar_share"] = max(w["bar_share"], s["rms"] / s["bar_rms"], s["max"] / s["bar_max"])
            if not s["within_bars"]:
                w["outside_bars"].append("%s/%s" % (c.name, s["segment"]))
        print(json.dumps({"case": c.name, "failed_check": rec.get("failed_check"),
                          "segments": {s["segment"]: [round(s["rms"] / s["bar_rms"], 3), round(s["max"] / s["bar_max"], 3)] for s in rec.get("segments", ())}}), flush=True)
    res["largest_ratio_to_the_floor_used"] = worst
    print(json.dumps(worst), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write(res, a.out)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
