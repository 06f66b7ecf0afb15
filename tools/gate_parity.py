"""The worst error / bar ratio per stage of the spectral gate's edge cases (tests/gate_cases.py, run by tests/test_gpu_gate_edges.py) from
one MI355X run -> profiles/gate_edges_parity.json.  These numbers are RECORDED, not asserted: the bars are the oracle's
(oracle/gate_oracle.py), derived from each case's own data, and the tests hold the device to them.

    python tools/gate_parity.py [--out profiles/gate_edges_parity.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_edges_parity.json"))
    a = ap.parse_args()
    import gate_cases as gc
    import test_gpu_gate_edges as t

    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(dev), cases=len(gc.NAMES),
               what="worst observed error / derived bar per stage of rvcmi_glue_spectral_gate against oracle/gate_oracle.py on the edge "
                    "cases of tests/gate_cases.py (1.0 is the bar); recorded, not asserted")
    worst, differing, decisions = {}, 0, 0
    for name in gc.NAMES:
        q = t.stage_ratios(name, dev)
        c = gc.CASES[name]
        if not c.nonstat:
            differing += q.pop("mraw_differing")
            decisions += (c.B - len(gc.zero_rows(name))) * c.F * c.K
        for stage, v in q.items():
            if v >= worst.get(stage, (-1.0, None))[0]:
                worst[stage] = (v, name)
        print("%-20s " % name + "  ".join("%s %.3g" % kv for kv in q.items()))
    res["stationary_mask"] = dict(decisions=decisions, differing=differing)
    res["worst_error_over_bar"] = {k: dict(ratio=v, case=n) for k, (v, n) in worst.items()}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
