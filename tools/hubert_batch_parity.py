"""Records the whole-model parity of the batched HuBERT path: per item of each group of tests/hubert_batch_cases.py ``MODEL_GROUPS``, the RMS
error of the batched call and of the lone call against the fp64 CPU encoder fed with the item's own extractor rows (the measurement of
tests/test_gpu_hubert_batch.py, ``hubert_batch_cases.whole_model_errors``), and the same with the naive sample mask.

    python tools/hubert_batch_parity.py --out profiles/hubert_batch_parity.json
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_batch_parity.json"))
    a = ap.parse_args()
    import hubert_batch_cases as bc

    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "model": dict(bc.SMALL, dtype="float32"),
           "bar": "e_batch <= 2 * e_single + 1e-6 * ref_rms", "groups": [], "naive_mask": []}
    for key, naive in (("groups", False), ("naive_mask", True)):
        for lens in bc.MODEL_GROUPS[:1] if naive else bc.MODEL_GROUPS:
            items = bc.whole_model_errors(dev, lens, naive=naive)
            for e in items:
                e["ratio"] = e["e_batch"] / e["e_single"] if e["e_single"] else None
                e["within_bar"] = bool(bc.within_bar(e))
            res[key].append({"lens": list(lens), "items": items})
            print(json.dumps(res[key][-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
