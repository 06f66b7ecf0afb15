"""Times the batched HuBERT path against the per-item loop it replaces, in one process, the two alternating:

  * the extractor alone: ``HubertFrontHIP.forward`` once per item against one ``forward_ragged`` call on the padded group;
  * the whole model: a fairseq-shaped wrapper (tests/hubert_batch_cases.py ``FairseqShaped``) of transformers' HuBERT-base in half precision
    with random weights (cost only), ``extract_features`` once per item against one ``hubert.extract_features_batch`` call.

    python tools/hubert_batch_time.py --out profiles/hubert_batch_time.json

Shapes: 2, 8 and 64 items of 12 s, and a mixed group of 3 - 12 s.  Per shape: median and range over ``--repeats`` timed calls after
``--warmup`` untimed ones, device-synchronised host clock.  The verdict is "batch faster" / "loop faster" only when the two ranges are
disjoint, else "tie"; ``hubert.HUBERT_BATCH`` may default to on only if the batch is faster at EVERY shape.  The mixed group is also planned
with ``hubert.plan_groups`` at several ``max_waste`` and timed group by group, which is what ``HUBERT_BATCH_MAX_WASTE`` is set from.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from hubert_fe_time import alternate  # noqa: E402

S = 16000
MIXED = tuple(int(S * s) for s in (3, 4.5, 5, 6, 7.25, 8, 9.5, 10, 11, 12, 12, 3.5))
SHAPES = (("2x12s", (12 * S,) * 2), ("8x12s", (12 * S,) * 8), ("64x12s", (12 * S,) * 64), ("mixed_3-12s", MIXED))
WASTES = (0.0, 0.1, 0.25, 0.5, 1.0)


def verdict(loop_s, batch_s):
    if batch_s["max_ms"] < loop_s["min_ms"]:
        return "batch faster"
    if loop_s["max_ms"] < batch_s["min_ms"]:
        return "loop faster"
    return "tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_batch_time.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import hubert_batch_cases as bc
    import rvc_amd
    from rvc_amd import hubert
    from transformers import HubertConfig

    dev = torch.device("cuda:0")
    base = HubertConfig()
    model = bc.make_model(dev, seed=0, num_hidden_layers=base.num_hidden_layers, hidden_size=base.hidden_size, num_attention_heads=base.num_attention_heads,
                          intermediate_size=base.intermediate_size, num_conv_pos_embeddings=base.num_conv_pos_embeddings,
                          num_conv_pos_embedding_groups=base.num_conv_pos_embedding_groups).half()
    assert rvc_amd.accelerate_hubert(model) == 1 and hubert.batch_capable(model)
    fe = model.feature_extractor
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "extractor": [], "model": [], "planned": [],
           "method": "same process, alternating loop / batch, device-synchronised host clock; extractor = HubertFrontHIP.forward per item vs one forward_ragged "
                     "(padding the batch not included); model = fairseq-shaped HuBERT-base .half(), random weights, extract_features per item vs one "
                     "extract_features_batch (padding and masks included), output_layer 12"}

    def loop_model(items):
        return [model.extract_features(source=w.view(1, -1), padding_mask=torch.zeros(1, w.shape[0], dtype=torch.bool, device=dev), output_layer=12)[0]
                for w in items]

    with torch.no_grad():
        for label, lens in SHAPES:
            items = [(0.1 * torch.randn(n, device=dev)).half() for n in lens]
            x = torch.zeros(len(lens), max(lens), device=dev, dtype=torch.float16)
            for i, w in enumerate(items):
                x[i, :lens[i]] = w
            lo, ba = alternate(lambda: [fe(w.view(1, -1)) for w in items], lambda: fe.forward_ragged(x, lens), a.warmup, a.repeats)
            row = {"label": label, "items": len(lens), "samples": sum(lens), "padded_samples": len(lens) * max(lens), "loop": lo, "batch": ba,
                   "verdict": verdict(lo, ba), "speedup_median": lo["median_ms"] / ba["median_ms"], "workspace_bytes": fe.workspace_bytes_ragged(len(lens), max(lens))}
            res["extractor"].append(row)
            print(json.dumps(row), flush=True)
            lo, ba = alternate(lambda: loop_model(items), lambda: hubert.extract_features_batch(model, items, 12), a.warmup, a.repeats)
            row = {"label": label, "items": len(lens), "samples": sum(lens), "padded_samples": len(lens) * max(lens), "loop": lo, "batch": ba,
                   "verdict": verdict(lo, ba), "speedup_median": lo["median_ms"] / ba["median_ms"]}
            res["model"].append(row)
            print(json.dumps(row), flush=True)
        items = [(0.1 * torch.randn(n, device=dev)).half() for n in MIXED]
        for w in WASTES:
            groups = hubert.plan_groups(MIXED, w)

            def planned():
                out = []
                for g in groups:
                    out += loop_model([items[i] for i in g]) if len(g) < hubert.HUBERT_BATCH_MIN_ITEMS else hubert.extract_features_batch(model, [items[i] for i in g], 12)
                return out

            lo, ba = alternate(lambda: loop_model(items), planned, a.warmup, a.repeats)
            row = {"max_waste": w, "groups": [len(g) for g in groups], "loop": lo, "batch": ba, "verdict": verdict(lo, ba), "speedup_median": lo["median_ms"] / ba["median_ms"]}
            res["planned"].append(row)
            print(json.dumps(row), flush=True)
    res["all_batch_faster"] = all(r["verdict"] == "batch faster" for r in res["extractor"] + res["model"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
