"""Times HuBERT's convolutional feature extractor: torch's ``.half()`` module (MIOpen) against ``HubertFrontHIP`` with the same weights, in one
process, the two alternating, and the whole ``transformers.HubertModel`` (random weights: cost only) with and without the swap.

    python tools/hubert_fe_time.py --out profiles/hubert_fe_time.json

Per shape: median and range over ``--repeats`` timed calls after ``--warmup`` untimed ones, device-synchronised host clock.  The verdict is
"hip faster" / "torch faster" only when the two ranges are disjoint, else "tie".
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (label, B, N): one second, the realtime window, a 12 s clip, a 71 s clip, a group of eight 12 s clips
SHAPES = (("1s", 1, 16000), ("realtime_window", 1, 44000), ("12s", 1, 192000), ("71s", 1, 71 * 16000), ("8x12s", 8, 192000))
MODEL_SHAPES = (("realtime_window", 1, 44000), ("12s", 1, 192000))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def verdict(torch_s, hip_s):
    if hip_s["max_ms"] < torch_s["min_ms"]:
        return "hip faster"
    if torch_s["max_ms"] < hip_s["min_ms"]:
        return "torch faster"
    return "tie"


def alternate(fa, fb, warmup, repeats):
    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _ in range(warmup):
        fa()
        fb()
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(fa))
        b.append(timed(fb))
    return summary(a), summary(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hubert_fe_time.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import rvc_amd
    from transformers import HubertConfig, HubertModel

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = HubertModel(HubertConfig()).eval().half().to(dev)
    fe = model.feature_extractor
    hip = rvc_amd.HubertFrontHIP.from_module(fe)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup, "shapes": [], "model": [],
           "method": "same process, alternating torch / HIP, device-synchronised host clock; torch = HubertFeatureEncoder.half() (MIOpen), "
                     "HIP = HubertFrontHIP.forward incl. its output allocation; model = HubertModel.half() forward, random weights"}
    with torch.no_grad():
        for label, B, N in SHAPES:
            x = (0.1 * torch.randn(B, N, device=dev)).half()
            t, h = alternate(lambda: fe(x), lambda: hip(x), a.warmup, a.repeats)
            L = [(N - 10) // 5 + 1]
            for k in (3, 3, 3, 3, 2, 2):
                L.append((L[-1] - k) // 2 + 1)
            flops = 2.0 * B * 512 * (10 * L[0] + sum(512 * k * l for k, l in zip((3, 3, 3, 3, 2, 2), L[1:])))
            row = {"label": label, "B": B, "N": N, "frames": L[-1], "torch_half": t, "hip": h, "verdict": verdict(t, h),
                   "speedup_median": t["median_ms"] / h["median_ms"], "flops": flops, "hip_tflops": flops / h["median_ms"] / 1e9,
                   "workspace_bytes": hip.workspace_bytes(B, N)}
            res["shapes"].append(row)
            print(json.dumps(row), flush=True)
        for label, B, N in MODEL_SHAPES:
            x = (0.1 * torch.randn(B, N, device=dev)).half()

            def run_off():
                rvc_amd.restore_hubert(model)
                return model(x).last_hidden_state

            def run_on():
                if not isinstance(model.feature_extractor, rvc_amd.HubertFrontHIP):
                    model.feature_extractor = hip
                return model(x).last_hidden_state

            object.__setattr__(hip, "_original", fe)
            t, h = alternate(run_off, run_on, a.warmup, a.repeats)
            rvc_amd.restore_hubert(model)
            row = {"label": label, "B": B, "N": N, "switch_off": t, "switch_on": h, "verdict": verdict(t, h), "speedup_median": t["median_ms"] / h["median_ms"]}
            res["model"].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
