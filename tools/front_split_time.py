"""Times the synthesizer front in its fp16 and fp16x2 operand modes, alone and inside the whole ``infer`` (fp16 generator), at B = 1 and
B = 16, T = 1198 -- and next to them the torch fp32 ``enc_p`` + ``flow`` that the fp16x2 front replaces under ``operand="fp32"``:
oracle/front_oracle.py (the same torch ops as the reference modules, as a function) run on the GPU.

    python tools/front_split_time.py --out profiles/front_split_time.json

One process, the legs of a shape alternating; per leg the median and range over ``--repeats`` timed calls after ``--warmup`` untimed
ones, device-synchronised host clock.  A verdict is "faster" / "slower" only when the two ranges are disjoint, else "tie".
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


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "n": len(ms)}


def verdict(a, b):
    """a against b"""
    if a["max_ms"] < b["min_ms"]:
        return "faster"
    if b["max_ms"] < a["min_ms"]:
        return "slower"
    return "tie"


def alternate(legs, warmup, repeats):
    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3

    for _ in range(warmup):
        for f in legs.values():
            f()
    ms = {k: [] for k in legs}
    for _ in range(repeats):
        for k, f in legs.items():
            ms[k].append(timed(f))
    return {k: summary(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "front_split_time.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--T", type=int, default=1198)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 16])
    a = ap.parse_args()
    import rvc_amd
    from oracle import front_oracle, nsf_oracle, synth
    from oracle.front_oracle import FrontConfig

    assert torch.cuda.is_available(), "this tool measures on the GPU"
    gpu = torch.device("cuda:0")
    T = a.T
    fcfg, cfg = FrontConfig(), nsf_oracle.CONFIGS["v2_48k"]
    wf, wd = synth.make_front_weights(fcfg, 1234), synth.make_dec_weights(cfg, 1234)
    wg = {k: v.to(gpu) for k, v in wf.items()}
    res = {"device": torch.cuda.get_device_name(0), "T": T, "repeats": a.repeats, "warmup": a.warmup, "shapes": [],
           "method": "one process, legs alternating, device-synchronised host clock; front = FrontHIP.forward incl. its output allocation; "
                     "torch_fp32 = oracle/front_oracle.infer_front on the GPU (torch fp32 ops of enc_p + z_p + flow); whole infer = "
                     "rvc_amd.infer_hip with the fp16 generator"}

    class Net:
        def __init__(self, dec):
            self.emb_g = lambda sid: wg["emb_g.weight"][sid]
            self.dec = dec

    for B in a.batches:
        phone = synth.make_phone(B, T, 768, 1234).to(gpu)
        pitchf = synth.make_f0(B, T)
        pitch = synth.make_pitch(pitchf).to(gpu)
        pitchf = pitchf.to(gpu)
        lengths = torch.full((B,), T, device=gpu)
        sid = (torch.arange(B) % 7).to(gpu)
        g = wg["emb_g.weight"][sid].unsqueeze(-1)
        nz = torch.randn(B, 192, T, generator=torch.Generator().manual_seed(8)).to(gpu)
        noise = nsf_oracle.reference_noise(B, T, cfg.upp, 114514).to(gpu)
        fronts = {op: rvc_amd.FrontHIP(vars(fcfg), wf, device=gpu, operand=op, max_B=B, max_T=T) for op in ("fp16", "fp16x2")}
        dec = rvc_amd.NSFGeneratorHIP(vars(cfg), wd, device=gpu, operand="fp16", max_B=B, max_T=T)

        def torch_fp32():
            with torch.no_grad(), torch.device(gpu):
                z, m1, _ = front_oracle.infer_front(fcfg, wg, phone, pitch, lengths, sid, nz)
                return z * m1

        legs = {"fp16": lambda: fronts["fp16"](phone, pitch, lengths, g, 0, noise=nz),
                "fp16x2": lambda: fronts["fp16x2"](phone, pitch, lengths, g, 0, noise=nz),
                "torch_fp32": torch_fp32}
        fr = alternate(legs, a.warmup, a.repeats)
        whole = alternate({op: (lambda f=f: rvc_amd.infer_hip(Net(dec), f, phone, lengths, sid, pitch, pitchf, noise_zp=nz, noise_dec=noise))
                           for op, f in fronts.items()}, a.warmup, a.repeats)
        row = {"B": B, "T": T, "front": fr, "whole_infer": whole,
               "front_fp16x2_over_fp16_median": fr["fp16x2"]["median_ms"] / fr["fp16"]["median_ms"],
               "front_fp16x2_against_torch_fp32": verdict(fr["fp16x2"], fr["torch_fp32"]),
               "front_fp16x2_against_fp16": verdict(fr["fp16x2"], fr["fp16"]),
               "whole_fp16x2_over_fp16_median": whole["fp16x2"]["median_ms"] / whole["fp16"]["median_ms"],
               "whole_fp16x2_against_fp16": verdict(whole["fp16x2"], whole["fp16"]),
               "workspace_bytes": {op: f.workspace_bytes for op, f in fronts.items()}}
        res["shapes"].append(row)
        print(json.dumps(row), flush=True)
        del fronts, dec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
