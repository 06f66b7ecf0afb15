"""Per-block cost of RealtimeStream.process (the realtime GUI's audio_infer DSP on the device) with a stub ``rvc`` that returns a
preallocated device chunk, so only the block's own work is timed: host wall time per block (p50 / p99, synchronised), plus the
HIP-event time of the sin^2 SOLA call against the phase-vocoder one.  Writes profiles/rt_block_time.json.

    python tools/rt_block_time.py [--blocks 200] [--out profiles/rt_block_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Stub:
    def __init__(self, tgt_sr, n, dev):
        self.tgt_sr = tgt_sr
        self.chunk = (0.2 * torch.randn(n, generator=torch.Generator().manual_seed(1))).to(dev)

    def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
        return self.chunk


def time_stream(dev, samplerate, tgt_sr, use_pv, rms_mix_rate, blocks, warmup=20):
    import rvc_amd

    geo = rvc_amd.stream_geometry(samplerate)
    stub = _Stub(tgt_sr, geo["return_length"] * tgt_sr // 100, dev)
    rt = rvc_amd.RealtimeStream(stub, samplerate=samplerate, rms_mix_rate=rms_mix_rate, use_pv=use_pv, device=dev)
    rng = np.random.default_rng(0)
    x = (0.3 * rng.standard_normal((blocks + warmup, rt.block_frame))).astype(np.float32)
    ts = []
    for j in range(blocks + warmup):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rt.process(x[j])
        torch.cuda.synchronize(dev)
        if j >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return dict(samplerate=samplerate, tgt_sr=tgt_sr, use_pv=use_pv, rms_mix_rate=rms_mix_rate, block_frame=rt.block_frame,
                sola_buffer_frame=rt.sola_buffer_frame, blocks=blocks, p50_ms=round(float(np.percentile(ts, 50)), 4),
                p99_ms=round(float(np.percentile(ts, 99)), 4), mean_ms=round(float(ts.mean()), 4))


def time_sola(dev, Lb, reps=200):
    import rvc_amd

    Ls, blk = Lb // 4, 25 * (Lb // 4)
    g = torch.Generator().manual_seed(2)
    wav = (0.3 * torch.randn(Ls + blk + Lb, generator=g)).to(dev)
    buf = (0.3 * torch.randn(Lb, generator=g)).to(dev)
    fi = (torch.sin(0.5 * np.pi * torch.linspace(0.0, 1.0, Lb)) ** 2).to(dev)
    fo = 1 - fi
    res = {}
    for name, pv in (("fade", False), ("pv", True)):
        for _ in range(10):
            rvc_amd.glue.sola(wav, buf, fi, fo, blk, Ls, use_pv=pv)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(reps):
            e0.record()
            rvc_amd.glue.sola(wav, buf, fi, fo, blk, Ls, use_pv=pv)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) * 1e3)
        res[name + "_us_p50"] = round(float(np.percentile(ms, 50)), 2)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record()
        rvc_amd.glue.phase_vocoder(buf, wav[:Lb], fo, fi)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) * 1e3)
    res["phase_vocoder_us_p50"] = round(float(np.percentile(ms, 50)), 2)
    return dict(n=Lb, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_block_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    streams = [time_stream(dev, sr, tsr, pv, mix, a.blocks)
               for sr, tsr, pv, mix in ((40000, 40000, False, 1.0), (40000, 40000, False, 0.0), (40000, 40000, True, 1.0),
                                        (40000, 40000, True, 0.0), (48000, 48000, True, 0.0))]
    sola = [time_sola(dev, Lb) for Lb in (1600, 1920)]
    res = dict(device=torch.cuda.get_device_name(dev), note="host wall time per RealtimeStream.process block (stub rvc, synchronised); "
               "HIP-event time per glue.sola call (fade vs pv) and per glue.phase_vocoder call", streams=streams, sola=sola)
    for s in streams:
        print("stream %5d Hz pv %-5s mix %.1f: p50 %.3f ms p99 %.3f ms" % (s["samplerate"], s["use_pv"], s["rms_mix_rate"], s["p50_ms"], s["p99_ms"]))
    for s in sola:
        print("sola n=%d: fade %.1f us, pv %.1f us, phase_vocoder %.1f us" % (s["n"], s["fade_us_p50"], s["pv_us_p50"], s["phase_vocoder_us_p50"]))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
