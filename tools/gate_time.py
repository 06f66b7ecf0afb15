"""Cost of the realtime GUI's noise reduction on the device at production geometry (0.25 s block, 0.05 s crossfade, 2.5 s extra):
``TorchGateHIP`` per call (HIP events, p50 / p99 after warm-up) in both GUI call shapes -- I-NR: ``Lb + block`` samples against
the whole ``input_wav`` (gui.py:981-985); O-NR: ``block + Lb + search`` against ``output_buffer`` (gui.py:1015-1022) -- stationary
and non-stationary, at 48 / 44.1 / 40 kHz; the same-chip anchor ``torch.stft`` + ``torch.istft`` of the same shapes on PyTorch-ROCm
(the two transforms TorchGate runs on the signal plus the noise STFT, i.e. the reference's three rocFFT calls, without the ~20
small ops in between); and ``RealtimeStream.process`` per block (host wall time, synchronised, stub ``rvc``) with the boxes off,
I only, O only and both.  Writes profiles/gate_time.json.

    python tools/gate_time.py [--reps 200] [--blocks 100] [--out profiles/gate_time.json]
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


def _events(fn, reps, warmup=20):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) * 1e3)
    return round(float(np.percentile(ms, 50)), 2), round(float(np.percentile(ms, 99)), 2)


def time_gate(dev, sr, reps):
    import rvc_amd

    g = rvc_amd.stream_geometry(sr)
    zc, blk, Lb, Ls = g["zc"], g["block_frame"], g["sola_buffer_frame"], g["sola_search_frame"]
    n_fft, hop = 4 * zc, zc
    gen = torch.Generator().manual_seed(sr)
    buf = (0.1 * torch.randn(g["input_wav_len"], generator=gen)).to(dev)
    shapes = {"I": (buf[None, -Lb - blk:], buf[None]), "O": (buf[None, -(blk + Lb + Ls):].contiguous(), buf[None])}
    res = []
    win = torch.hann_window(n_fft, device=dev)
    for shape, (x, xn) in shapes.items():
        for ns in (False, True):
            tg = rvc_amd.TorchGateHIP(sr=sr, n_fft=n_fft, prop_decrease=0.9, nonstationary=ns).to(dev)
            p50, p99 = _events(lambda: tg(x, xn), reps)
            res.append(dict(samplerate=sr, n_fft=n_fft, shape=shape, n_x=int(x.shape[1]), n_xn=int(xn.shape[1]), nonstationary=ns,
                            frames_x=1 + int(x.shape[1]) // hop, frames_xn=1 + int(xn.shape[1]) // hop, us_p50=p50, us_p99=p99))

        def anchor(x=x, xn=xn):
            kw = dict(n_fft=n_fft, hop_length=hop, win_length=n_fft, window=win, center=True, return_complex=True, pad_mode="constant")
            X = torch.stft(x, **kw)
            torch.stft(xn, **kw)
            torch.istft(X, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=win, center=True)

        p50, p99 = _events(anchor, reps)
        res.append(dict(samplerate=sr, n_fft=n_fft, shape=shape, n_x=int(x.shape[1]), n_xn=int(xn.shape[1]),
                        anchor="torch.stft(x) + torch.stft(xn) + torch.istft (fp32, rocFFT)", us_p50=p50, us_p99=p99))
    return res


class _Stub:
    def __init__(self, tgt_sr, n, dev):
        self.tgt_sr = tgt_sr
        self.chunk = (0.2 * torch.randn(n, generator=torch.Generator().manual_seed(1))).to(dev)

    def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
        return self.chunk


def time_stream(dev, sr, I_nr, O_nr, blocks, warmup=10):
    import rvc_amd

    geo = rvc_amd.stream_geometry(sr)
    stub = _Stub(sr, geo["return_length"] * sr // 100, dev)
    rt = rvc_amd.RealtimeStream(stub, samplerate=sr, device=dev, I_noise_reduce=I_nr, O_noise_reduce=O_nr)
    x = (0.3 * np.random.default_rng(0).standard_normal((blocks + warmup, rt.block_frame))).astype(np.float32)
    ts = []
    for j in range(blocks + warmup):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        rt.process(x[j])
        torch.cuda.synchronize(dev)
        if j >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts = np.array(ts)
    return dict(samplerate=sr, I_noise_reduce=I_nr, O_noise_reduce=O_nr, blocks=blocks, p50_ms=round(float(np.percentile(ts, 50)), 4),
                p99_ms=round(float(np.percentile(ts, 99)), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gate_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gate = []
    for sr in (48000, 44100, 40000):
        gate += time_gate(dev, sr, a.reps)
    for r in gate:
        print("%5d Hz %s n_x %6d n_xn %6d %-28s p50 %8.1f us  p99 %8.1f us" % (
            r["samplerate"], r["shape"], r["n_x"], r["n_xn"], r.get("anchor", "nonstationary" if r.get("nonstationary") else "stationary")[:28],
            r["us_p50"], r["us_p99"]))
    streams = [time_stream(dev, 48000, i, o, a.blocks) for i, o in ((False, False), (True, False), (False, True), (True, True))]
    for s in streams:
        print("stream 48 kHz I %-5s O %-5s: p50 %.3f ms p99 %.3f ms" % (s["I_noise_reduce"], s["O_noise_reduce"], s["p50_ms"], s["p99_ms"]))
    res = dict(device=torch.cuda.get_device_name(dev), geometry="block 0.25 s, crossfade 0.05 s, extra 2.5 s",
               note="gate rows: HIP-event time per TorchGateHIP call (us); anchor rows: torch.stft of x and xn plus torch.istft of the "
                    "same shapes on PyTorch-ROCm; streams: host wall time per RealtimeStream.process block (stub rvc, synchronised)",
               gate=gate, streams=streams)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
