"""Time of the f0 of a GROUP of files with the whole RMVPE estimator on HIP: one ``RMVPEHIP.f0`` call per file (what ``convert_files`` did)
against ONE ragged ``RMVPEHIP.f0_batch`` call for the group.

    python tools/rmvpe_batch_time.py --out profiles/rmvpe_batch_time.json [--repeats 12]

Both legs run in ONE process on the same object, alternating per-file loop / batch, every set warmed up first, timed with a device-synchronised
host clock; median and range of ``--repeats`` runs per leg.  Sets: 2, 8 and 64 clips of 10 s, and 64 files of 3 .. 30 s drawn with a fixed seed.
A set whose ranges overlap is a tie; the batch becomes the default for a group size only where its range lies wholly below the loop's.  For
the 64 x 10 s set also the stage split of the batch (mel / U-Net / GRU / head / decode, a synchronising clock after each stage: their sum is
above the unsplit time by the lost overlap).  Seeded weights (the stand-in objects of tests/rmvpe_cases.py), ``is_half``.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rmvpe_cases as rc  # noqa: E402

SR = 16000


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def leg(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def verdict(batch, loop):
    if batch["max_ms"] < loop["min_ms"]:
        return "f0_batch faster"
    if loop["max_ms"] < batch["min_ms"]:
        return "per-file loop faster"
    return "a tie"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import rvc_amd

    dev = torch.device("cuda:0")
    hip = rvc_amd.RMVPEHIP.from_reference(rc.RmvpeStandIn(dev, True))
    base = (rc.signal("voiced", 31 * SR) + 0.05 * torch.randn(31 * SR, generator=torch.Generator().manual_seed(0))).to(dev)
    g = torch.Generator().manual_seed(1)
    mixed = [int(n) for n in torch.randint(3 * SR, 30 * SR + 1, (64,), generator=g)]
    sets = [("2 x 10 s", [10 * SR] * 2), ("8 x 10 s", [10 * SR] * 8), ("64 x 10 s", [10 * SR] * 64), ("64 files of 3-30 s (seed 1)", mixed)]
    res = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, warmup=a.warmup, sets=[],
               method="same process and object, alternating (a) one RMVPEHIP.f0 call per file and (b) one RMVPEHIP.f0_batch call for the group, "
                      "device-synchronised host clock around each; seeded weights, is_half, key 0.  The batch leg includes what f0_batch does per call and "
                      "f0 does not: six buffers from torch's caching allocator, the blocking upload of the row offsets and one mel launch per "
                      "file (f0 keeps its buffers per shape only up to 512 rows, so at 10 s both legs allocate)")
    for name, lengths in sets:
        wavs = [base[i * 997: i * 997 + n].clone() for i, n in enumerate(lengths)]  # (another stretch of the signal per file)
        p_lens = [n // rc.HOP for n in lengths]

        def loop():
            return [hip.f0(w, p, 0) for w, p in zip(wavs, p_lens)]

        def batch():
            return hip.f0_batch(wavs, p_lens, 0)

        for _ in range(a.warmup):
            one, many = loop(), batch()
        worst = max(float((x[1] - y[1]).abs().max() / max(float(x[1].max()), 1.0)) for x, y in zip(one, many))
        ms = dict(loop=[], batch=[])
        for _ in range(a.repeats):
            ms["loop"].append(timed(loop, dev))
            ms["batch"].append(timed(batch, dev))
        lo, ba = leg(ms["loop"]), leg(ms["batch"])
        frames = [n // rc.HOP + 1 for n in lengths]
        row = dict(set=name, files=len(lengths), seconds_of_audio=sum(lengths) / SR, frames=sum(frames), packed_rows=sum(rc.pad32(t) for t in frames),
                   per_file_loop=lo, f0_batch=ba, verdict=verdict(ba, lo), speedup_median=lo["median_ms"] / ba["median_ms"],
                   per_file_ms_loop=lo["median_ms"] / len(lengths), per_file_ms_batch=ba["median_ms"] / len(lengths),
                   pitchf_max_rel_difference_batch_vs_loop=worst)
        if name == "64 x 10 s":
            split = {}
            for _ in range(a.repeats):
                stamps = []

                def mark(stage):
                    torch.cuda.synchronize(dev)
                    stamps.append((stage, time.perf_counter()))

                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                xs = hip._wavs(wavs)
                sal, off, fr = hip._salience_ragged(xs, mark)
                out = [rvc_amd.glue.rmvpe_f0(sal[o: o + t], p, 0, 0.03) for o, t, p in zip(off, fr, p_lens)]
                mark("decode")
                for stage, t in stamps:
                    split.setdefault(stage, []).append((t - t0) * 1e3)
                    t0 = t
            row["stage_split_batch_ms"] = {k: leg(v) for k, v in split.items()}
        print(json.dumps(row), flush=True)
        res["sets"].append(row)
        del wavs
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
