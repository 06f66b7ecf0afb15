"""Cost of the quiet-point search that cuts a long input (infer/modules/vc/pipeline.py:219-236), host loop against device search,
for 70 s / 305 s / 1200 s inputs (``long_input`` of tools/make_golden_cuts.py) at the (x_query, x_center, x_max) = (10, 60, 65)
geometry.  After a warm-up of each shape, alternating the two in one process:

  (a) host:    ``pipeline._cut_points`` (np.pad + 160 numpy passes over the whole file), host wall clock;
  (b) device:  as ``_prepare_file`` runs it (``pipeline._device_cuts``): upload of the fp64 signal + the two kernels + the
               synchronising read-back of the cuts, host wall clock ending in that read-back;
  (c) kernels: the two launches alone, HIP events, the signal already resident.

Medians and spread (min, max) in ms; the two must give the same cuts.  Writes profiles/cut_points_time.json.

    python tools/cut_points_time.py [--reps 10] [--out profiles/cut_points_time.json]
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from make_golden_cuts import long_input  # noqa: E402

SR = 16000


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3), "max_ms": round(float(np.max(ms)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seconds", type=int, nargs="+", default=[70, 305, 1200])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cut_points_time.json"))
    args = ap.parse_args()
    import rvc_amd
    import rvc_amd.pipeline as rp

    dev = torch.device("cuda:0")
    state = types.SimpleNamespace(window=160, t_query=10 * SR, t_center=60 * SR, t_max=65 * SR)
    rows = []
    for secs in args.seconds:
        audio = long_input(1000 + secs, secs * SR)

        def host():
            t0 = time.perf_counter()
            r = rp._cut_points(state, audio, np.pad(audio, (80, 80), mode="reflect"))
            return r, (time.perf_counter() - t0) * 1e3

        def device():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            r = rp._device_cuts(state, audio, dev)[0]  # ends in .tolist(): the synchronising read-back
            return r, (time.perf_counter() - t0) * 1e3

        a64 = torch.from_numpy(audio).to(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        L = rvc_amd._lib.lib()
        ncuts = rvc_amd.glue.cut_count(audio.shape[0], state.t_center)
        cuts = torch.empty(ncuts, device=dev, dtype=torch.int64)
        scratch = torch.empty(int(L.rvcmi_glue_cut_points_scratch_bytes(audio.shape[0], 160, state.t_center, state.t_query)), device=dev,
                              dtype=torch.uint8)

        def kernels():
            e0.record()
            rvc_amd._lib.check(L.rvcmi_glue_cut_points(rvc_amd._lib.ptr(a64), audio.shape[0], 160, state.t_center, state.t_query,
                                                       rvc_amd._lib.ptr(cuts), ncuts, None, rvc_amd._lib.ptr(scratch),
                                                       rvc_amd._lib.stream_ptr(dev)))
            e1.record()
            e1.synchronize()
            return cuts.tolist(), e0.elapsed_time(e1)

        want = host()[0]  # warm-up of each, and they agree
        assert device()[0] == want and kernels()[0] == want and len(want) == ncuts
        device(), kernels()
        t = {"host": [], "device": [], "kernels": []}
        for _ in range(args.reps):
            for name, fn in (("host", host), ("device", device), ("kernels", kernels)):
                r, ms = fn()
                assert r == want
                t[name].append(ms)
        row = {"seconds": secs, "samples": int(audio.shape[0]), "cuts": ncuts, "host_cut_points": stats(t["host"]),
               "device_upload_kernels_readback": stats(t["device"]), "device_kernels_only": stats(t["kernels"])}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "geometry": "x_query 10, x_center 60, x_max 65, window 160, 16 kHz", "reps": args.reps,
           "host_threads": torch.get_num_threads(),
           "note": "host_cut_points: pipeline._cut_points, host wall clock; device_upload_kernels_readback: pipeline._device_cuts (H2D of the fp64 "
                   "signal, two kernels, .tolist()), host wall clock; device_kernels_only: HIP events around rvcmi_glue_cut_points; the three "
                   "alternate in one process after a warm-up of each shape",
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
