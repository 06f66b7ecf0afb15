"""Cost of the input preparation of ``Pipeline.pipeline`` (infer/modules/vc/pipeline.py:221,241: high-pass ``filtfilt`` + reflection
pad) and of getting its result to where the GPU stages read it, host path against device path, for 10 s / 70 s / 305 s inputs at
B = 1 and for a ``convert_files`` group of 64 x 10 s.  Geometry x_pad 1, x_center 38, x_max 41 at 16 kHz; float32 inputs (``load_audio``).
Both paths end with the same device tensors: every segment and the padded signal as float32 (HuBERT, RMVPE), the unpadded signal as
float32 (``change_rms``), and, for an input longer than ``t_max``, the float64 signal the cut search reads.  The cut search itself
is common to both and not part of either (segments are taken at the multiples of ``t_center``).

  (a) host:    what the parent commit does per file -- ``signal.filtfilt``, ``np.pad``, one upload per consumer -- host wall clock
               ending in a synchronise;
  (b) device:  ``pipeline._device_prep`` -- ONE upload of the raw samples (all files of a group together), ``glue.filtfilt_flat``
               (two launches, the pad written by the second), device slices and casts -- host wall clock ending in a synchronise;
  (c) kernels: the two launches alone, HIP events, input resident, buffers preallocated.

After a warm-up of each shape the three alternate in one process; medians with min / max in ms.  Writes profiles/prep_time.json.

    python tools/prep_time.py [--reps 10] [--out profiles/prep_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SR = 16000


class State:
    """What ``pipeline._device_prep`` reads of a ``Pipeline`` object; its module (this script) holds ``bh, ah`` like the reference's."""
    window, t_pad, t_pad2, t_center, t_max = 160, SR, 2 * SR, 38 * SR, 41 * SR


def stats(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(float(np.min(ms)), 3), "max_ms": round(float(np.max(ms)), 3)}


def make_audio(seed, n):
    rng = np.random.default_rng(seed)
    return (0.2 * rng.standard_normal(n) + 0.2 * np.sin(np.arange(n) * 0.0864) + 0.01).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prep_time.json"))
    args = ap.parse_args()
    from scipy import signal

    import rvc_amd
    import rvc_amd.pipeline as rp
    from rvc_amd import glue

    dev = torch.device("cuda:0")
    global bh, ah
    bh, ah = signal.butter(N=5, Wn=48, btype="high", fs=16000)  # pipeline.py:23
    state = State()
    assert rp._ref_module(state).bh is bh
    os.environ["RVCMI_DEVICE_PREP"] = "1"
    rp.DEVICE_PREP_MIN_SAMPLES = 0  # every row is measured on both paths; the pipeline's threshold is chosen FROM these rows

    def consumers(audio, audio_pad, to_dev):
        """The tensors the GPU stages read, from the filtered signal and its padded twin (numpy on the host path, tensors on the
        device path)."""
        n, w = audio.shape[0], state.window
        out = []
        if n + 2 * (w // 2) > state.t_max:
            a64 = to_dev(audio, torch.float64)                            # the cut search ...
            out += [a64, a64.float()]                                     # ... whose copy change_rms shares (cast on the device)
        else:
            out.append(to_dev(audio, torch.float32))                      # change_rms
        out.append(to_dev(audio_pad, torch.float32))                      # RMVPE
        cuts = list(range(state.t_center, n, state.t_center)) if n + 2 * (w // 2) > state.t_max else []
        s, t = 0, None
        for t in cuts:
            out.append(to_dev(audio_pad[s: t + state.t_pad2 + w], torch.float32))
            s = t
        out.append(to_dev(audio_pad[t:], torch.float32))                  # HuBERT segments
        return out

    def host_to_dev(a, dt):  # as the parent's hubert_device / _rmvpe_on_device / _finish_file / _device_cuts do it
        if a.strides[0] < 0 or not a.flags.c_contiguous:  # (filtfilt returns a reversed view)
            a = np.ascontiguousarray(a, dtype=np.float32 if dt == torch.float32 else np.float64)
        t = torch.as_tensor(a)
        return (t.float() if dt == torch.float32 else t).to(dev)

    def dev_to_dev(a, dt):
        return a.float() if dt == torch.float32 else a

    rows = []
    for label, files in (("10 s", [10]), ("70 s", [70]), ("305 s", [305]), ("64 x 10 s", [10] * 64)):
        audios = [make_audio(1000 + 7 * i + secs, secs * SR) for i, secs in enumerate(files)]

        def host():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            keep = []
            for a in audios:
                f = signal.filtfilt(bh, ah, a)
                keep.append(consumers(f, np.pad(f, (state.t_pad, state.t_pad), mode="reflect"), host_to_dev))
            torch.cuda.synchronize(dev)
            return keep, (time.perf_counter() - t0) * 1e3

        def device():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            keep = [consumers(f, fp, dev_to_dev) for f, fp in rp._device_prep(state, audios, dev)]
            torch.cuda.synchronize(dev)
            return keep, (time.perf_counter() - t0) * 1e3

        bn, an, zi, order, padlen, warm = glue._filt_plan(bh, ah)
        L = rvc_amd._lib.lib()
        lens = [a.shape[0] for a in audios]
        total, B, pad = sum(lens), len(lens), state.t_pad
        flat = torch.from_numpy(np.concatenate(audios)).to(dev)
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int64, device=dev)
        out = torch.empty(total, device=dev, dtype=torch.float64)
        out_pad = torch.empty(total + 2 * pad * B, device=dev, dtype=torch.float64)
        nbytes = int(L.rvcmi_glue_filtfilt_scratch_bytes(B, total, order))
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        d = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731

        def kernels():
            e0.record()
            rvc_amd._lib.check(L.rvcmi_glue_filtfilt(rvc_amd._lib.ptr(flat), 0, rvc_amd._lib.ptr(offsets), B, max(lens), total, d(bn), d(an), d(zi), order, warm,
                                                     rvc_amd._lib.ptr(out), rvc_amd._lib.ptr(out_pad), pad, rvc_amd._lib.ptr(scratch), nbytes, rvc_amd._lib.stream_ptr(dev)))
            e1.record()
            e1.synchronize()
            return None, e0.elapsed_time(e1)

        # warm-up of each; the two paths give the same signal to rounding noise
        h, dv = host()[0], device()[0]
        kernels()
        diff = max(float((x.double() - y.double()).abs().max()) for hx, dx in zip(h, dv) for x, y in zip(hx, dx))
        assert diff < 1e-6, diff
        del h, dv
        host(), device(), kernels()
        t = {"host": [], "device": [], "kernels": []}
        for _ in range(args.reps):
            for name, fn in (("host", host), ("device", device), ("kernels", kernels)):
                t[name].append(fn()[1])
        row = {"input": label, "files": B, "samples": total, "lanes_per_pass": int(sum(-(-(n + 2 * padlen) // glue.FILT_LANE) for n in lens)),
               "host_filtfilt_pad_uploads": stats(t["host"]), "device_upload_kernels_pad": stats(t["device"]), "device_kernels_only": stats(t["kernels"]),
               "max_abs_difference_of_the_consumers_inputs": diff}
        h_, d_ = row["host_filtfilt_pad_uploads"], row["device_upload_kernels_pad"]
        row["device_faster_with_disjoint_ranges"] = bool(d_["max_ms"] < h_["min_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "geometry": "x_pad 1, x_center 38, x_max 41, window 160, 16 kHz, float32 inputs",
           "reps": args.reps, "host_threads": torch.get_num_threads(), "warmup_samples": int(warm), "lane": glue.FILT_LANE,
           "note": "host_filtfilt_pad_uploads: scipy filtfilt + np.pad + one upload per consumer, per file; device_upload_kernels_pad: "
                   "pipeline._device_prep (one H2D of the raw float32 samples, rvcmi_glue_filtfilt, device slices and casts); both host wall "
                   "clock ending in a synchronise; device_kernels_only: HIP events around rvcmi_glue_filtfilt; the three alternate in one "
                   "process after a warm-up of each shape",
           "rows": rows}
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
