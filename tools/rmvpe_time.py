"""Time of the f0 step ``pipeline._rmvpe_on_device`` with the whole RMVPE estimator on HIP (``RVCMI_RMVPE_HIP=1``, rvc_amd/rmvpe.py) against the
path it replaces, and the parity figures of its log-mel front end.

    python tools/rmvpe_time.py --out profiles/rmvpe_time.json [--parity profiles/rmvpe_parity.json] [--repeats 20]

Baseline: GRU and U-Net on HIP (``RVCMI_RMVPE_UNET=1``), mel front end and head on PyTorch-ROCm.  Candidate: the switch on.  Same seeded
weights (the stand-in objects of tests/rmvpe_cases.py), ``is_half``.  Both legs run in ONE process, alternating A / B, every shape warmed up
first, timed with a device-synchronised host clock; median and range of ``--repeats`` runs per leg, eager at 32, 64, 1201 and 3073 frames, and
for the two realtime sizes also replayed from the hipGraph of ``realtime._rmvpe_f0_graphed``.  A shape whose ranges overlap is a tie.

``--parity``: per signal of the GPU test, the max abs log-mel error against the fp64 oracle of the HIP front end and of the torch fp32 path
(``round_half = 0``), and the count of elements off the oracle in fp16 steps (``round_half = 1``).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import rmvpe_cases as rc  # noqa: E402

FRAMES = (32, 64, 1201, 3073)
LEGS = {"torch_mel_head": {"RVCMI_RMVPE_HIP": "0", "RVCMI_RMVPE_UNET": "1"}, "rmvpe_hip": {"RVCMI_RMVPE_HIP": "1", "RVCMI_RMVPE_UNET": "1"}}


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t) * 1e3


def leg(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def verdict(a, b):
    if a["max_ms"] < b["min_ms"]:
        return "rmvpe_hip faster"
    if b["max_ms"] < a["min_ms"]:
        return "torch mel + head faster"
    return "a tie"


def switch(name):
    os.environ.update(LEGS[name])


def parity(dev, path):
    import rvc_amd  # noqa: F401
    from rvc_amd import _lib

    L = _lib.lib()
    rows = []
    for bank_name, bank in (("htk", rc.htk_bank()), ("dense", rc.dense_bank())):
        h = C.c_void_p()
        b = bank.contiguous()
        _lib.check(L.rvcmi_mel_create(rc.N_FFT, rc.HOP, rc.N_FFT, 128, C.c_void_p(b.data_ptr()), rc.CLAMP, 0, C.byref(h)))
        for kind in ("voiced", "noise", "quiet", "sine"):
            for n in rc.LENGTHS:
                x = rc.signal(kind, n)
                T, T_pad = n // rc.HOP + 1, rc.pad32(n // rc.HOP + 1)
                xd = x.to(dev)
                row = dict(bank=bank_name, signal=kind, n=n, frames=T)
                for half in (0, 1):
                    out = torch.empty(1, T_pad, 128, device=dev)
                    _lib.check(L.rvcmi_mel_forward(h, 1, n, C.c_void_p(xd.data_ptr()), half, T_pad, C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
                    got = out[0, :T].cpu()
                    want = rc.log_mel(x[None], bank, torch.float64, bool(half))[0].T
                    ref = rc.log_mel(x[None], bank, torch.float32, bool(half))[0].T
                    if half:
                        u, ut = rc.half_ulps(got, want), rc.half_ulps(ref, want)
                        row.update(half_hip_not_equal=int((u > 0).sum()), half_hip_max_ulp=int(u.max()), half_torch_fp32_not_equal=int((ut > 0).sum()),
                                   half_torch_fp32_max_ulp=int(ut.max()), elements=u.numel())
                    else:
                        row.update(fp32_hip_max_abs=float((got.double() - want).abs().max()), fp32_torch_max_abs=float((ref.double() - want).abs().max()))
                print(json.dumps(row), flush=True)
                rows.append(row)
        L.rvcmi_mel_destroy(h)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(dict(reference="tests/rmvpe_cases.log_mel in fp64 on the CPU; torch = the same lines in fp32 on the CPU", cases=rows), open(path, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parity")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import rvc_amd.pipeline as rp
    from rvc_amd import realtime as rt

    dev = torch.device("cuda:0")
    if a.parity:
        parity(dev, a.parity)
    if not a.out:
        return
    res = dict(device=torch.cuda.get_device_name(dev), repeats=a.repeats, warmup=a.warmup, shapes=[],
               method="same process, alternating baseline / candidate, device-synchronised host clock around pipeline._rmvpe_on_device (eager) and "
                      "realtime._rmvpe_f0_graphed (replayed hipGraph); baseline = GRU and U-Net on HIP, mel front end and head on PyTorch-ROCm; "
                      "candidate = RVCMI_RMVPE_HIP=1; seeded weights, is_half")
    mes = {}
    for name in LEGS:
        r = rc.RmvpeStandIn(dev, True)
        mes[name] = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=r, is_half=True, device=dev))
    g = torch.Generator().manual_seed(0)
    for T in FRAMES:
        n = (T - 1) * rc.HOP
        wav = (rc.signal("voiced", n) + 0.05 * torch.randn(n, generator=g)).to(dev)
        p_len = n // rc.HOP
        row = dict(frames=T, samples=n)
        modes = [("eager", lambda me: rp._rmvpe_on_device(me, wav, p_len, 0))]
        if T <= 64:
            modes.append(("graph", lambda me: rt._rmvpe_f0_graphed(me, wav, p_len, 0)))
        for mode, fn in modes:
            ms = {k: [] for k in LEGS}
            for name in LEGS:
                switch(name)
                for _ in range(max(a.warmup, rt.RT_GRAPH_AFTER + 1)):
                    fn(mes[name])
                if mode == "graph":
                    assert "graph" in mes[name]._rvcmi_f0_graphs[(n, p_len, 0, str(wav.device))]
            for _ in range(a.repeats):
                for name in LEGS:
                    switch(name)
                    ms[name].append(timed(lambda: fn(mes[name]), dev))
            base, cand = leg(ms["torch_mel_head"]), leg(ms["rmvpe_hip"])
            row[mode] = dict(torch_mel_head=base, rmvpe_hip=cand, verdict=verdict(cand, base), speedup_median=base["median_ms"] / cand["median_ms"])
        assert hasattr(mes["rmvpe_hip"].f0_gen, "_rvcmi_rmvpe_hip") and not hasattr(mes["torch_mel_head"].f0_gen, "_rvcmi_rmvpe_hip")
        print(json.dumps(row), flush=True)
        res["shapes"].append(row)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
