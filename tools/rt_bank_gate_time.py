"""What the two per-session steps of a bank block cost, and what their replacements cost:

1. the input gate -- ``RealtimeBank`` with ``threhold = -40`` on a signal with quiet stretches, the gate on the host (numpy, per session)
   against the gate on the device (``glue.input_gate_batch``) against the same bank with ``threhold = -60`` (no gate), on the model of
   tools/rt_bank_time.py WITHOUT feeders (v1/40k generator, 768-d front, 10000 x 768 index, 282 / 250 / 31 frames, 0.26 s block at 40 kHz);
   and the solo ``RealtimeStream`` pair (host gate / device gate) on the same model;
2. the f0 decode -- ``RealtimeBank`` around ``rvc_infer_batch_hip`` with the stub feeders of tests/rt_bank_cases.py (``FramingHubert``,
   ``FramingRMVPE``: cheap, so the decode shows; v2/48k, 70 / 40 / 20 frames), the bank of the parent commit (its ``realtime.py``, given
   with ``--parent-realtime``: one ``glue.rmvpe_f0`` per session) against this one (its ``glue.rmvpe_f0`` calls per session gathered into one ragged
   decode call: two launches).  Gate off.

The project's convention: one process, the legs alternating, warm-up first, host wall time per block around a device synchronisation,
median and range over the repeats.  Writes profiles/rt_bank_gate_time.json, with the defaults the numbers decide: the device gate is the
bank's default iff its range lies wholly below the host gate's at every S >= 4, the solo stream's iff its own pair says so.

    python tools/rt_bank_gate_time.py [--sessions 1,4,16,64] [--reps 12] [--warmup 4] [--parent-realtime FILE] [--out profiles/rt_bank_gate_time.json]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

THREHOLD = -40
FEEDER_KW = dict(samplerate=48000, block_time=0.15, crossfade_time=0.14, extra_time=0.4)   # 70 frames, skip_head 40, return_length 20


def gated_signal(rng, shape, zc, threhold):
    """Noise whose level steps every three hops between ``threhold - 8`` and ``threhold + 8`` dB: quiet stretches and loud ones."""
    x = rng.standard_normal(shape).astype(np.float32)
    n = shape[-1]
    for lo in range(0, n, 3 * zc):
        x[..., lo: lo + 3 * zc] *= (10.0 ** ((threhold + rng.uniform(-8, 8, shape[:-1] + (1,))) / 20.0)).astype(np.float32)
    return x


def stats(ts):
    out = {}
    for name, v in ts.items():
        v = np.array(v)
        out[name] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4))
    return out


def alternate(dev, legs, reps, warmup):
    """legs: name -> fn(j); the legs alternate (A B C A B C ...) -> name -> list of ms."""
    ts = {name: [] for name in legs}
    for j in range(reps + warmup):
        for name, fn in legs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = fn(j)
            torch.cuda.synchronize(dev)
            if j >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
        assert bool(torch.isfinite(out).all())
    return ts


def below(a, b):
    """Does leg a's range lie wholly below leg b's?"""
    return bool(a["max_ms"] < b["min_ms"])


def measure_gate(dev, net, index, S, reps, warmup):
    import rt_bank_time as base
    import rvc_amd
    from oracle import synth

    SR = base.SR
    feats = torch.stack([synth.make_phone(1, base.NF, 768, 100 + s)[0] for s in range(S)]).to(dev)
    pitchf = synth.make_f0(S, base.P_LEN).to(dev)
    pitch = synth.make_pitch(pitchf.cpu()).to(dev)
    kw = dict(samplerate=SR, block_time=base.BLOCK_TIME, crossfade_time=0.05, extra_time=2.5, device=dev)

    def bank(**more):
        vcb = rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=base.INDEX_RATE, device=dev, tgt_sr=SR)
        return rvc_amd.RealtimeBank(base.BankRVC(vcb, feats, pitch, pitchf, SR), sessions=S, **dict(kw, **more))

    banks = dict(host_gate=bank(threhold=THREHOLD, device_gate=False), device_gate=bank(threhold=THREHOLD, device_gate=True),
                 gate_off=bank(threhold=-60, device_gate=False))
    b0 = banks["host_gate"]
    x = gated_signal(np.random.default_rng(S), (reps + warmup, S, b0.block_frame), b0.zc, THREHOLD)
    ts = alternate(dev, {name: (lambda j, b=b: b.process(x[j])) for name, b in banks.items()}, reps, warmup)
    assert torch.equal(banks["host_gate"].input_wav, banks["device_gate"].input_wav)            # the same gated signal, bit for bit
    zeroed = float((banks["host_gate"].input_wav[:, -b0.block_frame:] == 0).float().mean())
    row = dict(sessions=S, reps=reps, zeroed_share_of_last_block=round(zeroed, 3), **stats(ts))
    row["device_below_host"] = below(row["device_gate"], row["host_gate"])
    row["host_gate_cost_ms"] = round(row["host_gate"]["median_ms"] - row["gate_off"]["median_ms"], 4)
    row["device_gate_cost_ms"] = round(row["device_gate"]["median_ms"] - row["gate_off"]["median_ms"], 4)
    return row


def measure_stream(dev, net, index, reps, warmup):
    import rt_bank_time as base
    import rvc_amd
    from oracle import synth

    SR = base.SR
    feats = synth.make_phone(1, base.NF, 768, 100).to(dev)
    pitchf = synth.make_f0(1, base.P_LEN).to(dev)
    pitch = synth.make_pitch(pitchf.cpu()).to(dev)
    kw = dict(samplerate=SR, block_time=base.BLOCK_TIME, crossfade_time=0.05, extra_time=2.5, device=dev, threhold=THREHOLD)

    def stream(device_gate):
        vc = rvc_amd.RealtimeVC(net, index=index, index_rate=base.INDEX_RATE, device=dev, tgt_sr=SR)
        return rvc_amd.RealtimeStream(base.SoloRVC(vc, feats, pitch[0], pitchf[0], SR), device_gate=device_gate, **kw)

    streams = dict(host_gate=stream(False), device_gate=stream(True))
    s0 = streams["host_gate"]
    x = gated_signal(np.random.default_rng(1), (reps + warmup, s0.block_frame), s0.zc, THREHOLD)
    ts = alternate(dev, {name: (lambda j, s=s: s.process(x[j])) for name, s in streams.items()}, reps, warmup)
    assert torch.equal(streams["host_gate"].input_wav, streams["device_gate"].input_wav)
    row = dict(reps=reps, **stats(ts))
    row["device_below_host"] = below(row["device_gate"], row["host_gate"])
    return row


def measure_decode(dev, net, index, S, reps, warmup, parent):
    import rt_bank_cases as cases
    import rvc_amd

    net.rows = slice(0, S)
    keys = [(s % 25) - 12 + (0.35 if s % 3 == 2 else 0) for s in range(S)]

    def bank(module):
        b = module.RealtimeBank(cases.stub_rvc(net, index, dev, 0), sessions=S, device=dev, **FEEDER_KW)
        for s in range(S):
            b.set_key(s, keys[s])
        return b

    banks = dict(after=bank(rvc_amd.realtime))
    if parent is not None:
        banks = dict(before=bank(parent), **banks)
    b0 = banks["after"]
    x = (0.3 * np.random.default_rng(S).standard_normal((reps + warmup, S, b0.block_frame))).astype(np.float32)
    ts = alternate(dev, {name: (lambda j, b=b: b.process(x[j])) for name, b in banks.items()}, reps, warmup)
    row = dict(sessions=S, reps=reps, **stats(ts))
    if parent is not None:
        assert torch.equal(banks["before"].vc.pitch, banks["after"].vc.pitch) and torch.equal(banks["before"].vc.pitchf, banks["after"].vc.pitchf)
        row["pitch_caches_bit_equal"] = True
        row["after_below_before"] = below(row["after"], row["before"])
        row["before_over_after"] = round(row["before"]["median_ms"] / row["after"]["median_ms"], 3)
    return row


def load_parent(path):
    """The parent commit's ``realtime.py`` as a module of the installed package (its relative imports resolve to the package's modules)."""
    spec = importlib.util.spec_from_file_location("rvc_amd.realtime_parent", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--parent-realtime", default=None, help="realtime.py of the parent commit (git show HEAD~:.../realtime.py), for the decode table")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_bank_gate_time.json"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("at least 10 repeats")
    import rt_bank_cases as cases
    import rt_bank_time as base
    import rvc_amd
    from oracle import synth

    dev = torch.device("cuda:0")
    sessions = [int(s) for s in a.sessions.split(",")]
    idx = synth.make_ivf(10000, 768, seed=4321, kmeans_iters=1)
    index = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=dev)
    index.reserve(16 * max(sessions))
    net = base.Net(dev, max(sessions))
    gate_rows = []
    for S in sessions:
        row = measure_gate(dev, net, index, S, a.reps, a.warmup)
        gate_rows.append(row)
        print("gate   S %3d  host %8.3f [%8.3f, %8.3f]  device %8.3f [%8.3f, %8.3f]  off %8.3f [%8.3f, %8.3f]  device below host %s" % (
            (S,) + tuple(row[k][f] for k in ("host_gate", "device_gate", "gate_off") for f in ("median_ms", "min_ms", "max_ms")) + (row["device_below_host"],)),
            flush=True)
    stream_row = measure_stream(dev, net, index, a.reps, a.warmup)
    print("stream        host %8.3f [%8.3f, %8.3f]  device %8.3f [%8.3f, %8.3f]  device below host %s" % (
        tuple(stream_row[k][f] for k in ("host_gate", "device_gate") for f in ("median_ms", "min_ms", "max_ms")) + (stream_row["device_below_host"],)), flush=True)
    del net
    parent = load_parent(a.parent_realtime) if a.parent_realtime else None
    idx2 = cases.index_768()
    index2 = rvc_amd.IVFFlatHIP.from_arrays(idx2["centroids"], idx2["list_offsets"], idx2["ids"], idx2["vecs"], device=dev)
    net2 = cases.BankNet(dev, max(sessions))
    decode_rows = []
    for S in sessions:
        row = measure_decode(dev, net2, index2, S, a.reps, a.warmup, parent)
        decode_rows.append(row)
        print("decode S %3d  %s" % (S, "  ".join("%s %8.3f [%8.3f, %8.3f]" % (k, row[k]["median_ms"], row[k]["min_ms"], row[k]["max_ms"])
                                                 for k in ("before", "after") if k in row)), flush=True)
    big = [r for r in gate_rows if r["sessions"] >= 4]
    res = dict(device=torch.cuda.get_device_name(dev),
               what="ms per block of S sessions (host wall time around a device synchronisation; eager, no hipGraph), legs alternating in one process "
                    "after a warm-up; median [min, max] over the repeats",
               gate=dict(what="RealtimeBank.process WITHOUT feeders (the model of tools/rt_bank_time.py: v1/40k generator, 768-d front, 10000 x 768 index, "
                              "282 / 250 / 31 frames, 0.26 s block at 40 kHz), threhold -40 on noise whose level steps between -48 and -32 dB every three "
                              "hops: the gate on the host (numpy per session), on the device (glue.input_gate_batch), and the same bank with threhold -60",
                         rows=gate_rows),
               stream=dict(what="RealtimeStream.process on the same model and signal, host gate against device gate", row=stream_row),
               decode=dict(what="RealtimeBank.process around rvc_infer_batch_hip with the stub feeders of tests/rt_bank_cases.py (v2/48k, 70 / 40 / 20 frames, "
                                "0.15 s block at 48 kHz, a key per session, gate off): the parent commit's bank (one glue.rmvpe_f0 per session) against this "
                                "one (rvc_infer_batch_hip as committed: the per-session glue.rmvpe_f0 calls gathered into one rvcmi_glue_rmvpe_f0_ragged call)" + ("" if parent is not None else "; the parent's realtime.py was not given: no 'before' leg"),
                           rows=decode_rows),
               defaults=dict(rule="the device gate is the bank's default iff its range lies wholly below the host gate's at every S >= 4; the solo stream's "
                                  "default follows its own pair; a tie keeps the host gate",
                             bank_device_gate=bool(big) and all(r["device_below_host"] for r in big),
                             stream_device_gate=bool(stream_row["device_below_host"])))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("defaults:", res["defaults"]["bank_device_gate"], res["defaults"]["stream_device_gate"])
    print("wrote", a.out)


if __name__ == "__main__":
    main()
