"""One block of S live streams with BOTH noise-reduction boxes ticked on every session, at the GUI's 48 kHz geometry (0.25 s block, 2.5 s
extra: 282 noise frames of 1920 samples per gate, 30 signal frames), on the stub model of tools/rt_bank_time.py WITHOUT the feeders (fixed
HuBERT features and pitch; v2/48k generator, 768-d front, the 10000 x 768 index):

    (a) solo   S ``RealtimeStream`` objects with I_noise_reduce = O_noise_reduce = True, one pass each (what there was before the bank had boxes)
    (b) bank   ``RealtimeBank`` with ``set_noise_reduce(i, True, True)`` everywhere: the gates read the rolling spectrum cache
    (c) cold   the same bank with RVCMI_GATE_RING=0: every session transforms all its noise frames in every block (what the cache buys)

and, apart, the bare input-gate step (``TorchGateBank.forward``) at S = 64, cached against cold, by device events.

The project's convention: one process, the legs alternating (a b c a b c ...), warm-up first, host wall time per block around a device
synchronisation, median and range over the repeats.  Writes profiles/rt_bank_nr_time.json.

    python tools/rt_bank_nr_time.py [--sessions 1,4,16,64] [--reps 12] [--warmup 4] [--out profiles/rt_bank_nr_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

SR, BLOCK_TIME, BLOCK_MS = 48000, 0.25, 250.0


def stats(v):
    v = np.array(v)
    return dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4))


def below(a, b):
    """a's range lies wholly below b's."""
    return bool(a["max_ms"] < b["min_ms"])


class ring_switch:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get("RVCMI_GATE_RING")
        os.environ["RVCMI_GATE_RING"] = "1" if self.on else "0"

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("RVCMI_GATE_RING", None)
        else:
            os.environ["RVCMI_GATE_RING"] = self.old


def measure(dev, net, index, S, reps, warmup):
    import rt_bank_time as base
    import rvc_amd
    from oracle import synth

    geo = rvc_amd.stream_geometry(SR, BLOCK_TIME)
    p_len = geo["input_wav_res_len"] // 160
    nf = (p_len + 1) // 2
    feats = torch.stack([synth.make_phone(1, nf, 768, 100 + s)[0] for s in range(S)]).to(dev)
    pitchf = synth.make_f0(S, p_len).to(dev)
    pitch = synth.make_pitch(pitchf.cpu()).to(dev)
    kw = dict(samplerate=SR, block_time=BLOCK_TIME, crossfade_time=0.05, extra_time=2.5, device=dev)
    banks = {}
    for name in ("bank", "cold"):
        vcb = rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=base.INDEX_RATE, device=dev, tgt_sr=SR)
        banks[name] = rvc_amd.RealtimeBank(base.BankRVC(vcb, feats, pitch, pitchf, SR), sessions=S, **kw)
        for s in range(S):
            banks[name].set_noise_reduce(s, I=True, O=True)
    solos = [rvc_amd.RealtimeStream(base.SoloRVC(rvc_amd.RealtimeVC(net, index=index, index_rate=base.INDEX_RATE, device=dev, tgt_sr=SR), feats[s:s + 1],
                                                 pitch[s], pitchf[s], SR), I_noise_reduce=True, O_noise_reduce=True, **kw) for s in range(S)]
    x = (0.3 * np.random.default_rng(S).standard_normal((reps + warmup, S, banks["bank"].block_frame))).astype(np.float32)

    def run_bank(j):
        with ring_switch(True):
            return banks["bank"].process(x[j])

    def run_cold(j):
        with ring_switch(False):
            return banks["cold"].process(x[j])

    def run_solo(j):
        return [st.process(x[j, s]) for s, st in enumerate(solos)]

    ts = {"solo": [], "bank": [], "cold": []}
    outs = {}
    for j in range(reps + warmup):
        for name, fn in (("solo", run_solo), ("bank", run_bank), ("cold", run_cold)):   # the legs alternate
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            outs[name] = fn(j)
            torch.cuda.synchronize(dev)
            if j >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isfinite(outs["bank"]).all())
    assert banks["bank"].gate_I.last_modes == [1] * S and banks["cold"].gate_I.last_modes == [2] * S
    # the legs compute the same block: the bank rows are bit-equal to the cold bank's; the solos draw their own decoder noise, so they are not compared
    assert torch.equal(banks["bank"].input_wav_denoise, banks["cold"].input_wav_denoise)
    assert torch.equal(banks["bank"].input_wav_denoise[0], solos[0].input_wav_denoise)
    row = dict(sessions=S, reps=reps)
    for name, v in ts.items():
        row[name] = stats(v)
    row["bank_below_cold"] = below(row["bank"], row["cold"])
    row["bank_below_solo"] = below(row["bank"], row["solo"])
    row["solo_over_bank"] = round(row["solo"]["median_ms"] / row["bank"]["median_ms"], 3)
    row["cold_over_bank"] = round(row["cold"]["median_ms"] / row["bank"]["median_ms"], 3)
    row["ring_MB"] = round((banks["bank"].gate_I.ring_bytes + banks["bank"].gate_O.ring_bytes) / 1e6, 1)
    return row


def bare_gate(dev, S, reps, warmup):
    """TorchGateBank.forward alone (the input gate's shapes: x = the last 4 + 25 hops, xn = the 281-hop buffer rolled by one block)."""
    import rvc_amd

    geo = rvc_amd.stream_geometry(SR, BLOCK_TIME)
    zc, blk, nn = geo["zc"], geo["block_frame"], geo["input_wav_len"]
    n = geo["sola_buffer_frame"] + blk
    tg = rvc_amd.TorchGateHIP(sr=SR, n_fft=4 * zc, prop_decrease=0.9).to(dev)
    gates = {"cached": rvc_amd.TorchGateBank(tg, S, nn), "cold": rvc_amd.TorchGateBank(tg, S, nn)}
    gen = torch.Generator(device=dev).manual_seed(1)
    buf = 0.1 * torch.randn(S, nn, device=dev, generator=gen)
    ts = {"cached": [], "cold": []}
    for j in range(reps + warmup):
        buf[:, :-blk] = buf[:, blk:].clone()
        buf[:, -blk:] = 0.1 * torch.randn(S, blk, device=dev, generator=gen)
        for name in ("cached", "cold"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with ring_switch(name == "cached"):
                e0.record()
                gates[name].forward(buf[:, -n:], buf, blk, blk, [True] * S)
                e1.record()
            torch.cuda.synchronize(dev)
            if j >= warmup:
                ts[name].append(e0.elapsed_time(e1))
    assert gates["cached"].last_modes == [1] * S and gates["cold"].last_modes == [2] * S
    plan = rvc_amd.glue.gate_ring_plan(nn, 4 * zc, zc, blk, blk)
    row = dict(sessions=S, reps=reps, noise_frames=plan["Fn"], dirty_frames=plan["n_dirty"], signal_frames=1 + n // zc, cached=stats(ts["cached"]),
               cold=stats(ts["cold"]))
    row["cached_below_cold"] = below(row["cached"], row["cold"])
    row["cold_over_cached"] = round(row["cold"]["median_ms"] / row["cached"]["median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_bank_nr_time.json"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("at least 10 repeats")
    import rvc_amd
    from oracle import nsf_oracle, synth
    from oracle.front_oracle import FrontConfig

    dev = torch.device("cuda:0")
    sessions = [int(s) for s in a.sessions.split(",")]
    idx = synth.make_ivf(10000, 768, seed=4321, kmeans_iters=1)
    index = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=dev)
    index.reserve(16 * max(sessions))

    class Net:
        """tools/rt_bank_time.py's, on the v2/48k generator."""

        def __init__(self, max_B):
            cfg, fcfg = nsf_oracle.CONFIGS["v2_48k"], FrontConfig()
            wf = synth.make_front_weights(fcfg, 1234)
            self.dec = rvc_amd.NSFGeneratorHIP(vars(cfg), synth.make_dec_weights(cfg, 1234), device=dev, operand="fp16", max_B=max_B, max_T=64)
            self.front = rvc_amd.FrontHIP(vars(fcfg), wf, device=dev, operand="fp16", max_B=max_B, max_T=288)
            emb = wf["emb_g.weight"].to(dev)
            self.emb_g = lambda sid: emb[sid]

        def infer(self, phone, lengths, sid, pitch=None, pitchf=None, skip_head=None, return_length=None, return_length2=None):
            return rvc_amd.infer_hip(self, self.front, phone, lengths, sid, pitch, pitchf, skip_head, return_length, return_length2)

    net = Net(max(sessions))
    rows = []
    for S in sessions:
        row = measure(dev, net, index, S, a.reps, a.warmup)
        rows.append(row)
        print("S %3d  solo %8.3f [%8.3f, %8.3f]  bank %8.3f [%8.3f, %8.3f]  cold %8.3f [%8.3f, %8.3f] ms  solo/bank %.2f  cold/bank %.2f  bank below cold %s" % (
            S, row["solo"]["median_ms"], row["solo"]["min_ms"], row["solo"]["max_ms"], row["bank"]["median_ms"], row["bank"]["min_ms"], row["bank"]["max_ms"],
            row["cold"]["median_ms"], row["cold"]["min_ms"], row["cold"]["max_ms"], row["solo_over_bank"], row["cold_over_bank"], row["bank_below_cold"]),
            flush=True)
    gate = bare_gate(dev, 64, a.reps, a.warmup)
    print("bare gate S 64: cached %.3f [%.3f, %.3f]  cold %.3f [%.3f, %.3f] ms  cold/cached %.2f" % (
        gate["cached"]["median_ms"], gate["cached"]["min_ms"], gate["cached"]["max_ms"], gate["cold"]["median_ms"], gate["cold"]["min_ms"],
        gate["cold"]["max_ms"], gate["cold_over_cached"]), flush=True)
    under = [r["sessions"] for r in rows if r["bank"]["max_ms"] < BLOCK_MS]
    res = dict(device=torch.cuda.get_device_name(dev),
               what="ms per block of S sessions with both noise-reduction boxes ticked on every session (host wall time around a device synchronisation; "
                    "eager, no hipGraph; no feeders): S RealtimeStream.process calls (solo), RealtimeBank.process with the rolling spectrum cache (bank) "
                    "and with RVCMI_GATE_RING=0 (cold); v2/48k generator, 768-d front, 10000 x 768 index, 0.25 s block at 48 kHz, 2.5 s extra; legs "
                    "alternating in one process.  bare_gate: TorchGateBank.forward of the input gate alone by device events",
               rows=rows, bare_gate=gate,
               cache_is_default=all(r["bank_below_cold"] for r in rows if r["sessions"] >= 4),
               largest_measured_S_under_one_block=max(under) if under else None)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
