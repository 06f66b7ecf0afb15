"""One block of S live streams with a formant shift PER SESSION: ``RealtimeBank`` with S distinct shifts (one ragged partial decode, one
ragged resample) against (a) S solo ``RealtimeStream`` + ``RealtimeVC(formant_shift=f_s)`` objects, the only way to serve per-session shifts
before, and (b) the same bank with every shift zero: the cost of the feature.  Synthetic v2/48k model (generator, 768-d front, the
10000 x 768 index) WITHOUT the feeders: HuBERT features and the f0 estimator's output are fixed device tensors.  0.25 s blocks at 48 kHz:
281 / 250 / 30 frames; a shifted session decodes 27 .. 34 frames.

The project's convention: one process, the legs alternating (A B C A B C ...), warm-up first, eager, host wall time per block around a
device synchronisation, median and range over the repeats.  Writes profiles/rt_bank_formant_time.json.

    python tools/rt_bank_formant_time.py [--sessions 1,4,16,64] [--reps 12] [--warmup 4] [--out profiles/rt_bank_formant_time.json]
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

SR, BLOCK_TIME, PROTECT, INDEX_RATE = 48000, 0.25, 0.33, 0.75
NF, P_LEN = 140, 281


class Net:
    """What the realtime classes need of ``net_g``: ``infer`` on the HIP front + generator (``rvc_amd.infer_hip``), torch's RNG for the noise."""

    def __init__(self, dev, max_B):
        import rvc_amd
        from oracle import nsf_oracle, synth
        from oracle.front_oracle import FrontConfig

        cfg, fcfg = nsf_oracle.CONFIGS["v2_48k"], FrontConfig()
        wf = synth.make_front_weights(fcfg, 1234)
        self.dec = rvc_amd.NSFGeneratorHIP(vars(cfg), synth.make_dec_weights(cfg, 1234), device=dev, operand="fp16", max_B=max_B, max_T=64)
        self.front = rvc_amd.FrontHIP(vars(fcfg), wf, device=dev, operand="fp16", max_B=max_B, max_T=288)
        emb = wf["emb_g.weight"].to(dev)
        self.emb_g = lambda sid: emb[sid]

    def infer(self, phone, lengths, sid, pitch=None, pitchf=None, skip_head=None, return_length=None, return_length2=None):
        import rvc_amd

        return rvc_amd.infer_hip(self, self.front, phone, lengths, sid, pitch, pitchf, skip_head, return_length, return_length2)


class SoloRVC:
    """``rtrvc.RVC``-like without feeders: fixed features and pitch, a ``RealtimeVC`` of its own (which holds the session's shift)."""

    def __init__(self, vc, feats, pitch, pitchf, tgt_sr):
        self.vc, self.feats, self.pitch, self.pitchf, self.tgt_sr = vc, feats, pitch, pitchf, tgt_sr

    def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
        return self.vc.infer(self.feats, int(input_wav_res.shape[0]), block_frame_16k, skip_head, return_length, pitch=self.pitch, pitchf=self.pitchf,
                             protect=PROTECT)


class BankRVC:
    def __init__(self, vc, feats, pitch, pitchf, tgt_sr):
        self.vc, self.feats, self.pitch, self.pitchf, self.tgt_sr = vc, feats, pitch, pitchf, tgt_sr

    def infer_batch(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method, keys, sids, formants=None):
        return self.vc.infer(self.feats, int(input_wav_res.shape[1]), block_frame_16k, skip_head, return_length, pitch=self.pitch, pitchf=self.pitchf,
                             protect=PROTECT, sid=sids, formants=formants)


def shifts_for(S):
    """S distinct values of the GUI's slider (-2 .. 2 in steps of 0.05), spread over its range."""
    v = [round(round(float(x) / 0.05) * 0.05, 2) for x in np.linspace(-2.0, 2.0, S)] if S > 1 else [2.0]
    assert len(set(v)) == S
    return v


def measure(dev, net, index, S, reps, warmup):
    import rvc_amd
    from oracle import synth

    feats = torch.stack([synth.make_phone(1, NF, 768, 100 + s)[0] for s in range(S)]).to(dev)
    pitchf = synth.make_f0(S, P_LEN).to(dev)
    pitch = synth.make_pitch(pitchf.cpu()).to(dev)
    kw = dict(samplerate=SR, block_time=BLOCK_TIME, crossfade_time=0.05, extra_time=2.5, device=dev)
    shifts = shifts_for(S)

    def make_bank(fm):
        vcb = rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=INDEX_RATE, device=dev, tgt_sr=SR)
        bank = rvc_amd.RealtimeBank(BankRVC(vcb, feats, pitch, pitchf, SR), sessions=S, **kw)
        for s, f in enumerate(fm):
            bank.set_formant(s, f)
        return bank

    shifted, plain = make_bank(shifts), make_bank([0.0] * S)
    assert (shifted.skip_head, shifted.return_length, shifted.input_wav_res_len // 160) == (250, 30, P_LEN)
    solos = [rvc_amd.RealtimeStream(SoloRVC(rvc_amd.RealtimeVC(net, index=index, index_rate=INDEX_RATE, device=dev, tgt_sr=SR, formant_shift=shifts[s]),
                                            feats[s:s + 1], pitch[s], pitchf[s], SR), **kw) for s in range(S)]
    x = (0.3 * np.random.default_rng(S).standard_normal((reps + warmup, S, shifted.block_frame))).astype(np.float32)
    legs = (("bank_shifted", lambda j: shifted.process(x[j])), ("solo_shifted", lambda j: [st.process(x[j, s]) for s, st in enumerate(solos)]),
            ("bank_unshifted", lambda j: plain.process(x[j])))
    ts = {name: [] for name, _ in legs}
    for j in range(reps + warmup):
        for name, fn in legs:   # the legs alternate
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = fn(j)
            torch.cuda.synchronize(dev)
            if j >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
            assert bool(torch.isfinite(out[0]).all())
    rl2 = [rvc_amd.formant_geometry(f, shifted.return_length, SR)[1] for f in shifts]
    row = dict(sessions=S, reps=reps, shifts=shifts, return_length2_min=min(rl2), return_length2_max=max(rl2),
               resample_tables=len(shifted.rvc.vc._resample.offsets), resample_table_floats=shifted.rvc.vc._resample.table_floats)
    for name, v in ts.items():
        v = np.array(v)
        row[name] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4))

    def disjoint(a, b):
        return bool(row[a]["max_ms"] < row[b]["min_ms"] or row[b]["max_ms"] < row[a]["min_ms"])

    row["bank_vs_solo_ranges_disjoint"] = disjoint("bank_shifted", "solo_shifted")
    row["solo_over_bank"] = round(row["solo_shifted"]["median_ms"] / row["bank_shifted"]["median_ms"], 3)
    row["shifted_vs_unshifted_ranges_disjoint"] = disjoint("bank_shifted", "bank_unshifted")
    row["shifted_over_unshifted"] = round(row["bank_shifted"]["median_ms"] / row["bank_unshifted"]["median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_bank_formant_time.json"))
    a = ap.parse_args()
    if a.reps < 10:
        raise SystemExit("at least 10 repeats")
    import rvc_amd
    from oracle import synth

    dev = torch.device("cuda:0")
    sessions = [int(s) for s in a.sessions.split(",")]
    idx = synth.make_ivf(10000, 768, seed=4321, kmeans_iters=1)
    index = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=dev)
    index.reserve(16 * max(sessions))
    net = Net(dev, max(sessions))
    rows = []
    for S in sessions:
        row = measure(dev, net, index, S, a.reps, a.warmup)
        rows.append(row)
        fmt = lambda r: "%8.3f ms [%8.3f, %8.3f]" % (r["median_ms"], r["min_ms"], r["max_ms"])  # noqa: E731
        print("S %3d  bank, S shifts %s   %d solo, shifted %s   bank, no shift %s   solo/bank %.2f (disjoint %s)  shifted/unshifted %.2f (disjoint %s)" % (
            S, fmt(row["bank_shifted"]), S, fmt(row["solo_shifted"]), fmt(row["bank_unshifted"]), row["solo_over_bank"],
            row["bank_vs_solo_ranges_disjoint"], row["shifted_over_unshifted"], row["shifted_vs_unshifted_ranges_disjoint"]), flush=True)
    res = dict(device=torch.cuda.get_device_name(dev),
               what="ms per block of S sessions (host wall time around a device synchronisation; eager, no hipGraph; no feeders): RealtimeBank.process "
                    "with S distinct formant shifts against S RealtimeStream.process calls, each with its own RealtimeVC(formant_shift), and against "
                    "the same bank with every shift zero; v2/48k generator, 768-d front, 10000 x 768 index, 281 / 250 / 30 frames, 0.25 s block at "
                    "48 kHz, protect 0.33, index_rate 0.75; legs alternating in one process; ranges that overlap are a tie",
               rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
