"""One block of S live streams with the GUI's index_rate / protect / rms_mix_rate / threhold sliders PER SESSION: (a) ``RealtimeBank`` with
distinct values per session -- all four controls active in most sessions, a quarter of the sessions at ``index_rate = 0`` -- against (b) the
same bank with the shared bank-wide values (the path a bank without the setters runs), (c) S solo ``RealtimeStream`` objects with the
per-session values, the only way to serve them before, and (d) the bank of (a) with every session blending (what skipping the rate-0
sessions' search rows is worth).  Synthetic v2/48k model (generator, 768-d front, the 10000 x 768 index) WITHOUT the feeders: HuBERT features
and the f0 estimator's output are fixed device tensors.  0.25 s blocks at 48 kHz: 281 / 250 / 30 frames.

The project's convention: one process, the legs alternating (A B C D A B C D ...), warm-up first, eager, host wall time per block around a
device synchronisation, median and range over the repeats.  Writes profiles/rt_bank_sliders_time.json.

    python tools/rt_bank_sliders_time.py [--sessions 1,4,16,64] [--reps 12] [--warmup 4] [--out profiles/rt_bank_sliders_time.json]
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

from rt_bank_formant_time import NF, P_LEN, Net  # noqa: E402  (the same model and geometry)

SR, BLOCK_TIME = 48000, 0.25
BANK_WIDE = dict(index_rate=0.75, protect=0.33, rms_mix_rate=0.25, threhold=-40)


def sliders_for(S, all_blend=False):
    """Distinct values per session: every fourth session at index_rate 0 (unless ``all_blend``), every fifth without the protect mix, every
    sixth without the envelope mix, every eighth ungated."""
    return dict(index_rate=[0.0 if s % 4 == 3 and not all_blend else round(0.3 + 0.07 * (s % 7), 2) for s in range(S)],
                protect=[1.0 if s % 5 == 4 else round(0.2 + 0.04 * (s % 6), 2) for s in range(S)],
                rms_mix_rate=[1.0 if s % 6 == 5 else round(0.16 * (s % 5), 2) for s in range(S)],
                threhold=[-60 if s % 8 == 7 else -50 + 3 * (s % 9) for s in range(S)])


class SoloRVC:
    """``rtrvc.RVC``-like without feeders: fixed features and pitch, a ``RealtimeVC`` of its own (which holds the session's index_rate)."""

    def __init__(self, vc, feats, pitch, pitchf, tgt_sr, protect):
        self.vc, self.feats, self.pitch, self.pitchf, self.tgt_sr, self.protect = vc, feats, pitch, pitchf, tgt_sr, protect

    def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
        return self.vc.infer(self.feats, int(input_wav_res.shape[0]), block_frame_16k, skip_head, return_length, pitch=self.pitch, pitchf=self.pitchf,
                             protect=self.protect)


class BankRVC:
    def __init__(self, vc, feats, pitch, pitchf, tgt_sr):
        self.vc, self.feats, self.pitch, self.pitchf, self.tgt_sr, self.index_rate = vc, feats, pitch, pitchf, tgt_sr, BANK_WIDE["index_rate"]

    def infer_batch(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method, keys, sids, index_rates=None, protects=None):
        return self.vc.infer(self.feats, int(input_wav_res.shape[1]), block_frame_16k, skip_head, return_length, pitch=self.pitch, pitchf=self.pitchf,
                             protect=BANK_WIDE["protect"], sid=sids, index_rates=index_rates or [None] * self.vc.S, protects=protects or [None] * self.vc.S)


def measure(dev, net, index, S, reps, warmup):
    import rvc_amd
    from oracle import synth

    feats = torch.stack([synth.make_phone(1, NF, 768, 100 + s)[0] for s in range(S)]).to(dev)
    pitchf = synth.make_f0(S, P_LEN).to(dev)
    pitch = synth.make_pitch(pitchf.cpu()).to(dev)
    kw = dict(samplerate=SR, block_time=BLOCK_TIME, crossfade_time=0.05, extra_time=2.5, device=dev, device_gate=True)
    own = sliders_for(S)

    def make_bank(values):
        vcb = rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=BANK_WIDE["index_rate"], device=dev, tgt_sr=SR)
        bank = rvc_amd.RealtimeBank(BankRVC(vcb, feats, pitch, pitchf, SR), sessions=S, protect=BANK_WIDE["protect"], rms_mix_rate=BANK_WIDE["rms_mix_rate"],
                                    threhold=BANK_WIDE["threhold"], **kw)
        if values is not None:
            for s in range(S):
                bank.set_index_rate(s, values["index_rate"][s])
                bank.set_protect(s, values["protect"][s])
                bank.set_rms_mix_rate(s, values["rms_mix_rate"][s])
                bank.set_threhold(s, values["threhold"][s])
        return bank

    per_session, shared, all_blend = make_bank(own), make_bank(None), make_bank(sliders_for(S, all_blend=True))
    assert (shared.skip_head, shared.return_length, shared.input_wav_res_len // 160) == (250, 30, P_LEN)
    solos = [rvc_amd.RealtimeStream(SoloRVC(rvc_amd.RealtimeVC(net, index=index, index_rate=own["index_rate"][s], device=dev, tgt_sr=SR),
                                            feats[s:s + 1], pitch[s], pitchf[s], SR, own["protect"][s]),
                                    threhold=own["threhold"][s], rms_mix_rate=own["rms_mix_rate"][s], **kw) for s in range(S)]
    rng = np.random.default_rng(S)
    x = (0.3 * rng.standard_normal((reps + warmup, S, shared.block_frame))).astype(np.float32)
    x[:, :, : shared.block_frame // 3] *= np.float32(1e-3)   # a stretch that every gate closes on
    legs = (("bank_per_session", lambda j: per_session.process(x[j])), ("bank_shared", lambda j: shared.process(x[j])),
            ("solo_per_session", lambda j: [st.process(x[j, s]) for s, st in enumerate(solos)]),
            ("bank_per_session_all_blend", lambda j: all_blend.process(x[j])))
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
    row = dict(sessions=S, reps=reps, sliders=own, sessions_at_index_rate_0=sum(1 for r in own["index_rate"] if r == 0),
               sessions_ungated=sum(1 for t in own["threhold"] if t <= -60), sessions_unmixed=sum(1 for r in own["rms_mix_rate"] if r >= 1))
    for name, v in ts.items():
        v = np.array(v)
        row[name] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4))

    def disjoint(a, b):
        return bool(row[a]["max_ms"] < row[b]["min_ms"] or row[b]["max_ms"] < row[a]["min_ms"])

    def ratio(a, b):
        return round(row[a]["median_ms"] / row[b]["median_ms"], 3)

    row["per_session_over_shared"], row["per_session_vs_shared_ranges_disjoint"] = ratio("bank_per_session", "bank_shared"), disjoint("bank_per_session", "bank_shared")
    row["solo_over_bank"], row["bank_vs_solo_ranges_disjoint"] = ratio("solo_per_session", "bank_per_session"), disjoint("bank_per_session", "solo_per_session")
    row["all_blend_over_skipping"], row["skipping_vs_all_blend_ranges_disjoint"] = (ratio("bank_per_session_all_blend", "bank_per_session"),
                                                                                  disjoint("bank_per_session", "bank_per_session_all_blend"))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_bank_sliders_time.json"))
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
        fmt = lambda r: "%7.3f [%7.3f, %7.3f]" % (r["median_ms"], r["min_ms"], r["max_ms"])  # noqa: E731
        print("S %3d  (a) bank, per session %s  (b) bank, shared %s  (c) %d solo %s  (d) bank, all blend %s   a/b %.3f (disjoint %s)  c/a %.2f (disjoint %s)  "
              "d/a %.3f (disjoint %s)" % (S, fmt(row["bank_per_session"]), fmt(row["bank_shared"]), S, fmt(row["solo_per_session"]),
                                          fmt(row["bank_per_session_all_blend"]), row["per_session_over_shared"], row["per_session_vs_shared_ranges_disjoint"],
                                          row["solo_over_bank"], row["bank_vs_solo_ranges_disjoint"], row["all_blend_over_skipping"],
                                          row["skipping_vs_all_blend_ranges_disjoint"]), flush=True)
    res = dict(device=torch.cuda.get_device_name(dev),
               what="ms per block of S sessions (host wall time around a device synchronisation; eager, no hipGraph; no feeders): (a) RealtimeBank.process with "
                    "distinct index_rate / protect / rms_mix_rate / threhold per session (a quarter of the sessions at index_rate 0), (b) the same bank with "
                    "the shared bank-wide values (index_rate 0.75, protect 0.33, rms_mix_rate 0.25, threhold -40: the path without the setters), (c) S "
                    "RealtimeStream.process calls with the per-session values, (d) the bank of (a) with every session blending; device input gate; v2/48k "
                    "generator, 768-d front, 10000 x 768 index, 281 / 250 / 30 frames, 0.25 s block at 48 kHz; legs alternating in one process; ranges "
                    "that overlap are a tie",
               bank_wide=BANK_WIDE, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
