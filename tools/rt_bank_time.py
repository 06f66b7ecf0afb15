"""One block of S live streams: ``RealtimeBank`` (one pass for all sessions) against S solo ``RealtimeStream`` + ``RealtimeVC`` objects
(one pass each), on the ``stream`` leg's model -- v1/40k generator, 768-d front, the 10000 x 768 index, 282 / 250 / 31 frames (0.26 s
block at 40 kHz) -- WITHOUT the feeders: HuBERT features and the f0 estimator's output are fixed device tensors.  Timed is everything
after them: the block's host-to-device copy, the 16 kHz resample, retrieval (16 new rows per session, guarded), x2 + protect,
``net_g.infer`` (enc_p on 282 frames, flow on 56, decoder on 31), envelope mix and SOLA.

The project's convention: one process, the two legs alternating (A B A B ...), warm-up first, host wall time per block around a
device synchronisation, median and range over the repeats.  Writes profiles/rt_bank_time.json.

    python tools/rt_bank_time.py [--sessions 1,4,16,64] [--reps 12] [--warmup 4] [--out profiles/rt_bank_time.json]
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

SR, BLOCK_TIME, PROTECT, INDEX_RATE = 40000, 0.26, 0.33, 0.75
NF, P_LEN = 141, 282


class Net:
    """What the realtime classes need of ``net_g``: ``infer`` on the HIP front + generator (``rvc_amd.infer_hip``), torch's RNG for the noise."""

    def __init__(self, dev, max_B):
        import rvc_amd
        from oracle import nsf_oracle, synth
        from oracle.front_oracle import FrontConfig

        cfg, fcfg = nsf_oracle.CONFIGS["v1_40k"], FrontConfig()
        wf = synth.make_front_weights(fcfg, 1234)
        self.dec = rvc_amd.NSFGeneratorHIP(vars(cfg), synth.make_dec_weights(cfg, 1234), device=dev, operand="fp16", max_B=max_B, max_T=64)
        self.front = rvc_amd.FrontHIP(vars(fcfg), wf, device=dev, operand="fp16", max_B=max_B, max_T=288)
        emb = wf["emb_g.weight"].to(dev)
        self.emb_g = lambda sid: emb[sid]

    def infer(self, phone, lengths, sid, pitch=None, pitchf=None, skip_head=None, return_length=None, return_length2=None):
        import rvc_amd

        return rvc_amd.infer_hip(self, self.front, phone, lengths, sid, pitch, pitchf, skip_head, return_length, return_length2)


class SoloRVC:
    """``rtrvc.RVC``-like without feeders: fixed features and pitch, a ``RealtimeVC`` of its own."""

    def __init__(self, vc, feats, pitch, pitchf, tgt_sr):
        self.vc, self.feats, self.pitch, self.pitchf, self.tgt_sr = vc, feats, pitch, pitchf, tgt_sr

    def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
        return self.vc.infer(self.feats, int(input_wav_res.shape[0]), block_frame_16k, skip_head, return_length, pitch=self.pitch, pitchf=self.pitchf,
                             protect=PROTECT)


class BankRVC:
    def __init__(self, vc, feats, pitch, pitchf, tgt_sr):
        self.vc, self.feats, self.pitch, self.pitchf, self.tgt_sr = vc, feats, pitch, pitchf, tgt_sr

    def infer_batch(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method, keys, sids):
        return self.vc.infer(self.feats, int(input_wav_res.shape[1]), block_frame_16k, skip_head, return_length, pitch=self.pitch, pitchf=self.pitchf,
                             protect=PROTECT, sid=sids)


def measure(dev, net, index, S, reps, warmup):
    import rvc_amd
    from oracle import synth

    feats = torch.stack([synth.make_phone(1, NF, 768, 100 + s)[0] for s in range(S)]).to(dev)
    pitchf = synth.make_f0(S, P_LEN).to(dev)
    pitch = synth.make_pitch(pitchf.cpu()).to(dev)
    kw = dict(samplerate=SR, block_time=BLOCK_TIME, crossfade_time=0.05, extra_time=2.5, device=dev)
    vcb = rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=INDEX_RATE, device=dev, tgt_sr=SR)
    bank = rvc_amd.RealtimeBank(BankRVC(vcb, feats, pitch, pitchf, SR), sessions=S, **kw)
    assert (bank.skip_head, bank.return_length, bank.input_wav_res_len // 160) == (250, 31, P_LEN)
    solos = [rvc_amd.RealtimeStream(SoloRVC(rvc_amd.RealtimeVC(net, index=index, index_rate=INDEX_RATE, device=dev, tgt_sr=SR), feats[s:s + 1], pitch[s],
                                            pitchf[s], SR), **kw) for s in range(S)]
    x = (0.3 * np.random.default_rng(S).standard_normal((reps + warmup, S, bank.block_frame))).astype(np.float32)

    def run_bank(j):
        return bank.process(x[j])

    def run_solo(j):
        return [st.process(x[j, s]) for s, st in enumerate(solos)]

    ts = {"bank": [], "solo": []}
    for j in range(reps + warmup):
        for name, fn in (("bank", run_bank), ("solo", run_solo)):   # the two legs alternate
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = fn(j)
            torch.cuda.synchronize(dev)
            if j >= warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isfinite(out[0]).all())
    row = dict(sessions=S, reps=reps)
    for name, v in ts.items():
        v = np.array(v)
        row[name] = dict(median_ms=round(float(np.median(v)), 4), min_ms=round(float(v.min()), 4), max_ms=round(float(v.max()), 4),
                         streams_per_gpu=int(S * 256.0 / float(np.median(v))))
    row["ranges_disjoint"] = bool(row["bank"]["max_ms"] < row["solo"]["min_ms"] or row["solo"]["max_ms"] < row["bank"]["min_ms"])
    row["solo_over_bank"] = round(row["solo"]["median_ms"] / row["bank"]["median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rt_bank_time.json"))
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
        print("S %3d  bank %8.3f ms [%8.3f, %8.3f]  %d solo %8.3f ms [%8.3f, %8.3f]  solo/bank %.2f  disjoint %s  streams/GPU %d vs %d" % (
            S, row["bank"]["median_ms"], row["bank"]["min_ms"], row["bank"]["max_ms"], S, row["solo"]["median_ms"], row["solo"]["min_ms"],
            row["solo"]["max_ms"], row["solo_over_bank"], row["ranges_disjoint"], row["bank"]["streams_per_gpu"], row["solo"]["streams_per_gpu"]), flush=True)
    res = dict(device=torch.cuda.get_device_name(dev),
               what="ms per block of S sessions (host wall time around a device synchronisation; eager, no hipGraph; no feeders): RealtimeBank.process "
                    "against S RealtimeStream.process calls, each with its own RealtimeVC; v1/40k generator, 768-d front, 10000 x 768 index, "
                    "282 / 250 / 31 frames, 0.26 s block at 40 kHz, protect 0.33, index_rate 0.75; legs alternating in one process",
               streams_per_gpu="sessions * 256 ms / median ms per block: how many 256 ms streams one GPU serves at that rate (feeders not included)",
               rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
