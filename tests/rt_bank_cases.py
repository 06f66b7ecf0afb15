"""Inputs shared by tests/test_gpu_rt_bank.py and tools/rt_bank_parity.py (which measures, on the same inputs, how far the existing
``net_g.infer`` at batch 3 is from batch 1 and writes profiles/rt_bank_parity.json: the bar of the bank-against-solo comparisons).

Everything here is seeded and built without a GPU unless a ``dev`` is passed in."""
import json
import os
import types

import numpy as np
import torch

from oracle import nsf_oracle, synth
from oracle.front_oracle import FrontConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY_JSON = os.path.join(ROOT, "profiles", "rt_bank_parity.json")

# the geometry of the realtime golden infer_full_v2_48k_rt (oracle/make_golden.py): 70 frames, skip_head 40, return_length 20
T, SKIP_HEAD, RETURN_LENGTH, WINDOW = 70, 40, 20, 160
N_INPUT = T * WINDOW            # samples of the rolling 16 kHz window
N_FEATS = T // 2 - 1            # HuBERT frames of that window ((N_INPUT - 400) // 320 + 1); rtrvc.py:163 repeats the last one
BLOCK_16K = 1600                # the cache rolls by 10 frames per block
MODEL_SEED = 1234               # the fixture's seed: the same synthetic v2/48k weights
PROTECT, INDEX_RATE = 0.33, 0.75


class BankNet:
    """What ``RealtimeVC`` needs of ``net_g`` (``infer``, through ``rvc_amd.infer_hip``: front + generator on the HIP path), on the seeded
    synthetic v2/48k weights.  The two noise draws of ``infer`` are fixed PER SESSION (row ``i`` of ``noise_*``), so a batched call and the
    solo call of session ``i`` see the same noise: ``rows`` selects the sessions of the next call."""

    def __init__(self, dev, sessions: int, max_T: int = T, skip_head: int = SKIP_HEAD, return_length: int = RETURN_LENGTH):
        import rvc_amd

        cfg, fcfg = nsf_oracle.CONFIGS["v2_48k"], FrontConfig()
        wf = synth.make_front_weights(fcfg, MODEL_SEED)
        self.dec = rvc_amd.NSFGeneratorHIP(vars(cfg), synth.make_dec_weights(cfg, MODEL_SEED), device=dev, operand="fp16", max_B=sessions, max_T=64)
        self.front = rvc_amd.FrontHIP(vars(fcfg), wf, device=dev, operand="fp16", max_B=sessions, max_T=max_T)
        emb = wf["emb_g.weight"].to(dev)
        self.emb_g = lambda sid: emb[sid]
        gen = torch.Generator().manual_seed(99)
        self.noise_zp = torch.randn(sessions, 192, max_T - max(skip_head - 24, 0), generator=gen).to(dev)
        self.noise_dec = torch.randn(sessions, return_length * cfg.upp, generator=gen).to(dev)
        self.rows = slice(0, sessions)
        self.upp = cfg.upp

    def infer(self, phone, lengths, sid, pitch=None, pitchf=None, skip_head=None, return_length=None, return_length2=None):
        import rvc_amd

        return rvc_amd.infer_hip(self, self.front, phone, lengths, sid, pitch, pitchf, skip_head, return_length, return_length2,
                                 noise_zp=self.noise_zp[self.rows], noise_dec=self.noise_dec[self.rows])


def index_768():
    """A small 768-d IVF index (host arrays) for the v2 front."""
    x, centres = synth.make_clustered_rows(3000, 768, 30, seed=11, return_centres=True)
    return synth.make_ivf_from_rows(x, 30, kmeans_iters=1, init=centres)


def vc_blocks(sessions: int = 3, blocks: int = 2):
    """Per block: (feats [S, N_FEATS, 768], pitch [S, T] int64, pitchf [S, T] float32), distinct per session and block.  The pitch
    block has exactly p_len = T frames, so that protect < 0.5 applies (rtrvc.py:229)."""
    out = []
    f0 = synth.make_f0(1, T + 64)[0]
    for b in range(blocks):
        feats = torch.stack([synth.make_phone(1, N_FEATS, 768, 500 + 10 * b + s)[0] for s in range(sessions)])
        pitchf = torch.stack([f0[7 * s + 3 * b: 7 * s + 3 * b + T] * (1.0 + 0.05 * s) for s in range(sessions)]).contiguous()
        out.append((feats, synth.make_pitch(pitchf), pitchf))
    return out


SIDS = [1, 1, 2]   # two distinct speakers over three sessions


def solo_operands(net, index, dev, blocks, sids=SIDS):
    """The operands ``net_g.infer`` gets from the EXISTING single-stream code, per block and session: a ``RealtimeVC`` per session whose
    ``net_g`` only records.  -> list over blocks of lists over sessions of dict(phone, pitch, pitchf)."""
    import rvc_amd

    seen = {}

    class Rec:
        def infer(self, phone, lengths, sid, pitch=None, pitchf=None, skip_head=None, return_length=None, return_length2=None):
            seen.update(phone=phone.clone(), pitch=pitch.clone(), pitchf=pitchf.clone())
            return torch.zeros(1, 1, 8, device=phone.device)

    S = blocks[0][0].shape[0]
    rts = [rvc_amd.RealtimeVC(Rec(), index=index, index_rate=INDEX_RATE, device=dev, tgt_sr=48000) for _ in range(S)]
    out = []
    for feats, pitch, pitchf in blocks:
        row = []
        for s in range(S):
            rts[s].infer(feats[s:s + 1].to(dev), N_INPUT, BLOCK_16K, SKIP_HEAD, RETURN_LENGTH, pitch=pitch[s].to(dev), pitchf=pitchf[s].to(dev),
                         protect=PROTECT, sid=sids[s])
            row.append(dict(seen))
        out.append(row)
    return out


def direct_batch(net, ops, dev, sids=SIDS):
    """``net_g.infer`` at batch S on the stacked per-session operands of one block -> [S, L]."""
    S = len(ops)
    net.rows = slice(0, S)
    phone = torch.cat([o["phone"] for o in ops])
    lengths = torch.full((S,), phone.shape[1], dtype=torch.long, device=dev)
    out = net.infer(phone, lengths, torch.tensor(sids[:S], dtype=torch.long, device=dev), pitch=torch.cat([o["pitch"] for o in ops]),
                    pitchf=torch.cat([o["pitchf"] for o in ops]), skip_head=SKIP_HEAD, return_length=RETURN_LENGTH, return_length2=RETURN_LENGTH)
    return out.squeeze(1).float()


def direct_solo(net, op, s, dev, sids=SIDS):
    """``net_g.infer`` at batch 1 on session ``s``'s operands (its own noise rows) -> [L]."""
    net.rows = slice(s, s + 1)
    lengths = torch.full((1,), op["phone"].shape[1], dtype=torch.long, device=dev)
    out = net.infer(op["phone"], lengths, torch.tensor([sids[s]], dtype=torch.long, device=dev), pitch=op["pitch"], pitchf=op["pitchf"],
                    skip_head=SKIP_HEAD, return_length=RETURN_LENGTH, return_length2=RETURN_LENGTH)
    return out.squeeze(1).float()[0]


def recorded_bar(which: str = "batch3_vs_batch1"):
    """(max_abs, rms) of profiles/rt_bank_parity.json: the measured distance of the existing ``net_g.infer`` at batch S from batch 1 on the
    operands of the test that asks -- ``batch3_vs_batch1``: ``vc_blocks()``; ``batch2_vs_batch1_end_to_end_operands``: what the solo
    ``rvc_infer_hip`` hands to ``net_g.infer`` on ``e2e_waves()``.  (0, 0) means the bank must equal the solo run bit for bit."""
    d = json.load(open(PARITY_JSON))[which]
    return float(d["max_abs"]), float(d["rms"])


def within_bar(got: torch.Tensor, ref: torch.Tensor, bar) -> bool:
    if bar[0] == 0.0 and bar[1] == 0.0:
        return torch.equal(got, ref)
    e = (got.double() - ref.double())
    return float(e.abs().max()) <= bar[0] and float(e.pow(2).mean().sqrt()) <= bar[1]


# ---- stub feeders for rvc_infer_hip / rvc_infer_batch_hip: framing + element-wise operations only (no GEMM, no reduction), so a row of
# a batched call is the same bits as the call on that row alone whatever algorithm torch picks -------------------------------------------

class FramingHubert:
    """``extract_features(source [B, n], padding_mask, output_layer)`` -> ``(feats [B, (n - 400) // 320 + 1, 768],)``: channel ``c`` of frame
    ``t`` is a sine of ONE sample of that frame."""

    def __init__(self):
        self.calls, self.batches = 0, []

    def extract_features(self, source, padding_mask, output_layer):
        assert source.dim() == 2 and padding_mask.shape == source.shape and not bool(padding_mask.any()) and output_layer == 12
        self.calls += 1
        self.batches.append(int(source.shape[0]))
        fr = source.float().unfold(1, 400, 320)                                   # [B, n_frames, 400]
        c = torch.arange(768, device=source.device)
        x = fr[:, :, (c * 7) % 400]                                               # [B, n_frames, 768]
        return (0.5 * torch.sin(37.0 * x + 0.1 * c.float()),)


class FramingRMVPE:
    """``mel_extractor(audio [B, n], center=True)`` -> [B, 128, n // 160 + 1] (samples, framed) and ``_mel2hidden(mel)`` -> salience
    [B, frames, 360]: a bump of height 0.9 around a bin that follows the frame's first sample, 0 on 'unvoiced' frames."""

    def __init__(self, device):
        self.device, self.is_half = device, False
        self.mel_calls, self.batches = 0, []
        self.mel_extractor = self._mel

    def _mel(self, audio, center=True):
        assert audio.dim() == 2 and center
        self.mel_calls += 1
        self.batches.append(int(audio.shape[0]))
        n = int(audio.shape[1])
        t = torch.arange(n // 160 + 1, device=audio.device)[None, :] * 160 + torch.arange(128, device=audio.device)[:, None]
        return audio.float()[:, t.clamp(max=n - 1)]                               # [B, 128, frames]

    def _mel2hidden(self, mel):
        x = mel[:, 0, :]                                                          # [B, frames]
        centre = 150.0 + 120.0 * torch.tanh(4.0 * x)
        j = torch.arange(360, device=mel.device, dtype=torch.float32)
        sal = 0.9 * torch.exp(-0.5 * ((j[None, None, :] - centre[:, :, None]) / 2.0) ** 2)
        return sal * (mel[:, 1, :].abs() > 0.02)[:, :, None]


def stub_rvc(net, index, dev, key):
    """An ``rtrvc.RVC``-like object around the stub feeders, as ``rvc_infer_hip`` reads it."""
    def no_host_f0(*a, **k):
        raise AssertionError("the host f0 path must not run")

    return types.SimpleNamespace(index=index, net_g=net, index_rate=INDEX_RATE, device=dev, if_f0=1, tgt_sr=48000, f0_up_key=key, formant_shift=0,
                                 window=WINDOW, is_half=False, version="v2", hubert=FramingHubert(),
                                 f0_gen=types.SimpleNamespace(rmvpe=FramingRMVPE(dev), is_half=False, device=dev), _get_f0=no_host_f0)


def e2e_waves(sessions: int = 2, blocks: int = 2):
    """[blocks][S, N_INPUT] float32: every session's rolling 16 kHz window per block (distinct signals)."""
    return [torch.from_numpy(np.stack([synth.make_audio16k(N_INPUT, 40 + 5 * b + s) for s in range(sessions)])) for b in range(blocks)]


E2E_KEYS = [2, -3]


# ---- the per-session guard (test group 2) ---------------------------------------------------------------------------------------------

def guard_index(short: bool = True):
    """d = 256, 4000 rows; with ``short`` the last list holds 3 vectors (a tight far-away cluster), else every list is long.
    -> (index dict as oracle/ivf_oracle.py takes it, the short list's centroid or None)."""
    def base(n):   # clustered rows: 40 lists of about 100 rows each (i.i.d. Gaussian rows leave lists of 2 .. 400)
        x, centres = synth.make_clustered_rows(n, 256, 40, seed=21, return_centres=True)
        return synth.make_ivf_from_rows(x, 40, kmeans_iters=1, init=centres)

    if not short:
        return base(4000), None
    idx = base(3997)
    rng = np.random.default_rng(5)
    far = np.zeros(256, np.float32)
    far[:8] = 40.0
    v3 = (far[None] + 0.05 * rng.standard_normal((3, 256))).astype(np.float32)
    cent = v3.astype(np.float64).mean(0).astype(np.float32)
    out = dict(d=256, ntotal=4000, nlist=41, nprobe=1, centroids=np.vstack([idx["centroids"], cent[None]]).astype(np.float32),
               list_offsets=np.append(idx["list_offsets"], 4000).astype(np.int64), ids=np.append(idx["ids"], [3997, 3998, 3999]).astype(np.int64),
               vecs=np.vstack([idx["vecs"], v3]).astype(np.float32))
    return out, cent


GUARD_S, GUARD_NQ, GUARD_SKIP, GUARD_PLEN = 3, 12, 4, 23


def guard_feats(centroid):
    """feats [3, 12, 256]; with a ``centroid`` session 1's searched rows (4 ..) sit at it (a hair of noise keeps them distinct)."""
    feats = torch.stack([synth.make_phone(1, GUARD_NQ, 256, 700 + s)[0] for s in range(GUARD_S)])
    if centroid is not None:
        g = torch.Generator().manual_seed(3)
        feats[1, GUARD_SKIP:] = torch.from_numpy(centroid)[None] + 0.01 * torch.randn(GUARD_NQ - GUARD_SKIP, 256, generator=g)
    pitchf = torch.stack([synth.make_f0(1, 64)[0, 30 + 5 * s: 30 + 5 * s + GUARD_PLEN] for s in range(GUARD_S)]).contiguous()
    return feats.contiguous(), pitchf
