"""Inputs shared by tests/test_cpu_rt_formant.py, tests/test_gpu_nsf_nres_ragged.py, tests/test_gpu_rt_formant.py and
tools/rt_bank_formant_parity.py (which measures, on the same inputs, how far the existing ``net_g.infer`` at batch 3 with ONE shared
``return_length2`` is from its batch-1 calls and writes profiles/rt_bank_formant_parity.json: the bar of the bank-against-solo comparisons).

Everything here is seeded and built without a GPU unless a ``dev`` is passed in."""
import json
import os

import numpy as np
import torch

import rt_bank_cases as bank

ROOT = bank.ROOT
PARITY_JSON = os.path.join(ROOT, "profiles", "rt_bank_formant_parity.json")

TGT_SR = 48000
SLIDER = [round(0.05 * i, 2) for i in range(-40, 41)]     # the GUI's formant slider: -2 .. 2 in steps of 0.05 (gui.py)
RATES = (32000, 40000, 48000)
RETURN_LENGTHS = (20, 60, 100)

# RealtimeVCBatch: three sessions, a longer, an equal and a shorter decode (return_length2 23, 20, 19; upp_res 538, 480, 443 by rtrvc.py:248)
FORMANTS = [2.0, 0.0, -1.35]
# rvc_infer_batch_hip end to end: fractional f0 keys key - shift (return_length2 21, 20, 20; upp_res 494, 480, 466)
E2E_FORMANTS = [0.5, 0.0, -0.5]
E2E_KEYS = [2, -3, 0]


def reference_geometry(shift, return_length, tgt_sr):
    """infer/lib/rtrvc.py:190-191, 248, written out."""
    factor = pow(2, shift / 12)
    return_length2 = int(np.ceil(return_length * factor))
    upp_res = int(np.floor(factor * tgt_sr // 100))
    return factor, return_length2, upp_res


def geometry(shift, return_length=bank.RETURN_LENGTH, tgt_sr=TGT_SR):
    return reference_geometry(shift, return_length, tgt_sr)[1:]


def solo_operands(index, dev, blocks, formants, sids=bank.SIDS):
    """``rt_bank_cases.solo_operands`` with a formant shift per session: what ``net_g.infer`` gets from the EXISTING single-stream
    ``RealtimeVC(formant_shift=formants[s])``, per block and session -> list over blocks of lists over sessions of dict(phone, pitch, pitchf)."""
    import rvc_amd

    seen = {}

    class Rec:
        def infer(self, phone, lengths, sid, pitch=None, pitchf=None, skip_head=None, return_length=None, return_length2=None):
            seen.update(phone=phone.clone(), pitch=pitch.clone(), pitchf=pitchf.clone(), return_length2=return_length2)
            return torch.zeros(1, 1, 8, device=phone.device)

    S = blocks[0][0].shape[0]
    rts = [rvc_amd.RealtimeVC(Rec(), index=index, index_rate=bank.INDEX_RATE, device=dev, tgt_sr=TGT_SR, formant_shift=formants[s]) for s in range(S)]
    out = []
    for feats, pitch, pitchf in blocks:
        row = []
        for s in range(S):
            rts[s].infer(feats[s:s + 1].to(dev), bank.N_INPUT, bank.BLOCK_16K, bank.SKIP_HEAD, bank.RETURN_LENGTH, pitch=pitch[s].to(dev),
                         pitchf=pitchf[s].to(dev), protect=bank.PROTECT, sid=sids[s])
            row.append(dict(seen))
        out.append(row)
    return out


def direct_batch(net, ops, dev, return_length2, sids=bank.SIDS):
    """``net_g.infer`` at batch S on the stacked per-session operands of one block, ``return_length2`` an int (the existing call) or a
    list of S ints (the per-item decode) -> [S, max(return_length2) * upp]."""
    S = len(ops)
    net.rows = slice(0, S)
    phone = torch.cat([o["phone"] for o in ops])
    lengths = torch.full((S,), phone.shape[1], dtype=torch.long, device=dev)
    out = net.infer(phone, lengths, torch.tensor(sids[:S], dtype=torch.long, device=dev), pitch=torch.cat([o["pitch"] for o in ops]),
                    pitchf=torch.cat([o["pitchf"] for o in ops]), skip_head=bank.SKIP_HEAD, return_length=bank.RETURN_LENGTH,
                    return_length2=return_length2)
    return out.squeeze(1).float()


def direct_solo(net, op, s, dev, return_length2, sids=bank.SIDS):
    """``net_g.infer`` at batch 1 on session ``s``'s operands (its own noise rows) -> [return_length2 * upp]."""
    net.rows = slice(s, s + 1)
    lengths = torch.full((1,), op["phone"].shape[1], dtype=torch.long, device=dev)
    out = net.infer(op["phone"], lengths, torch.tensor([sids[s]], dtype=torch.long, device=dev), pitch=op["pitch"], pitchf=op["pitchf"],
                    skip_head=bank.SKIP_HEAD, return_length=bank.RETURN_LENGTH, return_length2=int(return_length2))
    return out.squeeze(1).float()[0]


_RS = {}


def solo_resample(row, upp_res, dev, return_length=bank.RETURN_LENGTH, tgt_sr=TGT_SR):
    """What ``RealtimeVC.infer`` does to one decoded row (realtime.py, rtrvc.py:248-259) with the EXISTING ``SincResample``; a row whose
    ``upp_res`` is the model's own rate is its first ``return_length * tgt_sr // 100`` samples (the bank's equal-rows rule)."""
    import rvc_amd

    new = tgt_sr // 100
    if upp_res == new:
        return row[: return_length * new]
    key = (upp_res, new, str(dev))
    if key not in _RS:
        _RS[key] = rvc_amd.SincResample(upp_res, new, dev)
    return _RS[key](row[None, : return_length * upp_res].contiguous())[0]


def recorded_bar(section: str, shift: float, factor: float = 2.0):
    """``factor`` x the (max_abs, rms) that profiles/rt_bank_formant_parity.json records under ``section`` for the shift's
    ``return_length2``: the measured distance of the EXISTING batch-3 ``net_g.infer`` + per-row ``SincResample`` from the batch-1 calls, all
    sessions at that one shift.  Twice, because a mixed batch is neither of the two launches measured: the generator's plan follows B and the
    longest item, so its rounding differs from both, from the same cause.  (0, 0) stays (0, 0): bit equality."""
    d = json.load(open(PARITY_JSON))[section]["%.2f" % shift]
    assert int(d["return_length2"]) == geometry(shift)[0]
    return factor * float(d["max_abs"]), factor * float(d["rms"])


def e2e_solo_rvc(net, index, dev, key, shift, keys_seen):
    """``rt_bank_cases.stub_rvc`` for one solo session with a formant shift.  The solo ``rvc_infer_hip`` hands a fractional f0 key to the
    object's own ``_get_f0`` (the device chain takes integral keys unless the opt-in RMVPE switch is on); this one runs the stub feeders and
    the existing fractional-key decode ``glue.rmvpe_f0`` -- what the bank does for every session -- and records the key it was given."""
    import rvc_amd
    from rvc_amd.pipeline import RMVPE_THRED

    rvc = bank.stub_rvc(net, index, dev, key)
    rvc.formant_shift = shift

    def get_f0(wav, f0_up_key, method="rmvpe"):
        keys_seen.append(f0_up_key)
        r = rvc.f0_gen.rmvpe
        hidden = r._mel2hidden(r.mel_extractor(wav.float().to(dev)[None], center=True))
        p, pf = rvc_amd.glue.rmvpe_f0(hidden[0].float(), int(wav.shape[0]) // bank.WINDOW, float(f0_up_key), RMVPE_THRED)
        return p[0], pf[0]

    rvc._get_f0 = get_f0
    return rvc
