"""The realtime bank's formant shift per session.

1. the ragged resampler (``rvcmi_glue_resample_poly_ragged``) is bit-equal, per row, to the existing ``SincResample`` of that row's ratio, or
   the head copy; 2. ``RealtimeVCBatch`` with a shift per session against a direct per-item ``net_g.infer`` (bit for bit) and against solo
   ``RealtimeVC(formant_shift=f_i)`` objects (recorded bar); 3. ``rvc_infer_batch_hip(formants=...)`` end to end with stub feeders; 4. the launch
   count of ``RealtimeBank``; 5. what stays refused."""
import numpy as np
import pytest
import torch

import rt_bank_cases as cases
import rt_formant_cases as fc

pytestmark = pytest.mark.gpu

S = 3


def _rows(t, pad_l, pad_r, gpu):
    """``t`` [S, n] as row slices of a longer device buffer (7.0 around them)."""
    big = torch.full((t.shape[0], pad_l + t.shape[1] + pad_r), 7.0, device=gpu, dtype=torch.float32)
    view = big[:, pad_l: pad_l + t.shape[1]]
    view.copy_(t)
    assert view.stride(0) != view.shape[1] and not view.is_contiguous()
    return view


# ---- 1. the ragged resampler ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("new,origs", [(480, (538, 480, 444)), (320, (359, 320, 296, 359))])
def test_ragged_resample_rows_equal_sinc_resample_bit_for_bit(new, origs, gpu):
    """48 kHz: +2, 0 and about -1.35 semitones; 32 kHz: a 320 -> 320 row (the un-resampled edge: the head copy) between an up and a down
    ratio, and two rows that share a table.  Rows are views into longer buffers; the longest row's taps hang over its end (zeros there, not
    the 7.0 behind the slice)."""
    import rvc_amd

    frames = 20
    n = frames * max(origs)
    x = torch.from_numpy((0.3 * np.random.default_rng(new).standard_normal((len(origs), n))).astype(np.float32))
    view = _rows(x, 9, 40, gpu)
    rs = rvc_amd.SincResampleRagged(new, gpu)
    got = rs(view, origs, frames)
    assert got.shape == (len(origs), frames * new) and got.is_contiguous() and rs.rebuilds == 1
    for s, o in enumerate(origs):
        row = x[s, : frames * o].to(gpu).contiguous()
        ref = row[: frames * new] if o == new else rvc_amd.SincResample(o, new, gpu)(row)
        assert ref.shape == (frames * new,)
        assert torch.equal(got[s], ref), "row %d (%d -> %d): max abs %.3e" % (s, o, new, float((got[s] - ref).abs().max()))
    assert torch.equal(rs(view, origs, frames), got) and rs.rebuilds == 1        # nothing rebuilt, nothing uploaded
    swapped = tuple(reversed(origs))
    got2 = rs(view, swapped, frames)
    assert rs.rebuilds == 2
    for s, o in enumerate(swapped):
        row = x[s, : frames * o].to(gpu).contiguous()
        assert torch.equal(got2[s], row[: frames * new] if o == new else rvc_amd.SincResample(o, new, gpu)(row))


def test_ragged_resample_rejects_bad_arguments(gpu):
    import rvc_amd
    from rvc_amd import _lib

    rs = rvc_amd.SincResampleRagged(480, gpu)
    x = torch.zeros(S, 20 * 538, device=gpu)
    rs(x, (538, 480, 444), 20)
    table, desc, _ = rs._dev
    out = torch.zeros(S, 9600, device=gpu)
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu)
    n = int(x.shape[1])
    with torch.cuda.device(gpu):
        assert L.rvcmi_glue_resample_poly_ragged(S, p(x), n, n, p(table), table.numel(), p(desc), p(out), 9600, 9600, st) == 0
        assert L.rvcmi_glue_resample_poly_ragged(0, p(x), n, n, p(table), table.numel(), p(desc), p(out), 9600, 9600, st) == _lib.ERR_INVALID
        assert L.rvcmi_glue_resample_poly_ragged(S, p(x), n - 1, n, p(table), table.numel(), p(desc), p(out), 9600, 9600, st) == _lib.ERR_INVALID
        assert L.rvcmi_glue_resample_poly_ragged(S, p(x), n, n, p(table), table.numel(), p(desc), p(out), 9599, 9600, st) == _lib.ERR_INVALID
        assert L.rvcmi_glue_resample_poly_ragged(S, p(x), n, n, p(table), table.numel(), None, p(out), 9600, 9600, st) == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        rs(x, (538, 480), 20)                     # two rates for three rows
    with pytest.raises(ValueError):
        rs(x[:, :-1], (538, 480, 444), 20)        # a row shorter than its input
    with pytest.raises(rvc_amd.RvcmiError):
        rs(x.cpu(), (538, 480, 444), 20)
    torch.cuda.synchronize(gpu)


# ---- 2. RealtimeVCBatch -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vc_setup(gpu):
    import rvc_amd

    idx = cases.index_768()
    index = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=gpu)
    return cases.BankNet(gpu, S), index


def _report(what, got, ref, bar):
    e = got.double() - ref.double()
    msg = "%s: max abs %.3e rms %.3e (bar %.3e / %.3e)" % (what, float(e.abs().max()), float(e.pow(2).mean().sqrt()), bar[0], bar[1])
    print(msg)
    return msg


def test_realtime_vc_batch_with_a_formant_shift_per_session(vc_setup, gpu):
    """Two consecutive blocks (the cache roll), shifts +2, 0 and -1.35 semitones (return_length2 23, 20, 19).  (a) row i == the existing
    per-row ``SincResample`` of row i of a direct ``net_g.infer`` at batch 3 with the ``return_length2`` LIST, on the operands three solo
    ``RealtimeVC(formant_shift=f_i)`` prepare: isolates the new Python and the ragged resampler, bit for bit.  (b) row i against the solo
    ``RealtimeVC(formant_shift=f_i).infer`` under twice the recorded distance of the existing batch-3 ``infer`` with that ONE
    ``return_length2`` from its batch-1 calls (profiles/rt_bank_formant_parity.json, tools/rt_bank_formant_parity.py).  (c) the pitch caches
    equal the solo ones."""
    import rvc_amd

    net, index = vc_setup
    blocks = cases.vc_blocks(S, 2)
    fm = fc.FORMANTS
    geo = [fc.geometry(f) for f in fm]
    assert [g[0] for g in geo] == [23, 20, 19]
    ops = fc.solo_operands(index, gpu, blocks, fm)
    bank = rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000)
    for s in range(S):
        bank.set_session_formant(s, fm[s])
    solos = [rvc_amd.RealtimeVC(net, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000, formant_shift=fm[s]) for s in range(S)]
    bars = [fc.recorded_bar("batch3_vs_batch1", f) for f in fm]
    L = cases.RETURN_LENGTH * 480
    for b, (feats, pitch, pitchf) in enumerate(blocks):
        net.rows = slice(0, S)
        got = bank.infer(feats.to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, pitch=pitch.to(gpu),
                         pitchf=pitchf.to(gpu), protect=cases.PROTECT, sid=cases.SIDS)
        assert got.shape == (S, L) and bool(torch.isfinite(got).all())
        assert [o["return_length2"] for o in ops[b]] == [g[0] for g in geo]
        direct = fc.direct_batch(net, ops[b], gpu, [g[0] for g in geo])
        assert direct.shape == (S, 23 * net.upp)
        for s in range(S):
            assert not direct[s, geo[s][0] * net.upp:].any()
            ref = fc.solo_resample(direct[s], geo[s][1], gpu)
            assert torch.equal(got[s], ref), "block %d session %d: max abs %.3e from the direct per-item infer + SincResample" % (
                b, s, float((got[s] - ref).abs().max()))
        for s in range(S):
            net.rows = slice(s, s + 1)
            solo = solos[s].infer(feats[s:s + 1].to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, pitch=pitch[s].to(gpu),
                                  pitchf=pitchf[s].to(gpu), protect=cases.PROTECT, sid=cases.SIDS[s])
            assert solo.shape == (L,)
            msg = _report("block %d session %d (shift %+.2f)" % (b, s, fm[s]), got[s], solo, bars[s])
            assert cases.within_bar(got[s], solo, bars[s]), msg
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])
    for s in range(S):
        assert torch.equal(bank.pitch[s], solos[s].cache.pitch) and torch.equal(bank.pitchf[s], solos[s].cache.pitchf)


def test_a_bank_without_shifts_is_the_bank_before(vc_setup, gpu):
    """(d) all shifts zero, shifts passed as zeros, and shifts set and cleared again: the same bits as an untouched ``RealtimeVCBatch``,
    and ``net_g.infer`` is handed the plain int."""
    import rvc_amd

    net, index = vc_setup
    blocks = cases.vc_blocks(S, 2)
    seen = []
    inner = net.infer

    def spy(*a, **k):
        seen.append(k.get("return_length2"))
        return inner(*a, **k)

    mk = lambda: rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000)  # noqa: E731
    plain, zeros, cleared = mk(), mk(), mk()
    net.infer = spy
    try:
        for b, (feats, pitch, pitchf) in enumerate(blocks):
            net.rows = slice(0, S)
            args = (feats.to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH)
            kw = dict(pitch=pitch.to(gpu), pitchf=pitchf.to(gpu), protect=cases.PROTECT, sid=cases.SIDS)
            ref = plain.infer(*args, **kw)
            assert torch.equal(zeros.infer(*args, formants=[0, 0.0, 0], **kw), ref)
            if b == 0:
                for s in range(S):
                    cleared.set_session_formant(s, fc.FORMANTS[s])
                shifted = cleared.infer(*args, **kw)
                assert shifted.shape == ref.shape and not torch.equal(shifted[0], ref[0])
                assert torch.equal(cleared.pitch, plain.pitch) and torch.equal(cleared.pitchf, plain.pitchf)   # the caches do not see the shift
            else:
                for s in range(S):
                    cleared.set_session_formant(s, 0.0)
                assert torch.equal(cleared.infer(*args, **kw), ref)
    finally:
        net.infer = inner
    assert seen == [20, 20, [23, 20, 19], 20, 20, 20]


# ---- 3. rvc_infer_batch_hip end to end ----------------------------------------------------------------------------------------------------

def test_rvc_infer_batch_hip_with_formants_against_solo_rvc_infer_hip(vc_setup, gpu, monkeypatch):
    """Stub feeders (batch-invariant by construction), three sessions with keys 2, -3, 0 and shifts +0.5, 0, -0.5, two blocks: each session
    against its solo ``rvc_infer_hip`` with that ``formant_shift`` under twice the distance recorded for its shift on these operands; the f0
    decode of session s is asked for ``key - shift``, the solo object's own key."""
    import rvc_amd
    from rvc_amd.realtime import rvc_infer_batch_hip, rvc_infer_hip

    net, index = vc_setup
    keys, fm = fc.E2E_KEYS, fc.E2E_FORMANTS
    both = cases.stub_rvc(net, index, gpu, 0)
    solo_keys = [[] for _ in range(S)]
    solos = [fc.e2e_solo_rvc(net, index, gpu, keys[s], fm[s], solo_keys[s]) for s in range(S)]
    bars = [fc.recorded_bar("batch3_vs_batch1_end_to_end_operands", f) for f in fm]
    asked = []
    real = rvc_amd.glue.rmvpe_f0
    for b, wav in enumerate(cases.e2e_waves(S, 2)):
        w = wav.to(gpu)
        net.rows = slice(0, S)
        monkeypatch.setattr(rvc_amd.glue, "rmvpe_f0", lambda sal, m, key, *a, **k: (asked.append(key), real(sal, m, key, *a, **k))[1])
        got = rvc_infer_batch_hip(both, w, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0, keys=keys, sids=[0, 0, 0], formants=fm)
        monkeypatch.setattr(rvc_amd.glue, "rmvpe_f0", real)
        assert got.shape == (S, cases.RETURN_LENGTH * net.upp) and bool(torch.isfinite(got).all())
        assert asked[-S:] == [keys[s] - fm[s] if fm[s] else keys[s] for s in range(S)] == [1.5, -3, 0.5]
        for s in range(S):
            net.rows = slice(s, s + 1)
            ref = rvc_infer_hip(solos[s], w[s], cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0)
            msg = _report("block %d session %d (shift %+.2f)" % (b, s, fm[s]), got[s], ref, bars[s])
            assert cases.within_bar(got[s], ref, bars[s]), msg
            assert torch.equal(both._rvcmi_rt_bank.pitch[s], solos[s]._rvcmi_rt.cache.pitch)
            assert torch.equal(both._rvcmi_rt_bank.pitchf[s], solos[s]._rvcmi_rt.cache.pitchf)
    assert solo_keys == [[1.5, 1.5], [], [0.5, 0.5]]   # the solo objects with a shift asked their own f0 method for key - shift
    assert both._rvcmi_rt_bank.formants == fm and both.hubert.batches == [S, S] and both.f0_gen.rmvpe.batches == [S, S]
    with pytest.raises(ValueError):
        rvc_infer_batch_hip(both, w, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0, keys=keys, sids=[0, 0, 0], formants=[0.5])
    both.formant_shift = 0.5
    with pytest.raises(ValueError, match="formant"):
        rvc_infer_batch_hip(both, w, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0, keys=keys, sids=[0, 0, 0])


# ---- 4. RealtimeBank: the launch count --------------------------------------------------------------------------------------------------

BANK_KW = dict(samplerate=48000, block_time=0.15, crossfade_time=0.14, extra_time=0.4)   # 70 frames, skip_head 40, return_length 20


class _BankRVC:
    """``rtrvc.RVC``-like without feeders (fixed HuBERT features and f0 per session) around a ``RealtimeVCBatch``; ``formants`` arrives only
    while some session is shifted, and is recorded."""

    def __init__(self, vc, feats, pitch, pitchf):
        self.vc, self.feats, self.pitch, self.pitchf, self.tgt_sr, self.seen = vc, feats, pitch, pitchf, 48000, []

    def infer_batch(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method, keys, sids, **kw):
        assert set(kw) <= {"formants"}
        self.seen.append(kw.get("formants"))
        return self.vc.infer(self.feats, int(input_wav_res.shape[1]), block_frame_16k, skip_head, return_length, pitch=self.pitch, pitchf=self.pitchf,
                             protect=cases.PROTECT, sid=sids, formants=kw.get("formants", [0.0] * self.vc.S))


def _launches(fn, gpu):
    """Kernels and device-to-device copies ``fn`` enqueues, by torch.profiler (as tests/test_gpu_rt_bank_nr.py counts them)."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize(gpu)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(gpu)
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sorted(n for n in names if "memset" not in n.lower() and not ("memcpy" in n.lower() and "dtod" not in n.lower()))


def _diff(a, b):
    from collections import Counter

    ca, cb = Counter(n[:60] for n in a), Counter(n[:60] for n in b)
    return "only in the first: %r; only in the second: %r" % (dict(ca - cb), dict(cb - ca))


def _warm_bank(net, index, gpu, n, shifts, clear=False):
    """A bank of n sessions after two blocks with ``shifts`` (None: never touched); ``clear``: the shifts are set back to 0 and one more
    block runs; -> (bank, a closure that processes the next block)."""
    import rvc_amd

    feats, pitch, pitchf = (t[:n].to(gpu) for t in cases.vc_blocks(S, 1)[0])
    vc = rvc_amd.RealtimeVCBatch(net, n, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000)
    bank = rvc_amd.RealtimeBank(_BankRVC(vc, feats, pitch, pitchf), sessions=n, device=gpu, **BANK_KW)
    assert (bank.skip_head, bank.return_length, bank.input_wav_res_len // 160) == (cases.SKIP_HEAD, cases.RETURN_LENGTH, cases.T)
    net.rows = slice(0, n)
    if shifts is not None:
        for s in range(n):
            bank.set_formant(s, shifts[s])
    x = (0.3 * np.random.default_rng(n).standard_normal((4, n, bank.block_frame))).astype(np.float32)
    for j in range(2):
        bank.process(x[j])
    if clear:
        for s in range(n):
            bank.set_formant(s, 0.0)
        bank.process(x[2])
        return bank, lambda: bank.process(x[3])
    return bank, lambda: bank.process(x[2])


def test_bank_launch_count_with_formant_shifts(vc_setup, gpu):
    """One warm ``RealtimeBank.process`` around a real ``RealtimeVCBatch`` (no feeders), counted by torch.profiler.  What a shift adds to the
    block -- the two per-item interpolations (excitation, x) and the ragged resample, three launches, nothing dropped -- is the same at
    S = 1 and S = 3 and for one or three distinct shifts; the whole block issues the same number of launches at S = 2 and S = 3; a bank that
    never heard of formants and one whose shifts were set and cleared issue exactly the same launches.

    The whole-block count at S = 1 is NOT the count at S = 3, with or without this feature: measured on an MI355X, 107 against 109 launches
    unshifted and 110 against 112 shifted without an index (115 against 119 with one: the IVF search picks another kernel set for one
    session's 16 rows).  Every [1, n] slice of a rolling buffer is contiguous, so at S = 1 torch skips two copies that a strided [S, n]
    slice needs.  That is the existing bank's behaviour, so S = 1 enters through the difference shifted - unshifted, which is what this
    feature launches.  The generator's ResBlock family is pinned for the count (its own choice follows the number of rows, i.e. S)."""
    net, index = vc_setup
    for k, v in (("RB_STREAM", 0), ("NO_RB_SPLIT", 1)):
        net.dec.set_option(k, v)
    try:
        _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)   # (the profiler's own start-up)
        shifted, plain = {}, {}
        for n in (1, 2, 3):
            bank, step = _warm_bank(net, index, gpu, n, fc.FORMANTS[:n] if n > 1 else [2.0])
            shifted[n] = _launches(step, gpu)
            assert bank.rvc.seen == [bank.formants] * 3 and bank.rvc.vc._resample.rebuilds == 1    # nothing rebuilt or uploaded per block
            plain_bank, step = _warm_bank(net, index, gpu, n, None)
            plain[n] = _launches(step, gpu)
            assert plain_bank.rvc.seen == [None] * 3
            print("S %d: %d launches unshifted, %d shifted" % (n, len(plain[n]), len(shifted[n])))
            # the shift costs the two per-item interpolations and the ragged resample, nothing else comes or goes
            assert len(plain[n]) > 12 and len(shifted[n]) == len(plain[n]) + 3, _diff(shifted[n], plain[n])
            assert sum("k_interp_linear_ragged" in k for k in shifted[n]) == 2 and sum("k_resample_poly_ragged" in k for k in shifted[n]) == 1
            assert not any("ragged" in k for k in plain[n])
        assert len(shifted[2]) == len(shifted[3]), _diff(shifted[2], shifted[3])
        same = _launches(_warm_bank(net, index, gpu, S, [2.0, 2.0, 2.0])[1], gpu)
        assert len(same) == len(shifted[3]), _diff(same, shifted[3])
        cleared_bank, cleared_step = _warm_bank(net, index, gpu, S, fc.FORMANTS, clear=True)
        cleared = _launches(cleared_step, gpu)
        assert cleared_bank.rvc.seen == [fc.FORMANTS] * 2 + [None] * 2
        assert plain[3] == cleared, _diff(plain[3], cleared)
    finally:
        for k in ("RB_STREAM", "NO_RB_SPLIT"):
            net.dec.set_option(k, None)
        net.rows = slice(0, S)


def test_bank_set_formant_survives_reset_and_equals_the_vc_batch(vc_setup, gpu):
    """``set_formant`` between blocks changes the next block only for that session's row; ``reset(i)`` leaves the shift as it leaves the key."""
    net, index = vc_setup
    bank, _ = _warm_bank(net, index, gpu, S, None)
    x = np.zeros((S, bank.block_frame), np.float32)
    bank.set_formant(2, -1.35)
    bank.process(x)
    assert bank.formants == [0.0, 0.0, -1.35] and bank.rvc.seen[-1] == [0.0, 0.0, -1.35]
    bank.reset(2)
    assert bank.formants == [0.0, 0.0, -1.35] and bank.keys[2] == bank.keys[0]
    bank.set_formant(2, 0)
    bank.process(x)
    assert bank.rvc.seen[-1] is None
    net.rows = slice(0, S)


# ---- 5. what stays refused ---------------------------------------------------------------------------------------------------------------

def test_bank_wide_formant_shifts_stay_refused(gpu):
    import rvc_amd

    net = type("N", (), {})()
    with pytest.raises(ValueError, match="formant"):
        rvc_amd.RealtimeVCBatch(net, S, device=gpu, formant_shift=1.0)
    with pytest.raises(ValueError, match="formant"):
        rvc_amd.RealtimeVCBatch(net, S, device=gpu).set_formant(-2)
    stub = type("R", (), {"tgt_sr": 40000})()
    bank = rvc_amd.RealtimeBank(stub, sessions=S, samplerate=40000, block_time=0.1, extra_time=0.5, device=gpu)
    with pytest.raises(IndexError):
        bank.set_formant(S, 1.0)
    with pytest.raises(IndexError):
        bank.set_formant(-1, 1.0)
    with pytest.raises(IndexError):
        rvc_amd.RealtimeVCBatch(net, S, device=gpu).set_session_formant(S, 1.0)
    bank.set_formant(S - 1, 1.0)
    assert bank.formants == [0.0, 0.0, 1.0]
    stub.formant_shift, stub.net_g, stub.index_rate, stub.if_f0 = 1.0, net, 0.0, 1
    with pytest.raises(ValueError, match="formant"):
        bank.process(np.zeros((S, bank.block_frame), np.float32))
    with pytest.raises(ValueError):
        rvc_amd.infer_hip(None, None, torch.zeros(S, 4, 8), None, None, return_length2=[4, 4, 4])             # no skip_head / return_length
    with pytest.raises(ValueError):
        rvc_amd.infer_hip(None, None, torch.zeros(S, 4, 8), None, None, skip_head=0, return_length=4, return_length2=[4, 4])
    torch.cuda.synchronize(gpu)
