"""The realtime bank: S live streams of one voice in one pass per block.

1. the batched block DSP (``rvcmi_glue_*_batch``) is bit-equal, per session, to the single-stream entry points on rows that are slices
   of longer buffers; 2. the realtime guard of the batched retrieval is per session; 3. ``RealtimeVCBatch`` against the existing
   ``net_g.infer`` / ``RealtimeVC.infer``; 4. ``RealtimeBank`` over the committed GUI fixtures against solo ``RealtimeStream`` runs;
   5. ``rvc_infer_batch_hip`` end to end with stub feeders; 6. what is refused."""
import ctypes as C

import numpy as np
import pytest
import torch

import rt_bank_cases as cases
from conftest import load_golden
from oracle import ivf_oracle

S = 3


def _fades(n):
    fade_in = torch.sin(0.5 * np.pi * torch.linspace(0.0, 1.0, steps=n, dtype=torch.float32)) ** 2  # gui.py:841-855
    return fade_in, 1 - fade_in


def _rows(t, pad_l, pad_r, gpu):
    """``t`` [S, n] as row slices of a longer device buffer: the row stride is not the row length, the rows start off the base."""
    big = torch.full((t.shape[0], pad_l + t.shape[1] + pad_r), 7.0, device=gpu, dtype=torch.float32)
    view = big[:, pad_l: pad_l + t.shape[1]]
    view.copy_(t)
    assert view.stride(0) != view.shape[1] and not view.is_contiguous()
    return view


# ---- 1. batched kernels against the single-stream ones --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("use_pv", [False, True])
@pytest.mark.parametrize("blk,Lb,Ls,zero", [(240, 64, 40, False), (100, 33, 10, False), (240, 64, 40, True), (100, 33, 10, True)])
def test_sola_batch_is_bit_equal_to_sola_per_session(blk, Lb, Ls, zero, use_pv, gpu):
    """Planted offsets 0, Ls // 2 and Ls over the three sessions; ``zero``: all-zero chunks (nothing planted: every correlation is
    0 / sqrt(1e-8), the first offset wins).  Outputs, updated tails and offsets with torch.equal; the odd Lb is the odd bin count of the pv."""
    import rvc_amd

    n = Ls + blk + Lb + 5
    offs = [0, Ls // 2, Ls]
    gen = torch.Generator().manual_seed(blk + Lb)
    t = torch.arange(n, dtype=torch.float32)
    wav = torch.stack([0.4 * torch.sin(2 * np.pi * (0.011 + 0.003 * s) * t) + 0.2 * torch.sin(2 * np.pi * 0.0373 * t) + 0.05 * torch.randn(n, generator=gen)
                       for s in range(S)])
    buf = torch.stack([wav[s, offs[s]: offs[s] + Lb] * 0.9 + 0.01 * torch.randn(Lb, generator=gen) for s in range(S)])
    if zero:
        wav = torch.zeros_like(wav)
    fi, fo = (w.to(gpu) for w in _fades(Lb))
    wav_v, buf_v = _rows(wav, 5, 32, gpu), _rows(buf, 3, 8, gpu)
    ref = []
    for s in range(S):
        b = buf[s].to(gpu).clone()
        o, off = rvc_amd.glue.sola(wav[s].to(gpu).contiguous(), b, fi, fo, blk, Ls, return_offset=True, use_pv=use_pv)
        ref.append((o, b, off))
    out, offsets = rvc_amd.glue.sola_batch(wav_v, buf_v, fi, fo, blk, Ls, use_pv=use_pv)
    assert out.shape == (S, blk) and offsets.shape == (S,) and offsets.dtype == torch.int32
    for s in range(S):
        assert int(offsets[s]) == int(ref[s][2]) == (0 if zero else offs[s]), (s, int(offsets[s]), int(ref[s][2]))
        assert torch.equal(out[s], ref[s][0]), "session %d: output block" % s
        assert torch.equal(buf_v[s], ref[s][1]), "session %d: updated sola_buffer" % s
    assert bool((buf_v._base[:, :3] == 7.0).all()) and bool((buf_v._base[:, 3 + Lb:] == 7.0).all())  # nothing written outside the rows


@pytest.mark.gpu
@pytest.mark.parametrize("orig,new,n", [(48000, 16000, 1001), (40000, 48000, 1003)])
def test_resample_batch_is_bit_equal_to_the_row_loop(orig, new, n, gpu):
    """``n`` is no multiple of the reduced input rate: the taps of the last output samples hang over the end of the row (zeros there,
    NOT the neighbour's samples or the 7.0 behind the slice)."""
    import rvc_amd

    rs = rvc_amd.SincResample(orig, new, gpu)
    x = torch.from_numpy((0.3 * np.random.default_rng(n).standard_normal((S, n))).astype(np.float32))
    view = _rows(x, 9, 40, gpu)
    got = rs.batch(view)
    ref = rs(x.to(gpu))
    assert got.shape == ref.shape == (S, -(-rs.new * n // rs.orig))
    assert torch.equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("zc", [160, 441])
def test_envelope_mix_batch_is_bit_equal_to_envelope_mix_per_session(zc, rate, gpu):
    import rvc_amd

    n = 7 * zc + 13
    rng = np.random.default_rng(zc)
    inp = (0.3 * rng.standard_normal((S, n + 3 * zc))).astype(np.float32)
    wav = (0.2 * rng.standard_normal((S, n))).astype(np.float32)
    wav[1, 2 * zc: 4 * zc] = 0.0      # the 1e-3 floor of rms2
    inp[2, zc: 3 * zc] = 0.0          # rms1 = 0
    inp_v, wav_v = _rows(torch.from_numpy(inp), 17, 0, gpu), _rows(torch.from_numpy(wav), 2, 6, gpu)
    ref = [rvc_amd.glue.envelope_mix(torch.from_numpy(inp[s]).to(gpu), torch.from_numpy(wav[s]).to(gpu), zc, rate) for s in range(S)]
    got = rvc_amd.glue.envelope_mix_batch(inp_v, wav_v, zc, rate)
    assert got.data_ptr() == wav_v.data_ptr()
    for s in range(S):
        assert torch.equal(got[s], ref[s]), "session %d" % s
    assert bool((wav_v._base[:, :2] == 7.0).all()) and bool((wav_v._base[:, 2 + n:] == 7.0).all())


# ---- 2. the guard is per session ---------------------------------------------------------------------------------------------------

def test_guard_case_on_the_cpu_oracle():
    """Before anything goes to the GPU: the oracle alone returns a negative id for session 1's searched rows and for no other row; with
    every list long, for none."""
    for short in (True, False):
        idx, cent = cases.guard_index(short)
        sizes = np.diff(idx["list_offsets"])
        assert (int(sizes.min()) == 3 and int((sizes < 8).sum()) == 1) if short else int(sizes.min()) >= 8
        feats, _ = cases.guard_feats(cent)
        for s in range(cases.GUARD_S):
            _, ids = ivf_oracle.search(idx, feats[s, cases.GUARD_SKIP:].numpy(), 8)
            assert bool((ids < 0).any()) == (short and s == 1), (short, s)


@pytest.mark.gpu
@pytest.mark.parametrize("short", [True, False])
def test_realtime_guard_is_per_session(short, gpu):
    import rvc_amd

    idx, cent = cases.guard_index(short)
    feats, pitchf = cases.guard_feats(cent)
    hip = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=gpu)
    f, pf = feats.to(gpu), pitchf.to(gpu)
    kw = dict(protect=0.33, p_len=cases.GUARD_PLEN, realtime_guard=True, skip_rows=cases.GUARD_SKIP)
    got = rvc_amd.glue.retrieve_blend_expand_batch(f, hip, 0.75, pf, **kw)
    assert got.shape == (cases.GUARD_S, cases.GUARD_PLEN, 256)
    for s in range(cases.GUARD_S):
        solo = rvc_amd.glue.retrieve_blend_expand(f[s:s + 1], hip, 0.75, pf[s:s + 1], **kw)[0]
        plain = rvc_amd.glue.retrieve_blend_expand(f[s:s + 1], None, 0.0, pf[s:s + 1], 0.33, cases.GUARD_PLEN)[0]
        if short and s == 1:
            assert torch.equal(got[s], plain), "the session that probes the 3-vector list must come out un-blended"
        else:
            assert torch.equal(got[s], solo), "session %d differs from its own guarded single-session call" % s
            assert not torch.equal(got[s], plain), "session %d was not blended" % s
        assert torch.equal(got[s, : 2 * cases.GUARD_SKIP], plain[: 2 * cases.GUARD_SKIP])   # the old frames keep their features
    # without an index: the expansion and the protect mix alone, one launch for the bank
    none = rvc_amd.glue.retrieve_blend_expand_batch(f, None, 0.0, pf, 0.33, cases.GUARD_PLEN)
    for s in range(cases.GUARD_S):
        assert torch.equal(none[s], rvc_amd.glue.retrieve_blend_expand(f[s:s + 1], None, 0.0, pf[s:s + 1], 0.33, cases.GUARD_PLEN)[0])


# ---- 3. RealtimeVCBatch ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def vc_setup(gpu):
    import rvc_amd

    idx = cases.index_768()
    index = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=gpu)
    return cases.BankNet(gpu, S), index


@pytest.mark.gpu
def test_realtime_vc_batch_against_the_existing_infer(vc_setup, gpu):
    """Two consecutive blocks (the cache roll), three sessions, two speakers.  (a) row i == row i of a direct ``net_g.infer`` at batch 3 on
    the operands the existing single-stream helpers prepare: isolates the new code, bit for bit.  (b) row i against the solo
    ``RealtimeVC.infer`` of session i under the recorded distance of the existing batch-3 ``infer`` from batch 1 on these inputs
    (profiles/rt_bank_parity.json, tools/rt_bank_parity.py): zero there means bit equality here."""
    import rvc_amd

    net, index = vc_setup
    blocks = cases.vc_blocks(S, 2)
    ops = cases.solo_operands(net, index, gpu, blocks)
    bank = rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000)
    solos = [rvc_amd.RealtimeVC(net, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000) for _ in range(S)]
    bar = cases.recorded_bar()
    for b, (feats, pitch, pitchf) in enumerate(blocks):
        net.rows = slice(0, S)
        got = bank.infer(feats.to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, pitch=pitch.to(gpu),
                         pitchf=pitchf.to(gpu), protect=cases.PROTECT, sid=cases.SIDS)
        assert got.shape == (S, cases.RETURN_LENGTH * net.upp) and bool(torch.isfinite(got).all())
        ref = cases.direct_batch(net, ops[b], gpu)
        assert torch.equal(got, ref), "block %d: max abs %.3e from the direct batch-3 infer" % (b, float((got - ref).abs().max()))
        for s in range(S):
            net.rows = slice(s, s + 1)
            solo = solos[s].infer(feats[s:s + 1].to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, pitch=pitch[s].to(gpu),
                                  pitchf=pitchf[s].to(gpu), protect=cases.PROTECT, sid=cases.SIDS[s])
            e = got[s].double() - solo.double()
            print("block %d session %d: max abs %.3e rms %.3e (bar %s)" % (b, s, float(e.abs().max()), float(e.pow(2).mean().sqrt()), bar))
            assert cases.within_bar(got[s], solo, bar), "block %d session %d: max abs %.3e rms %.3e, bar %s" % (
                b, s, float(e.abs().max()), float(e.pow(2).mean().sqrt()), bar)
    assert not torch.equal(got[0], got[1]) and not torch.equal(got[1], got[2])
    # the caches rolled like the solo ones
    for s in range(S):
        assert torch.equal(bank.pitch[s], solos[s].cache.pitch) and torch.equal(bank.pitchf[s], solos[s].cache.pitchf)


# ---- 4. RealtimeBank over the GUI fixtures -------------------------------------------------------------------------------------------

class _SoloStub:
    """``rtrvc.RVC``-like for one ``RealtimeStream``: returns the fixture's chunks in the session's (cyclically shifted) order."""

    def __init__(self, d, dev, order):
        self.d, self.dev, self.order, self.j = d, dev, list(order), 0
        self.tgt_sr = int(d["tgt_sr"])

    def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
        j = self.order[self.j]
        self.j += 1
        return torch.from_numpy(self.d["chunks"][j]).to(self.dev)


class _BankStub:
    """The same for the bank: ``infer_batch`` returns [S, .], session s's chunk shifted by s; records what it was handed."""

    def __init__(self, d, dev):
        self.d, self.dev, self.j, self.seen = d, dev, 0, []
        self.tgt_sr = int(d["tgt_sr"])

    def infer_batch(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method, keys, sids):
        d, K = self.d, self.d["chunks"].shape[0]
        assert (block_frame_16k, skip_head, return_length) == (int(d["block_frame_16k"]), int(d["skip_head"]), int(d["return_length"]))
        assert input_wav_res.is_cuda and input_wav_res.shape == (S,) + d["input_wav_res"][0].shape and len(keys) == len(sids) == S
        self.seen.append(input_wav_res.clone())
        out = torch.from_numpy(np.stack([d["chunks"][(self.j + s) % K] for s in range(S)])).to(self.dev)
        self.j += 1
        return out


def _mono(x):
    x = np.asarray(x, dtype=np.float32)
    return np.mean(x.T, axis=0) if x.ndim == 2 else x    # librosa.to_mono(indata.T), as RealtimeStream.process does


def _stream_kw(d, gpu):
    return dict(samplerate=int(d["samplerate"]), block_time=float(d["block_time"]), crossfade_time=float(d["crossfade_time"]),
                extra_time=float(d["extra_time"]), threhold=float(d["threhold"]), rms_mix_rate=float(d["rms_mix_rate"]), use_pv=bool(d["use_pv"]),
                device=gpu)


def _rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pv40k", "mix48k", "pv44k"])
def test_realtime_bank_matches_solo_streams_and_the_fixture(case, gpu):
    """Session s is fed the fixture's blocks cyclically shifted by s.  Every session's blocks and offsets are bit-equal to a solo
    ``RealtimeStream`` on the same data (so is the 16 kHz window handed to the model); session 0 also meets the fixture's bars."""
    import rvc_amd

    d = load_golden("gui_stream_" + case)
    K = d["indata"].shape[0]
    kw = _stream_kw(d, gpu)
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **kw)
    solos = [rvc_amd.RealtimeStream(_SoloStub(d, gpu, [(j + s) % K for j in range(K)]), **kw) for s in range(S)]
    for j in range(K):
        out = bank.process(np.stack([_mono(d["indata"][(j + s) % K]) for s in range(S)]))
        assert out.is_cuda and out.shape == (S, d["out"][j].shape[0]) and bank.last_offsets.shape == (S,)
        for s in range(S):
            ref = solos[s].process(d["indata"][(j + s) % K])
            assert torch.equal(out[s], ref), "block %d session %d: max abs %.3e" % (j, s, float((out[s] - ref).abs().max()))
            assert int(bank.last_offsets[s]) == int(solos[s].last_offset), (j, s)
            assert torch.equal(bank.rvc.seen[j][s], solos[s].input_wav_res)
            assert torch.equal(bank.sola_buffer[s], solos[s].sola_buffer)
        assert int(bank.last_offsets[0]) == int(d["offsets"][j]), j
        err = out[0].cpu().numpy().astype(np.float64) - d["out"][j]
        bar_max, bar_rms = (2e-5, 2.5e-6) if bool(d["use_pv"]) else (1e-6, 1e-7)
        assert np.abs(err).max() <= bar_max and _rms(err) <= bar_rms, "block %d: max %.2e rms %.2e" % (j, np.abs(err).max(), _rms(err))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["pv40k", "mix48k", "pv44k"])
def test_realtime_bank_reset_touches_one_session(case, gpu):
    """``reset(1)`` after two blocks: sessions 0 and 2 go on as their solo streams do, session 1 equals a FRESH solo stream."""
    import rvc_amd

    d = load_golden("gui_stream_" + case)
    K = d["indata"].shape[0]
    kw = _stream_kw(d, gpu)
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **kw)
    order = lambda s: [(j + s) % K for j in range(K)]  # noqa: E731
    solos = [rvc_amd.RealtimeStream(_SoloStub(d, gpu, order(s)), **kw) for s in range(S)]
    for j in range(K):
        if j == 2:
            bank.reset(1)
            solos[1] = rvc_amd.RealtimeStream(_SoloStub(d, gpu, order(1)[2:]), **kw)
        out = bank.process(np.stack([_mono(d["indata"][(j + s) % K]) for s in range(S)]))
        for s in range(S):
            ref = solos[s].process(d["indata"][(j + s) % K])
            assert torch.equal(out[s], ref), "block %d session %d" % (j, s)
            assert int(bank.last_offsets[s]) == int(solos[s].last_offset), (j, s)


# ---- 5. rvc_infer_batch_hip end to end -----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_rvc_infer_batch_hip_against_solo_rvc_infer_hip(vc_setup, gpu):
    """Stub feeders whose rows are batch-invariant by construction (framing + element-wise operations), two sessions with different keys,
    two blocks.  HuBERT and the f0 network run ONCE per block on the [2, .] batch; each session equals its solo ``rvc_infer_hip`` under
    bar (b) of test 3: the recorded distance of the EXISTING ``net_g.infer`` at this batch size from batch 1 on these operands
    (``batch2_vs_batch1_end_to_end_operands`` of profiles/rt_bank_parity.json, measured by tools/rt_bank_parity.py on the operands the solo
    ``rvc_infer_hip`` prepares, without any code of the bank): 1.663e-3 max-abs, 2.988e-4 RMS on an MI355X.  The figure recorded for test 3's
    own inputs at batch 3 (1.526e-3 / 3.096e-4) is a property of THOSE inputs: these differ from their solo run by 1.474e-3, 1.393e-3,
    1.264e-3 and 1.663e-3 max-abs, all of it the batched ``infer``'s own distance.  protect = 1.0: the estimator's 31 frames are not
    p_len = 70 (rtrvc.py:229)."""
    from rvc_amd.realtime import rvc_infer_batch_hip, rvc_infer_hip

    net, index = vc_setup
    keys = cases.E2E_KEYS
    both = cases.stub_rvc(net, index, gpu, 0)
    solos = [cases.stub_rvc(net, index, gpu, keys[s]) for s in range(2)]
    bar = cases.recorded_bar("batch2_vs_batch1_end_to_end_operands")
    for b, wav in enumerate(cases.e2e_waves(2, 2)):
        w = wav.to(gpu)
        net.rows = slice(0, 2)
        got = rvc_infer_batch_hip(both, w, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0, keys=keys, sids=[0, 0])
        assert got.shape == (2, cases.RETURN_LENGTH * net.upp) and bool(torch.isfinite(got).all())
        for s in range(2):
            net.rows = slice(s, s + 1)
            ref = rvc_infer_hip(solos[s], w[s], cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0)
            e = got[s].double() - ref.double()
            print("block %d session %d: max abs %.3e rms %.3e (bar %s)" % (b, s, float(e.abs().max()), float(e.pow(2).mean().sqrt()), bar))
            assert cases.within_bar(got[s], ref, bar), "block %d session %d: max abs %.3e rms %.3e, bar %s" % (
                b, s, float(e.abs().max()), float(e.pow(2).mean().sqrt()), bar)
            # the pitch caches hold each session's own key
            assert torch.equal(both._rvcmi_rt_bank.pitch[s], solos[s]._rvcmi_rt.cache.pitch)
            assert torch.equal(both._rvcmi_rt_bank.pitchf[s], solos[s]._rvcmi_rt.cache.pitchf)
    assert both.hubert.batches == [2, 2] and both.f0_gen.rmvpe.batches == [2, 2]   # one feeder call per block, whatever S
    assert not torch.equal(both._rvcmi_rt_bank.pitch[0], both._rvcmi_rt_bank.pitch[1]) and float(both._rvcmi_rt_bank.pitchf.max()) > 0
    with pytest.raises(TypeError):
        rvc_infer_batch_hip(both, w, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, (None, None))
    both.index = object()
    with pytest.raises(TypeError):
        rvc_infer_batch_hip(both, w, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe")


# ---- 6. rejections: errors, never a fault ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_bank_rejects_bad_arguments(gpu):
    import rvc_amd
    from rvc_amd import _lib

    L = _lib.lib()
    st = _lib.stream_ptr(gpu)
    x = torch.zeros(S, 400, device=gpu)
    buf = torch.zeros(S, 64, device=gpu)
    fi, fo = (w.to(gpu) for w in _fades(64))
    out = torch.zeros(S, 240, device=gpu)
    off = torch.zeros(S, dtype=torch.int32, device=gpu)
    scratch = torch.zeros(S * 200, dtype=torch.float64, device=gpu)
    p = _lib.ptr
    # S = 0 at the C ABI of every batched entry point
    assert L.rvcmi_glue_sola_batch(0, p(x), 400, 400, p(buf), 64, 64, 40, p(fi), p(fo), 240, p(out), 240, p(off), st) == _lib.ERR_INVALID
    assert L.rvcmi_glue_sola_pv_batch(0, p(x), 400, 400, p(buf), 64, 64, 40, p(fi), p(fo), 240, p(out), 240, p(off), p(scratch), st) == _lib.ERR_INVALID
    assert L.rvcmi_glue_resample_poly_batch(0, p(x), 400, 400, p(fi), 3, 1, 8, 2, p(out), 240, 134, st) == _lib.ERR_INVALID
    assert L.rvcmi_glue_envelope_mix_batch(0, p(x), 400, p(out), 240, 240, 40, C.c_double(0.0), p(scratch), st) == _lib.ERR_INVALID
    assert L.rvcmi_glue_expand_protect_batch(0, p(x), 4, 100, 2, None, C.c_float(1.0), 8, p(out), st) == _lib.ERR_INVALID
    # a row stride shorter than the row
    assert L.rvcmi_glue_sola_batch(S, p(x), 399, 400, p(buf), 64, 64, 40, p(fi), p(fo), 240, p(out), 240, p(off), st) == _lib.ERR_INVALID
    assert L.rvcmi_glue_sola_batch(S, p(x), 400, 400, p(buf), 63, 64, 40, p(fi), p(fo), 240, p(out), 240, p(off), st) == _lib.ERR_INVALID
    assert L.rvcmi_glue_sola_pv_batch(S, p(x), 400, 400, p(buf), 64, 64, 40, p(fi), p(fo), 240, p(out), 239, p(off), p(scratch), st) == _lib.ERR_INVALID
    assert L.rvcmi_glue_resample_poly_batch(S, p(x), 399, 400, p(fi), 3, 1, 8, 2, p(out), 240, 134, st) == _lib.ERR_INVALID
    assert L.rvcmi_glue_envelope_mix_batch(S, p(x), 400, p(out), 239, 240, 40, C.c_double(0.0), p(scratch), st) == _lib.ERR_INVALID
    # ... and through the Python layer: overlapping rows (an as_strided view), no session at all
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.glue.sola_batch(x.as_strided((S, 400), (100, 1)), buf, fi, fo, 240, 40)
    with pytest.raises(ValueError):
        rvc_amd.glue.sola_batch(x[:0], buf[:0], fi, fo, 240, 40)
    with pytest.raises(ValueError):
        rvc_amd.glue.retrieve_blend_expand_batch(torch.zeros(0, 4, 8, device=gpu), None, 0.0)
    # the LDS limit (2 Lb + Ls floats <= 150 KB) and the phase vocoder's size limit are kept
    big = torch.zeros(1, 60000, device=gpu)
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.glue.sola_batch(big, torch.zeros(1, 19000, device=gpu), torch.zeros(19000, device=gpu), torch.zeros(19000, device=gpu), 100, 1000)
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.glue.sola_batch(big, torch.zeros(1, 4097, device=gpu), torch.zeros(4097, device=gpu), torch.zeros(4097, device=gpu), 100, 10, use_pv=True)
    # the objects
    net = type("N", (), {})()
    with pytest.raises(ValueError):
        rvc_amd.RealtimeVCBatch(net, 0, device=gpu)
    with pytest.raises(ValueError, match="formant"):
        rvc_amd.RealtimeVCBatch(net, S, device=gpu, formant_shift=1.0)
    with pytest.raises(ValueError, match="formant"):
        rvc_amd.RealtimeVCBatch(net, S, device=gpu).set_formant(-2)
    stub = type("R", (), {"tgt_sr": 40000})()
    for bad in (dict(I_noise_reduce=True), dict(O_noise_reduce=True), dict(function="im"), dict(sessions=0)):
        with pytest.raises(ValueError):
            rvc_amd.RealtimeBank(stub, **{"sessions": S, "samplerate": 40000, "device": gpu, **bad})
    bank = rvc_amd.RealtimeBank(stub, sessions=S, samplerate=40000, block_time=0.1, extra_time=0.5, device=gpu)
    for shape in ((S, bank.block_frame + 1), (S + 1, bank.block_frame), (bank.block_frame,), (S, bank.block_frame, 2)):
        with pytest.raises(ValueError):
            bank.process(np.zeros(shape, np.float32))
    stub.formant_shift, stub.net_g, stub.index_rate, stub.if_f0 = 1.0, net, 0.0, 1
    with pytest.raises(ValueError, match="formant"):
        bank.process(np.zeros((S, bank.block_frame), np.float32))
    torch.cuda.synchronize(gpu)
