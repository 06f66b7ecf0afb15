"""The realtime bank's remaining sliders per session: index_rate, protect, rms_mix_rate and threhold.

1. ``glue.envelope_mix_sessions``, 2. ``glue.input_gate_sessions`` and 3. ``glue.retrieve_blend_expand_sessions`` against the solo calls with
each session's own value, bit for bit, sessions that are off included; 4. the realtime guard stays per session when the searched rows are
compacted; 5. ``RealtimeVCBatch`` with a rate and a protect per session against the direct batch-S ``net_g.infer`` on solo-prepared operands;
6. ``RealtimeBank`` over the committed GUI fixtures against solo ``RealtimeStream`` runs whose attributes move at the same blocks; 7. the launch
counts; 8. what is refused.  No tolerance anywhere: every comparison is ``torch.equal`` (or on the int32 views where a -0.0 or a NaN matters)."""
import ctypes as C

import numpy as np
import pytest
import torch

import input_gate_cases as gc
import rt_bank_cases as cases
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _rows(t, pad_l, pad_r, gpu, fill=7.0):
    """``t`` [S, n] as row slices of a longer device buffer (row stride != row length)."""
    big = torch.full((t.shape[0], pad_l + t.shape[1] + pad_r), fill, device=gpu, dtype=torch.float32)
    view = big[:, pad_l: pad_l + t.shape[1]]
    view.copy_(t)
    assert view.stride(0) != view.shape[1]
    return view


def _bits(t):
    return t.contiguous().view(torch.int32)


def _hip_index(idx, gpu):
    import rvc_amd

    return rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=gpu)


# ---- 1. envelope mix ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("zc", [160, 441])
def test_envelope_mix_sessions(zc, gpu):
    import rvc_amd

    S, n, rates = 3, 5 * zc + 7, (0.0, 0.5, 1.0)
    rng = np.random.default_rng(zc)
    inp = (0.3 * rng.standard_normal((S, n + 2 * zc))).astype(np.float32)
    wav = (0.2 * rng.standard_normal((S, n))).astype(np.float32)
    wav[1, zc: 3 * zc] = 0.0                 # the 1e-3 floor of rms2
    wav[2, 5], wav[2, 9] = -0.0, np.nan      # the off session's row must come back bit for bit
    inp_v, wav_v = _rows(torch.from_numpy(inp), 17, 0, gpu), _rows(torch.from_numpy(wav), 2, 6, gpu)
    before = _bits(wav_v[2]).clone()
    ref = [rvc_amd.glue.envelope_mix(torch.from_numpy(inp[s, :n].copy()).to(gpu), torch.from_numpy(wav[s]).to(gpu), zc, rates[s]) for s in range(2)]
    got = rvc_amd.glue.envelope_mix_sessions(inp_v, wav_v, zc, rates)
    assert got.data_ptr() == wav_v.data_ptr()
    for s in range(2):
        assert torch.equal(got[s], ref[s]), "session %d" % s
        assert not torch.equal(got[s], torch.from_numpy(wav[s]).to(gpu))
    assert torch.equal(_bits(wav_v[2]), before), "the session at rate 1 was written"
    assert bool((wav_v._base[:, :2] == 7.0).all()) and bool((wav_v._base[:, 2 + n:] == 7.0).all())
    # every session off: nothing is written
    all_before = _bits(wav_v._base).clone()
    rvc_amd.glue.envelope_mix_sessions(inp_v, wav_v, zc, (1, 1, 1))
    assert torch.equal(_bits(wav_v._base), all_before)


# ---- 2. input gate --------------------------------------------------------------------------------------------------------------------

GATE_THREHOLDS = (-40.5, -20, -60, -55)


@pytest.mark.parametrize("zc,blk", gc.GEOMETRIES)
def test_input_gate_sessions(zc, blk, gpu):
    import rvc_amd
    from rvc_amd.realtime import input_gate

    S, thr = 4, GATE_THREHOLDS
    rng = np.random.default_rng(zc + blk)
    # per session three blocks of noise around ITS threshold, levels moving every 3 hops: the first and the last block centred 4 dB below it, the
    # middle one 4 dB above, so that frames fall on both sides (the off session: around -50 dB, which a bank-wide gate at -40.5 would close on)
    x = np.stack([np.stack([gc.stretches(rng, blk, zc, (t if t > -60 else -50.0) + (4.0 if j == 1 else -4.0), spread=2.0) for t in thr])
                  for j in range(3)])                                        # [3, S, blk]
    host_rms = [np.zeros(4 * zc, np.float32) for _ in range(S)]
    rms_dev = _rows(torch.zeros(S, 4 * zc), 3, 5, gpu)
    rms_dev[2] = 0.25                                                        # canaries in the off session's rms_buffer row
    zeroed, kept = [0] * S, [0] * S
    for j in range(3):
        dst = _rows(torch.full((S, blk + 2 * zc), 3.0), 11, 4, gpu)          # 3.0: the canaries in front of the off session's block
        rvc_amd.glue.input_gate_sessions(_rows(torch.from_numpy(x[j]), 1, 2, gpu), rms_dev, dst, zc, thr)
        for s in range(S):
            if thr[s] > -60:
                want = input_gate(x[j, s], host_rms[s], zc, thr[s])
                assert torch.equal(dst[s].cpu(), torch.from_numpy(want)), "block %d session %d" % (j, s)
                assert torch.equal(rms_dev[s].cpu(), torch.from_numpy(host_rms[s])), "block %d session %d: rms_buffer" % (j, s)
                zeroed[s] += int(((want[2 * zc:] == 0) & (x[j, s] != 0)).sum())   # samples of quiet frames (the gate zeroes zc at a time)
                kept[s] += int((want[2 * zc:] != 0).sum())                        # samples of frames that are not quiet
            else:
                assert torch.equal(dst[s, 2 * zc:].cpu(), torch.from_numpy(x[j, s])), "the off session's raw block"
                assert bool((dst[s, : 2 * zc] == 3.0).all()), "the 2 zc samples in front of an off session's block were touched"
                assert bool((rms_dev[s] == 0.25).all()), "an off session's rms_buffer row was touched"
        assert bool((dst._base[:, :11] == 7.0).all()) and bool((dst._base[:, 11 + blk + 2 * zc:] == 7.0).all())
    for s in range(S):   # from the host rule: every gated session had quiet and non-quiet hops, so nothing passes with nothing gated
        assert thr[s] <= -60 or (zeroed[s] >= zc // 2 and kept[s] >= zc // 2), (s, zeroed, kept)
    assert bool((rms_dev._base[:, :3] == 7.0).all()) and bool((rms_dev._base[:, 3 + 4 * zc:] == 7.0).all())


# ---- 3. retrieval ---------------------------------------------------------------------------------------------------------------------

NQ, SKIP, PLEN = 9, 4, 17
RATES, PROTECTS = (0.75, 0.0, 0.3), (0.33, 1.0, 0.49)


@pytest.fixture(scope="module", params=[256, 768])
def index_d(request, gpu):
    idx = cases.guard_index(short=False)[0] if request.param == 256 else cases.index_768()
    return _hip_index(idx, gpu), request.param


def _retrieval_inputs(d, gpu):
    from oracle import synth

    S = 3
    feats = torch.stack([synth.make_phone(1, NQ, d, 900 + s)[0] for s in range(S)]).contiguous()
    feats[1, 2, 5] = -0.0                    # an old frame of the rate-0 session
    feats[1, 6, 7] = -0.0                    # one of its new frames
    feats[0, 7, 3] = -0.0                    # a searched row of a session that blends
    f0 = synth.make_f0(1, 64)[0]
    pitchf = torch.stack([f0[20 + 6 * s: 20 + 6 * s + PLEN] for s in range(S)]).contiguous()
    pitchf[:, 3:6] = 0.0                     # voiced and unvoiced frames in every session
    assert bool((pitchf < 1).any()) and bool((pitchf >= 1).any())
    return feats.to(gpu), pitchf.to(gpu)


def _solo(f, index, rate, pf, protect, s):
    import rvc_amd

    return rvc_amd.glue.retrieve_blend_expand(f[s:s + 1], index, rate, pf[s], protect, PLEN, realtime_guard=True, skip_rows=SKIP)[0]


def test_retrieve_blend_expand_sessions(index_d, gpu):
    import rvc_amd

    index, d = index_d
    f, pf = _retrieval_inputs(d, gpu)
    for idx, rates in ((index, RATES), (None, RATES), (index, (0.0, 0.0, 0.0))):
        searched = idx is not None and any(r != 0 for r in rates)
        index.profile(True)
        index.profile_read()
        got = rvc_amd.glue.retrieve_blend_expand_sessions(f, idx, rates, pf, PROTECTS, PLEN, skip_rows=SKIP)
        stats = {st["name"]: st for st in index.profile_read()}
        index.profile(False)
        assert got.shape == (3, PLEN, d)
        for s in range(3):
            want = _solo(f, idx, rates[s], pf, PROTECTS[s], s)
            assert torch.equal(got[s], want), "session %d (index %s, rates %s)" % (s, idx is not None, rates)
            assert torch.equal(_bits(got[s]), _bits(want)), "session %d: a zero changed its sign" % s
        plain = rvc_amd.glue.retrieve_blend_expand(f[1:2], None, 0.0, None, 1.0, PLEN)[0]
        assert torch.equal(_bits(got[1]), _bits(plain)), "the session that neither blends nor protect-mixes is not the bits of its input rows"
        if searched:
            assert not torch.equal(got[0], _solo(f, None, 0.0, pf, PROTECTS[0], 0)), "session 0 was not blended"
            assert stats["ivf_blend_x2"]["flops"] == 2 * 2 * (NQ - SKIP) * 8 * d     # two of three sessions were searched
            assert len(stats) > 1
        elif idx is not None:
            assert set(stats) == {"ivf_blend_x2"} and stats["ivf_blend_x2"]["flops"] == 0, "a search was launched with no session active: %s" % sorted(stats)
        else:
            assert not stats
    for rates, active in (((0.0, 0.5, 0.0), 1), ((0.75, 0.5, 0.3), 3)):
        index.profile(True)
        index.profile_read()
        got = rvc_amd.glue.retrieve_blend_expand_sessions(f, index, rates, pf, PROTECTS, PLEN, skip_rows=SKIP)
        stats = {st["name"]: st for st in index.profile_read()}
        index.profile(False)
        assert stats["ivf_blend_x2"]["flops"] == 2 * active * (NQ - SKIP) * 8 * d and stats["ivf_blend_x2"]["launches"] == 1
        for s in range(3):
            assert torch.equal(_bits(got[s]), _bits(_solo(f, index, rates[s], pf, PROTECTS[s], s))), (rates, s)
    # the device copy of the values is uploaded when they change, not per call
    n0 = rvc_amd.glue.session_rows_uploads
    rvc_amd.glue.retrieve_blend_expand_sessions(f, index, RATES, pf, PROTECTS, PLEN, skip_rows=SKIP)
    rvc_amd.glue.retrieve_blend_expand_sessions(f, index, RATES, pf, PROTECTS, PLEN, skip_rows=SKIP)
    assert rvc_amd.glue.session_rows_uploads == n0


# ---- 4. the guard stays per session under compaction ------------------------------------------------------------------------------------

def test_guard_is_per_session_under_compaction(gpu):
    """Session 1 probes the 3-vector list.  (a) 1 and 2 active, 0 at rate 0: session 1 (packed slot 0) keeps its features, session 2 (slot 1)
    blends.  (b) session 1 at rate 0 beside two active ones: its short list changes nothing for either."""
    import rvc_amd

    idx, cent = cases.guard_index(short=True)
    feats, pitchf = cases.guard_feats(cent)
    hip = _hip_index(idx, gpu)
    f, pf = feats.to(gpu), pitchf.to(gpu)
    kw = dict(p_len=cases.GUARD_PLEN, realtime_guard=True, skip_rows=cases.GUARD_SKIP)
    solo = lambda s, index, rate: rvc_amd.glue.retrieve_blend_expand(f[s:s + 1], index, rate, pf[s], 0.33, **kw)[0]  # noqa: E731
    prots = [0.33] * 3
    got = rvc_amd.glue.retrieve_blend_expand_sessions(f, hip, (0.0, 0.75, 0.5), pf, prots, **kw)
    assert torch.equal(got[0], solo(0, None, 0.0))
    assert torch.equal(got[1], solo(1, hip, 0.75)) and torch.equal(got[1], solo(1, None, 0.0)), "the session on the short list must keep its features"
    assert torch.equal(got[2], solo(2, hip, 0.5)) and not torch.equal(got[2], solo(2, None, 0.0)), "the session beside it must blend"
    got = rvc_amd.glue.retrieve_blend_expand_sessions(f, hip, (0.75, 0.0, 0.5), pf, prots, **kw)
    assert torch.equal(got[0], solo(0, hip, 0.75)) and not torch.equal(got[0], solo(0, None, 0.0))
    assert torch.equal(got[1], solo(1, None, 0.0))
    assert torch.equal(got[2], solo(2, hip, 0.5)) and not torch.equal(got[2], solo(2, None, 0.0))


# ---- 5. RealtimeVCBatch -------------------------------------------------------------------------------------------------------------------

S_NET = 5   # the model serves the three-session tests and the five-session launch count


@pytest.fixture(scope="module")
def vc_setup(gpu):
    return cases.BankNet(gpu, S_NET), _hip_index(cases.index_768(), gpu)


class _Spy:
    """``net_g`` that records the ``phone`` it is handed."""

    def __init__(self, net):
        self.net, self.phone = net, None

    def infer(self, phone, *a, **k):
        self.phone = phone.clone()
        return self.net.infer(phone, *a, **k)


def test_realtime_vc_batch_with_a_rate_and_a_protect_per_session(vc_setup, gpu, monkeypatch):
    import rvc_amd

    net, index = vc_setup
    S = 3
    blocks = cases.vc_blocks(S, 2)
    rates = [list(RATES), [0.75, 0.5, 0.3]]            # session 1 moves from 0 to 0.5 between the blocks
    seen = {}

    class Rec:
        def infer(self, phone, lengths, sid, pitch=None, pitchf=None, skip_head=None, return_length=None, return_length2=None):
            seen.update(phone=phone.clone(), pitch=pitch.clone(), pitchf=pitchf.clone())
            return torch.zeros(1, 1, 8, device=phone.device)

    solos = [rvc_amd.RealtimeVC(Rec(), index=index, index_rate=rates[0][s], device=gpu, tgt_sr=48000) for s in range(S)]
    spy = _Spy(net)
    bank = rvc_amd.RealtimeVCBatch(spy, S, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000)
    calls = {"batch": 0, "sessions": 0}
    real_batch, real_sessions = rvc_amd.glue.retrieve_blend_expand_batch, rvc_amd.glue.retrieve_blend_expand_sessions
    monkeypatch.setattr(rvc_amd.glue, "retrieve_blend_expand_batch", lambda *a, **k: (calls.__setitem__("batch", calls["batch"] + 1), real_batch(*a, **k))[1])
    monkeypatch.setattr(rvc_amd.glue, "retrieve_blend_expand_sessions",
                        lambda *a, **k: (calls.__setitem__("sessions", calls["sessions"] + 1), real_sessions(*a, **k))[1])
    for s in range(S):
        bank.set_session_protect(s, PROTECTS[s])
    for b, (feats, pitch, pitchf) in enumerate(blocks):
        ops = []
        for s in range(S):
            solos[s].set_index_rate(rates[b][s])
            bank.set_session_index_rate(s, rates[b][s])
            solos[s].infer(feats[s:s + 1].to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, pitch=pitch[s].to(gpu),
                           pitchf=pitchf[s].to(gpu), protect=PROTECTS[s], sid=cases.SIDS[s])
            ops.append(dict(seen))
        net.rows = slice(0, S)
        got = bank.infer(feats.to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, pitch=pitch.to(gpu), pitchf=pitchf.to(gpu),
                         protect=cases.PROTECT, sid=cases.SIDS)
        f1 = torch.cat((feats, feats[:, -1:, :]), 1).to(gpu)
        for s in range(S):
            assert torch.equal(spy.phone[s], ops[s]["phone"][0]), "block %d session %d: phone" % (b, s)
            use = rates[b][s] > 0
            want = rvc_amd.glue.retrieve_blend_expand(f1[s:s + 1], index if use else None, rates[b][s] if use else 0.0,
                                                      pitchf[s].to(gpu) if PROTECTS[s] < 0.5 else None, PROTECTS[s], cases.T, realtime_guard=True,
                                                      skip_rows=cases.SKIP_HEAD // 2)[0]
            assert torch.equal(spy.phone[s], want), "block %d session %d: phone against the solo glue call" % (b, s)
        ref = cases.direct_batch(net, ops, gpu)
        assert torch.equal(got, ref), "block %d: max abs %.3e from the direct batch-%d infer" % (b, float((got - ref).abs().max()), S)
    assert calls == {"batch": 0, "sessions": 2}
    assert not torch.equal(spy.phone[1], f1[1].repeat_interleave(2, 0)[: cases.T])   # session 1 blends in the second block
    # no session value set: today's call
    plain = rvc_amd.RealtimeVCBatch(spy, S, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000)
    feats, pitch, pitchf = blocks[0]
    plain.infer(feats.to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, pitch=pitch.to(gpu), pitchf=pitchf.to(gpu),
                protect=cases.PROTECT, sid=cases.SIDS)
    plain.set_session_index_rate(1, cases.INDEX_RATE)   # explicitly the bank-wide value: still today's call
    plain.infer(feats.to(gpu), cases.N_INPUT, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, pitch=pitch.to(gpu), pitchf=pitchf.to(gpu),
                protect=cases.PROTECT, sid=cases.SIDS)
    assert calls == {"batch": 2, "sessions": 2}


# ---- 6. RealtimeBank against solo streams -----------------------------------------------------------------------------------------------

S = 3


class _SoloStub:
    def __init__(self, d, dev, order):
        self.d, self.dev, self.order, self.j = d, dev, list(order), 0
        self.tgt_sr = int(d["tgt_sr"])

    def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
        j = self.order[self.j]
        self.j += 1
        return torch.from_numpy(self.d["chunks"][j]).to(self.dev)


class _BankStub:
    def __init__(self, d, dev):
        self.d, self.dev, self.j, self.seen = d, dev, 0, []
        self.tgt_sr = int(d["tgt_sr"])

    def infer_batch(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method, keys, sids):
        K = self.d["chunks"].shape[0]
        self.seen.append(input_wav_res.clone())
        out = torch.from_numpy(np.stack([self.d["chunks"][(self.j + s) % K] for s in range(S)])).to(self.dev)
        self.j += 1
        return out


def _mono(x):
    x = np.asarray(x, dtype=np.float32)
    return np.mean(x.T, axis=0) if x.ndim == 2 else x


@pytest.mark.parametrize("device_gate", [True, False])
@pytest.mark.parametrize("case", ["pv40k", "mix48k", "pv44k"])
def test_realtime_bank_sliders_match_solo_streams(case, device_gate, gpu):
    import rvc_amd
    from rvc_amd.realtime import input_gate

    d = load_golden("gui_stream_" + case)
    K, blocks = d["indata"].shape[0], 8
    assert K == 4
    kw = dict(samplerate=int(d["samplerate"]), block_time=float(d["block_time"]), crossfade_time=float(d["crossfade_time"]),
              extra_time=float(d["extra_time"]), threhold=float(d["threhold"]), rms_mix_rate=float(d["rms_mix_rate"]), use_pv=bool(d["use_pv"]),
              device=gpu, device_gate=device_gate)
    loud = -14 if case == "mix48k" else -12
    thr, mix = [-40, -60, loud], [0.25, 1.0, 0.0]
    updates = {2: ("threhold", 1, -40), 5: ("threhold", 1, -60), 3: ("rms_mix_rate", 2, 1.0), 6: ("rms_mix_rate", 2, 0.5)}
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **kw)
    solos = [rvc_amd.RealtimeStream(_SoloStub(d, gpu, [(j + s) % K for j in range(blocks)]), **kw) for s in range(S)]
    for s in range(S):
        bank.set_threhold(s, thr[s])
        bank.set_rms_mix_rate(s, mix[s])
        solos[s].threhold, solos[s].rms_mix_rate = thr[s], mix[s]
    host_rms = [np.zeros(4 * bank.zc, np.float32) for _ in range(S)]
    zeroed, kept, gated_blocks = [0] * S, [0] * S, [0] * S
    for j in range(blocks):
        if j in updates:
            what, s, v = updates[j]
            (bank.set_threhold if what == "threhold" else bank.set_rms_mix_rate)(s, v)
            setattr(solos[s], what, v)
        x = np.stack([_mono(d["indata"][(j + s) % K]) for s in range(S)])
        for s in range(S):   # the host rule, for the claim that the thresholds gate something and not everything
            if solos[s].threhold > -60:
                g = input_gate(x[s].copy(), host_rms[s], bank.zc, solos[s].threhold)[2 * bank.zc:]
                zeroed[s] += int(((g == 0) & (x[s] != 0)).sum())   # samples of quiet frames (the gate zeroes one hop at a time)
                kept[s] += int((g != 0).sum())                     # samples of frames that are not quiet
                gated_blocks[s] += 1
        out = bank.process(x)
        assert out.shape == (S, bank.block_frame)
        for s in range(S):
            ref = solos[s].process(d["indata"][(j + s) % K])
            assert torch.equal(out[s], ref), "block %d session %d: max abs %.3e" % (j, s, float((out[s] - ref).abs().max()))
            assert int(bank.last_offsets[s]) == int(solos[s].last_offset), (j, s)
            assert torch.equal(bank.sola_buffer[s], solos[s].sola_buffer), (j, s)
            assert torch.equal(bank.rvc.seen[j][s], solos[s].input_wav_res), "block %d session %d: the 16 kHz window" % (j, s)
            assert torch.equal(bank.input_wav[s], solos[s].input_wav), (j, s)
            if device_gate:
                assert torch.equal(bank.rms_buffer[s], solos[s].rms_buffer), "block %d session %d: rms_buffer" % (j, s)
            else:
                assert np.array_equal(bank.rms_buffer[s], solos[s].rms_buffer), "block %d session %d: rms_buffer" % (j, s)
    assert gated_blocks == [8, 3, 8]
    for s in range(S):
        assert zeroed[s] >= bank.zc // 2 and kept[s] >= bank.zc // 2, "session %d: %d samples zeroed, %d kept over the run" % (s, zeroed[s], kept[s])


@pytest.mark.parametrize("device_gate", [True, False])
def test_realtime_bank_sliders_beside_a_noise_reduction_box(device_gate, gpu):
    """The 16 kHz window has three ranges then: session 0 gates and has its input box ticked (the denoised ``blk + 2 zc``), session 1 has the
    box and does not gate, session 2 gates without a box (``m + 2 zc`` of the gated input); its threshold moves to -60 before block 2."""
    import rvc_amd

    d = load_golden("gui_stream_mix48k")
    K = d["indata"].shape[0]
    kw = dict(samplerate=int(d["samplerate"]), block_time=float(d["block_time"]), crossfade_time=float(d["crossfade_time"]),
              extra_time=float(d["extra_time"]), threhold=float(d["threhold"]), rms_mix_rate=float(d["rms_mix_rate"]), use_pv=bool(d["use_pv"]),
              device=gpu, device_gate=device_gate)
    thr, mix, box = [-40, -60, -14], [0.25, 0.5, 1.0], [True, True, False]
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **kw)
    solos = [rvc_amd.RealtimeStream(_SoloStub(d, gpu, [(j + s) % K for j in range(K)]), I_noise_reduce=box[s], **kw) for s in range(S)]
    for s in range(S):
        bank.set_threhold(s, thr[s])
        bank.set_rms_mix_rate(s, mix[s])
        bank.set_noise_reduce(s, I=box[s])
        solos[s].threhold, solos[s].rms_mix_rate = thr[s], mix[s]
    for j in range(K):
        if j == 2:
            bank.set_threhold(2, -60)
            solos[2].threhold = -60
        out = bank.process(np.stack([_mono(d["indata"][(j + s) % K]) for s in range(S)]))
        for s in range(S):
            ref = solos[s].process(d["indata"][(j + s) % K])
            assert torch.equal(bank.rvc.seen[j][s], solos[s].input_wav_res), "block %d session %d: the 16 kHz window" % (j, s)
            assert torch.equal(out[s], ref), "block %d session %d: max abs %.3e" % (j, s, float((out[s] - ref).abs().max()))
            assert int(bank.last_offsets[s]) == int(solos[s].last_offset) and torch.equal(bank.sola_buffer[s], solos[s].sola_buffer), (j, s)
            assert torch.equal(bank.input_wav[s], solos[s].input_wav), (j, s)
            if box[s]:
                assert torch.equal(bank.input_wav_denoise[s], solos[s].input_wav_denoise) and torch.equal(bank.nr_buffer[s], solos[s].nr_buffer), (j, s)


# ---- 7. launch counts ---------------------------------------------------------------------------------------------------------------------

BANK_KW = dict(samplerate=48000, block_time=0.15, crossfade_time=0.14, extra_time=0.4)   # 70 frames, skip_head 40, return_length 20
KEYS = [2, -3, 0.35, 1, -1]


def _launches(fn, gpu):
    """Kernels and device-to-device copies ``fn`` enqueues, by torch.profiler (as tests/test_gpu_rt_bank_gate.py counts them)."""
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


@pytest.fixture()
def pinned(vc_setup):
    """The generator's ResBlock family pinned for a count (its own choice follows the number of rows, i.e. S)."""
    net, _ = vc_setup
    for k, v in (("RB_STREAM", 0), ("NO_RB_SPLIT", 1)):
        net.dec.set_option(k, v)
    yield
    for k in ("RB_STREAM", "NO_RB_SPLIT"):
        net.dec.set_option(k, None)
    net.rows = slice(0, S_NET)


def _feeder_bank(net, index, gpu, n, setup, **kw):
    """A bank over the stub feeders, two blocks warm; ``setup(bank)`` moves its sliders before the first block."""
    import rvc_amd

    net.rows = slice(0, n)
    rvc = cases.stub_rvc(net, index, gpu, 0)
    bank = rvc_amd.RealtimeBank(rvc, sessions=n, device=gpu, device_gate=True, **dict(BANK_KW, **kw))
    for s in range(n):
        bank.set_key(s, KEYS[s])
    setup(bank)
    rng = np.random.default_rng(100 + n)
    x = np.stack([np.stack([gc.stretches(rng, bank.block_frame, bank.zc, -40, spread=6.0) for _ in range(n)]) for _ in range(3)])
    bank.process(x[0])
    bank.process(x[1])
    return bank, lambda: bank.process(x[2])


def _distinct(bank):
    """Distinct values per session, every control active in most sessions; every second session from 2 on at index_rate 0 or ungated / unmixed.
    (Sessions 0 and 1 blend at either S: the search then has 30 and 60 rows, both on the scan it takes from 16 rows on.)"""
    for s in range(bank.S):
        bank.set_index_rate(s, 0.0 if s == 2 else 0.75 - 0.1 * s)
        bank.set_protect(s, 1.0 if s == 3 else 0.6 + 0.05 * s)   # (the stub estimator's 31 frames are not p_len: no protect below 0.5, rtrvc.py:229)
        bank.set_rms_mix_rate(s, 1.0 if s == 1 else 0.1 * s)
        bank.set_threhold(s, -60 if s == 4 else -45 + 3 * s)


def test_launch_count_with_distinct_sliders_does_not_depend_on_s(vc_setup, pinned, gpu):
    net, index = vc_setup
    _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)   # (the profiler's own start-up)
    counts = {}
    for n in (2, 5):
        bank, step = _feeder_bank(net, index, gpu, n, _distinct)
        counts[n] = _launches(step, gpu)
        for k in ("k_input_gate_sessions", "k_gate_stage_sessions", "k_envelope_mix_sessions", "k_blend_expand_sessions", "k_gather_session_rows"):
            assert sum(k in name for name in counts[n]) == 1, (n, k)
        assert sum("k_frame_rms_sessions" in name for name in counts[n]) == 3
        assert not any("k_input_gate_batch" in name or "k_envelope_mix_batch" in name or "k_blend_expand_batch" in name for name in counts[n])
    assert len(counts[2]) == len(counts[5]), _diff(counts[2], counts[5])


def test_sliders_at_the_bank_wide_values_issue_the_launches_of_a_bank_without_them(vc_setup, pinned, gpu):
    net, index = vc_setup
    _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)

    def explicit(bank):
        for s in range(bank.S):
            bank.set_index_rate(s, cases.INDEX_RATE)
            bank.set_protect(s, 1.0)
            bank.set_rms_mix_rate(s, 0.25)
            bank.set_threhold(s, -40)

    kw = dict(rms_mix_rate=0.25, threhold=-40)
    plain = _launches(_feeder_bank(net, index, gpu, S, lambda bank: None, **kw)[1], gpu)
    same = _launches(_feeder_bank(net, index, gpu, S, explicit, **kw)[1], gpu)
    assert plain == same, _diff(plain, same)
    assert not any("_sessions" in name or "k_gather_session_rows" in name for name in same)
    assert any("k_input_gate_batch" in name for name in same) and any("k_envelope_mix_batch" in name for name in same)


# ---- 8. refusals: errors, never a launch ------------------------------------------------------------------------------------------------

def test_sessions_entries_refuse_bad_arguments(gpu):
    import rvc_amd
    from rvc_amd import _lib

    L, st, p = _lib.lib(), _lib.stream_ptr(gpu), _lib.ptr
    nan = float("nan")

    def both(struct, rows):
        arr = (struct * len(rows))(*[struct(*r) for r in rows])
        dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(gpu)
        return arr, C.cast(arr, C.c_void_p), dev

    zc, blk, n = 160, 480, 800
    x = torch.full((S, n), 5.0, device=gpu)
    wav = torch.full((S, n), 6.0, device=gpu)
    block = torch.full((S, blk), 0.5, device=gpu)
    rbuf = torch.full((S, 4 * zc), 8.0, device=gpu)
    dst = torch.full((S, blk + 2 * zc), 9.0, device=gpu)
    scratch = torch.zeros(S * 4000, device=gpu)
    feats = torch.ones(S, NQ, 256, device=gpu)
    pf = torch.ones(S, PLEN, device=gpu)
    out = torch.full((S, PLEN, 256), 4.0, device=gpu)
    _, mix_h, mix_d = both(_lib.SessionMix, [(1.0, 1)] * S)
    _, mix_nan_h, mix_nan_d = both(_lib.SessionMix, [(1.0, 1), (nan, 1), (0.5, 1)])
    _, gate_h, gate_d = both(_lib.SessionGate, [(0.01, 100.0, 1, 0)] * S)
    _, gate_nan_h, gate_nan_d = both(_lib.SessionGate, [(0.01, 100.0, 1, 0), (nan, 100.0, 1, 0), (0.01, 100.0, 1, 0)])
    _, bl_h, bl_d = both(_lib.SessionBlend, [(0.0, 0.33, -1, 1)] * S)
    _, bl_nan_h, bl_nan_d = both(_lib.SessionBlend, [(0.0, 0.33, -1, 1), (nan, 0.33, -1, 1), (0.0, 0.33, -1, 1)])
    _, bl_slot_h, bl_slot_d = both(_lib.SessionBlend, [(0.5, 0.33, 0, 1)] * S)     # a slot, and no index handle

    def mix(S_, ins, ws, host, dev):
        return L.rvcmi_glue_envelope_mix_sessions(S_, p(x), ins, p(wav), ws, n, zc, host, p(dev), p(scratch), st)

    def gate(S_, bs, rs, ds, host, dev):
        return L.rvcmi_glue_input_gate_sessions(S_, p(block), bs, p(rbuf), rs, p(dst), ds, zc, blk, host, p(dev), p(scratch), st)

    def blend(S_, p_len, host, dev, pitchf=pf):
        return L.rvcmi_ivf_search_blend_expand_sessions(None, S_, NQ, 256, SKIP, p(feats), host, p(dev), 8, 1, p(pitchf), p_len, p(out), st)

    bad = [mix(0, n, n, mix_h, mix_d), mix(S, n, n, mix_nan_h, mix_nan_d), mix(S, n - 1, n, mix_h, mix_d), mix(S, n, n - 1, mix_h, mix_d),
           mix(S, n, n, None, mix_d), mix(65536, n, n, mix_h, mix_d),
           gate(0, blk, 4 * zc, blk + 2 * zc, gate_h, gate_d), gate(S, blk, 4 * zc, blk + 2 * zc, gate_nan_h, gate_nan_d),
           gate(S, blk - 1, 4 * zc, blk + 2 * zc, gate_h, gate_d), gate(S, blk, 4 * zc - 1, blk + 2 * zc, gate_h, gate_d),
           gate(S, blk, 4 * zc, blk + 2 * zc - 1, gate_h, gate_d), gate(S, blk, 4 * zc, blk + 2 * zc, None, gate_d),
           blend(0, PLEN, bl_h, bl_d), blend(S, PLEN, bl_nan_h, bl_nan_d), blend(S, 2 * NQ + 1, bl_h, bl_d), blend(S, PLEN, bl_slot_h, bl_slot_d),
           blend(S, PLEN, bl_h, bl_d, pitchf=None), blend(S, PLEN, None, bl_d)]
    assert bad == [_lib.ERR_INVALID] * len(bad), bad
    torch.cuda.synchronize(gpu)
    assert bool((wav == 6.0).all()) and bool((dst == 9.0).all()) and bool((rbuf == 8.0).all()) and bool((out == 4.0).all())
    # ... and a call that is fine does write (the canaries above prove something)
    assert mix(S, n, n, mix_h, mix_d) == 0 and gate(S, blk, 4 * zc, blk + 2 * zc, gate_h, gate_d) == 0 and blend(S, PLEN, bl_h, bl_d) == 0
    torch.cuda.synchronize(gpu)
    assert not bool((wav == 6.0).all()) and not bool((dst == 9.0).any()) and not bool((out == 4.0).any())
    # the Python layer
    with pytest.raises(ValueError):
        rvc_amd.glue.envelope_mix_sessions(x, wav, zc, (0.5, nan, 0.5))
    with pytest.raises(ValueError):
        rvc_amd.glue.envelope_mix_sessions(x, wav, zc, (0.5, 0.5))
    with pytest.raises(ValueError):
        rvc_amd.glue.input_gate_sessions(block, rbuf, dst, zc, (-40, nan, -40))
    with pytest.raises(ValueError):
        rvc_amd.glue.input_gate_sessions(block, rbuf, dst[:, :-1], zc, (-40, -40, -40))
    with pytest.raises(ValueError):
        rvc_amd.glue.retrieve_blend_expand_sessions(feats, None, (0.5, nan, 0.5), pf, (0.33,) * 3, PLEN)
    with pytest.raises(ValueError):
        rvc_amd.glue.retrieve_blend_expand_sessions(feats[:0], None, (), pf[:0], (), PLEN)
    stub = type("R", (), {"tgt_sr": 40000})()
    bank = rvc_amd.RealtimeBank(stub, sessions=S, samplerate=40000, block_time=0.1, extra_time=0.5, device=gpu)
    for setter in (bank.set_index_rate, bank.set_protect, bank.set_rms_mix_rate, bank.set_threhold):
        with pytest.raises(IndexError):
            setter(S, 0.5)
        with pytest.raises(ValueError):
            setter(0, nan)
        setter(0, 0.5)
        setter(0, None)
    vc = rvc_amd.RealtimeVCBatch(type("N", (), {})(), S, device=gpu)
    for setter in (vc.set_session_index_rate, vc.set_session_protect):
        with pytest.raises(IndexError):
            setter(-1, 0.5)
        with pytest.raises(ValueError):
            setter(0, float("inf"))
    bank.set_threhold(1, -30)
    bank.reset(1)
    assert bank.sliders.own["threhold"] == [None, -30.0, None]   # reset leaves the sliders as it leaves the key
