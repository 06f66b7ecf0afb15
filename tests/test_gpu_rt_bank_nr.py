"""Per-session noise reduction in the realtime bank: ``RealtimeBank.set_noise_reduce`` over the committed GUI fixtures
``gui_stream_nr_*`` against solo ``RealtimeStream`` runs with the same boxes -- bit for bit, every rolling buffer included -- and, for
session 0, against the reference-made fixture at the bars tests/test_gpu_torchgate.py holds the solo stream to; a mixed bank, ``reset``,
and the launch count, which may depend on whether any session has a box ticked but never on ``S``."""
import numpy as np
import pytest
import torch

from conftest import load_golden

S = 3
CASES = ["i48k", "o40k", "io44k", "toggle48k", "pv40k"]


class _SoloStub:
    """``rtrvc.RVC``-like for one ``RealtimeStream``: returns the fixture's chunks in the session's (cyclically shifted) order and keeps
    the 16 kHz window it was handed."""

    def __init__(self, d, dev, order):
        self.d, self.dev, self.order, self.j, self.seen = d, dev, list(order), 0, []
        self.tgt_sr = int(d["tgt_sr"])

    def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
        j = self.order[self.j]
        self.j += 1
        self.seen.append(input_wav_res.clone())
        return torch.from_numpy(self.d["chunks"][j]).to(self.dev)


class _BankStub:
    """The same for a bank of ``n`` sessions: session s's chunk is the fixture's shifted by s."""

    def __init__(self, d, dev, n=S):
        self.d, self.dev, self.n, self.j, self.seen = d, dev, n, 0, []
        self.tgt_sr = int(d["tgt_sr"])

    def infer_batch(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method, keys, sids):
        d, K = self.d, self.d["chunks"].shape[0]
        assert (block_frame_16k, skip_head, return_length) == (int(d["block_frame_16k"]), int(d["skip_head"]), int(d["return_length"]))
        assert input_wav_res.is_cuda and input_wav_res.shape == (self.n,) + d["input_wav_res"][0].shape
        self.seen.append(input_wav_res.clone())
        out = torch.from_numpy(np.stack([d["chunks"][(self.j + s) % K] for s in range(self.n)])).to(self.dev)
        self.j += 1
        return out


def _mono(x):
    x = np.asarray(x, dtype=np.float32)
    return np.mean(x.T, axis=0) if x.ndim == 2 else x


def _kw(d, gpu):
    return dict(samplerate=int(d["samplerate"]), block_time=float(d["block_time"]), crossfade_time=float(d["crossfade_time"]),
                extra_time=float(d["extra_time"]), threhold=float(d["threhold"]), rms_mix_rate=float(d["rms_mix_rate"]), use_pv=bool(d["use_pv"]),
                device=gpu)


def _rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


def _order(K, s, start=0):
    return [(j + s) % K for j in range(start, K)]


def _same_state(bank, solos, s, j, out, ref):
    what = "block %d session %d" % (j, s)
    assert torch.equal(out[s], ref), what + ": output block, max abs %.3e" % float((out[s] - ref).abs().max())
    assert int(bank.last_offsets[s]) == int(solos[s].last_offset), what + ": SOLA offset"
    assert torch.equal(bank.rvc.seen[j][s], solos[s].rvc.seen[-1]), what + ": the 16 kHz window handed to the model"
    for name in ("sola_buffer", "input_wav_denoise", "nr_buffer", "output_buffer", "input_wav", "input_wav_res"):
        assert torch.equal(getattr(bank, name)[s], getattr(solos[s], name)), what + ": " + name


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_bank_with_per_session_boxes_equals_solo_streams_and_the_fixture(case, gpu):
    """Session s is fed the fixture's blocks cyclically shifted by s, with the fixture's per-block boxes shifted likewise (in toggle48k the
    sessions therefore switch at different blocks)."""
    import rvc_amd

    d = load_golden("gui_stream_nr_" + case)
    K = d["indata"].shape[0]
    kw = _kw(d, gpu)
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **kw)
    solos = [rvc_amd.RealtimeStream(_SoloStub(d, gpu, _order(K, s)), **kw) for s in range(S)]
    for j in range(K):
        for s in range(S):
            I, O = bool(d["I_noise_reduce"][(j + s) % K]), bool(d["O_noise_reduce"][(j + s) % K])
            bank.set_noise_reduce(s, I=I, O=O)
            solos[s].I_noise_reduce, solos[s].O_noise_reduce = I, O
        out = bank.process(np.stack([_mono(d["indata"][(j + s) % K]) for s in range(S)]))
        assert out.is_cuda and out.shape == (S, d["out"][j].shape[0])
        for s in range(S):
            _same_state(bank, solos, s, j, out, solos[s].process(d["indata"][(j + s) % K]))
        assert int(bank.last_offsets[0]) == int(d["offsets"][j]), j
        err = out[0].cpu().numpy().astype(np.float64) - d["out"][j]
        bar_max, bar_rms = (2e-5, 2.5e-6) if bool(d["use_pv"]) else (5e-7, 6e-8)
        assert np.abs(err).max() <= bar_max and _rms(err) <= bar_rms, "block %d: max %.2e rms %.2e" % (j, np.abs(err).max(), _rms(err))
    # the cache was used: a session ticked in two consecutive blocks ran warm in the second
    for gate, key in ((bank.gate_I, "I_noise_reduce"), (bank.gate_O, "O_noise_reduce")):
        if d[key][K - 2] and d[key][K - 1]:
            assert gate.last_modes[0] == 1 and gate.ring is not None and gate.ring.numel() == gate.ring_bytes
        elif not d[key].any():
            assert gate is None


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["io44k", "pv40k"])
def test_mixed_bank(case, gpu):
    """Session 0 has I only, session 1 O only, session 2 neither: session 2 equals a plain solo stream and its noise-reduction buffers stay
    all zero.  io44k runs the host input gate, so the 16 kHz write-back ranges of sessions 0 and 1 differ by 320 samples."""
    import rvc_amd

    d = load_golden("gui_stream_nr_" + case)
    K = d["indata"].shape[0]
    kw = _kw(d, gpu)
    boxes = [(True, False), (False, True), (False, False)]
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **kw)
    solos = []
    for s, (I, O) in enumerate(boxes):
        bank.set_noise_reduce(s, I=I, O=O)
        solos.append(rvc_amd.RealtimeStream(_SoloStub(d, gpu, _order(K, s)), I_noise_reduce=I, O_noise_reduce=O, **kw))
    for j in range(K):
        out = bank.process(np.stack([_mono(d["indata"][(j + s) % K]) for s in range(S)]))
        for s in range(S):
            _same_state(bank, solos, s, j, out, solos[s].process(d["indata"][(j + s) % K]))
    assert not bank.input_wav_denoise[2].any() and not bank.nr_buffer[2].any() and not bank.output_buffer[2].any()
    assert not bank.output_buffer[0].any() and not bank.input_wav_denoise[1].any()
    assert bank.input_wav_denoise[0].any() and bank.output_buffer[1].any()
    assert bank.gate_I.last_modes == [1, 0, 0] and bank.gate_O.last_modes == [0, 1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["io44k", "toggle48k"])
def test_reset_touches_one_session_and_keeps_its_boxes(case, gpu):
    """``reset(1)`` after two blocks: sessions 0 and 2 go on as their solo streams do, session 1 equals a FRESH solo stream with the same
    boxes (its cached spectra are dropped: it runs cold)."""
    import rvc_amd

    d = load_golden("gui_stream_nr_" + case)
    K = d["indata"].shape[0]
    kw = _kw(d, gpu)
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **kw)
    solos = [rvc_amd.RealtimeStream(_SoloStub(d, gpu, _order(K, s)), **kw) for s in range(S)]
    for j in range(K):
        if j == 2:
            bank.reset(1)
            solos[1] = rvc_amd.RealtimeStream(_SoloStub(d, gpu, _order(K, 1, 2)), **kw)
            assert not bank.input_wav_denoise[1].any() and not bank.nr_buffer[1].any() and not bank.output_buffer[1].any()
        for s in range(S):
            I, O = bool(d["I_noise_reduce"][(j + s) % K]), bool(d["O_noise_reduce"][(j + s) % K])
            if j != 2 or s != 1:      # (reset keeps session 1's boxes of block 1; the fresh solo gets them too)
                bank.set_noise_reduce(s, I=I, O=O)
            solos[s].I_noise_reduce, solos[s].O_noise_reduce = bank.I_noise_reduce[s], bank.O_noise_reduce[s]
        out = bank.process(np.stack([_mono(d["indata"][(j + s) % K]) for s in range(S)]))
        if j == 2:
            for gate, flags in ((bank.gate_I, bank.I_noise_reduce), (bank.gate_O, bank.O_noise_reduce)):
                if gate is not None and flags[1]:
                    assert gate.last_modes[1] == 2
        for s in range(S):
            _same_state(bank, solos, s, j, out, solos[s].process(d["indata"][(j + s) % K]))


def _launches(fn, gpu):
    """What ``fn`` enqueues on the device, counted by torch.profiler: kernels and device-to-device copies (torch turns a copy between
    contiguous tensors -- every [1, n] slice is one -- into a copy command instead of a kernel, so the two are counted together);
    host-to-device copies (the block, a mode vector that changed) and memsets are not."""
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


def _warm_bank(d, gpu, n, boxes, touch=False):
    """A bank of n sessions after two blocks; -> a closure that processes the third."""
    import rvc_amd

    K = d["indata"].shape[0]
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu, n), sessions=n, **_kw(d, gpu))
    for s in range(n):
        if boxes is not None:
            bank.set_noise_reduce(s, I=boxes[0], O=boxes[1])
    blocks = lambda j: np.stack([_mono(d["indata"][(j + s) % K]) for s in range(n)])   # noqa: E731
    for j in range(2):
        bank.process(blocks(j))
    if touch:   # boxes that were ticked and are not any more: the gates exist, nothing may be launched for them
        for s in range(n):
            bank.set_noise_reduce(s, I=False, O=False)
        bank.process(blocks(2))
        return bank, lambda: bank.process(blocks(3))
    return bank, lambda: bank.process(blocks(2))


@pytest.mark.gpu
def test_launch_count_does_not_depend_on_the_number_of_sessions(gpu):
    """One warm ``process`` with both boxes ticked everywhere at S = 1 and S = 3: the same kernels, the same number of times.  With no box
    ticked: the launches of a bank that never heard of noise reduction, whether the boxes were never touched or ticked and unticked."""
    d = load_golden("gui_stream_nr_io44k")
    _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)   # (the profiler's own start-up)
    counts = {}
    for n in (1, 3):
        bank, step = _warm_bank(d, gpu, n, (True, True))
        counts[n] = _launches(step, gpu)
        assert bank.gate_I.last_modes == [1] * n and bank.gate_O.last_modes == [1] * n
    assert len(counts[1]) > 12 and len(counts[1]) == len(counts[3]), _diff(counts[1], counts[3])
    plain = _launches(_warm_bank(d, gpu, 3, None)[1], gpu)
    unticked = _launches(_warm_bank(d, gpu, 3, (True, True), touch=True)[1], gpu)
    only_i = _launches(_warm_bank(d, gpu, 3, (True, False))[1], gpu)
    assert len(plain) > 0 and len(plain) == len(unticked), _diff(plain, unticked)
    assert len(plain) < len(only_i) < len(counts[3])


@pytest.mark.gpu
def test_what_the_bank_still_refuses(gpu):
    import rvc_amd

    d = load_golden("gui_stream_nr_i48k")
    for bad in (dict(I_noise_reduce=True), dict(O_noise_reduce=True), dict(function="im")):
        with pytest.raises(ValueError):
            rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **dict(_kw(d, gpu), **bad))
    bank = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **_kw(d, gpu))
    with pytest.raises(IndexError):
        bank.set_noise_reduce(S, I=True)
    assert bank.gate_I is None and bank.gate_O is None
    short = rvc_amd.RealtimeBank(_BankStub(d, gpu), sessions=S, **dict(_kw(d, gpu), block_time=0.03))
    assert short.block_frame < short.sola_buffer_frame
    with pytest.raises(ValueError):
        short.set_noise_reduce(0, I=True)
    short.set_noise_reduce(0, O=True)
