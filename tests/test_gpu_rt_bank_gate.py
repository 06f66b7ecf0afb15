"""The realtime bank without per-session work: the input gate on the device (``device_gate=True``) and the ragged f0 decode inside
``rvc_infer_batch_hip``.

1. ``RealtimeBank(device_gate=True)`` against the host-gate bank, bit for bit, also with a noise-reduction box ticked; 2. ``RealtimeStream``
likewise, on the committed GUI fixtures that gate; 3. the pitch ``rvc_infer_batch_hip`` hands on equals the per-session ``glue.rmvpe_f0``; 4. the
launch counts: independent of S with feeders and gate, and untouched with the gate off."""
import numpy as np
import pytest
import torch

import input_gate_cases as gc
import rt_bank_cases as cases
from conftest import load_golden

pytestmark = pytest.mark.gpu

S = 3
BANK_KW = dict(samplerate=48000, block_time=0.15, crossfade_time=0.14, extra_time=0.4)   # 70 frames, skip_head 40, return_length 20
THREHOLD = -40


@pytest.fixture(scope="module")
def vc_setup(gpu):
    import rvc_amd

    idx = cases.index_768()
    index = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], device=gpu)
    return cases.BankNet(gpu, S), index


class _BankRVC:
    """``rtrvc.RVC``-like without feeders (fixed HuBERT features and f0 per session) around a ``RealtimeVCBatch``; records the 16 kHz windows."""

    def __init__(self, vc, feats, pitch, pitchf):
        self.vc, self.feats, self.pitch, self.pitchf, self.tgt_sr, self.seen = vc, feats, pitch, pitchf, 48000, []

    def infer_batch(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method, keys, sids, **kw):
        self.seen.append(input_wav_res.clone())
        return self.vc.infer(self.feats, int(input_wav_res.shape[1]), block_frame_16k, skip_head, return_length, pitch=self.pitch, pitchf=self.pitchf,
                             protect=cases.PROTECT, sid=sids)


def _gated_blocks(n, blocks, block_frame, zc, seed=0):
    """[blocks][n, block_frame]: noise whose level moves around the threshold every three hops, with a silent stretch in session 0."""
    rng = np.random.default_rng(100 + seed)
    x = np.stack([np.stack([gc.stretches(rng, block_frame, zc, THREHOLD, spread=6.0) for _ in range(n)]) for _ in range(blocks)])
    x[:, 0, : block_frame // 3] = 0
    return x


def _bank(net, index, gpu, n, **kw):
    import rvc_amd

    feats, pitch, pitchf = (t[:n].to(gpu) for t in cases.vc_blocks(S, 1)[0])
    vc = rvc_amd.RealtimeVCBatch(net, n, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000)
    return rvc_amd.RealtimeBank(_BankRVC(vc, feats, pitch, pitchf), sessions=n, device=gpu, **dict(BANK_KW, **kw))


@pytest.mark.parametrize("box", [None, "I"])
def test_bank_with_the_device_gate_equals_the_host_gate_bank(box, vc_setup, gpu):
    """S = 3, threhold -40, three blocks and a ``reset(1)`` after the first.  ``box``: session 2 has its input noise reduction ticked (its
    16 kHz write range is blk + 2 zc samples of the denoised input, the others' m + 2 zc of the gated input)."""
    net, index = vc_setup
    net.rows = slice(0, S)
    host, dev = _bank(net, index, gpu, S, threhold=THREHOLD, device_gate=False), _bank(net, index, gpu, S, threhold=THREHOLD, device_gate=True)
    assert isinstance(host.rms_buffer, np.ndarray) and torch.is_tensor(dev.rms_buffer) and dev.rms_buffer.shape == (S, 4 * dev.zc) and dev.rms_buffer.is_cuda
    if box:
        for b in (host, dev):
            b.set_noise_reduce(2, I=True)
    x = _gated_blocks(S, 3, host.block_frame, host.zc)
    zeroed = 0
    for j in range(3):
        if j == 1:
            host.reset(1)
            dev.reset(1)
            assert not bool(dev.rms_buffer[1].any()) and bool(dev.rms_buffer[0].any())
        want, got = host.process(x[j]), dev.process(x[j])
        assert torch.equal(got, want), "block %d: max abs %.3e" % (j, float((got - want).abs().max()))
        assert torch.equal(dev.input_wav, host.input_wav) and torch.equal(dev.input_wav_res, host.input_wav_res)
        assert torch.equal(dev.rvc.seen[-1], host.rvc.seen[-1])
        assert torch.equal(dev.sola_buffer, host.sola_buffer) and torch.equal(dev.last_offsets, host.last_offsets)
        assert np.array_equal(dev.rms_buffer.cpu().numpy(), host.rms_buffer)
        if box:
            assert torch.equal(dev.input_wav_denoise, host.input_wav_denoise) and torch.equal(dev.nr_buffer, host.nr_buffer)
        tail = host.input_wav[:, -host.block_frame:].cpu().numpy()
        zeroed += int(((tail == 0) & (x[j] != 0)).sum())
        assert ((tail != 0) & (x[j] != 0)).any()
    assert zeroed > host.zc   # the gate did close on something


@pytest.mark.parametrize("case", ["mix48k", "pv44k"])
def test_stream_with_the_device_gate_equals_the_host_gate_stream(case, gpu):
    """The committed GUI fixtures whose ``threhold`` is above -60 (-40 at 48 kHz, -50 at 44.1 kHz where zc is odd)."""
    import rvc_amd

    d = load_golden("gui_stream_" + case)
    assert float(d["threhold"]) > -60

    class Stub:
        def __init__(self):
            self.j, self.tgt_sr = 0, int(d["tgt_sr"])

        def infer(self, input_wav_res, block_frame_16k, skip_head, return_length, f0method):
            self.j += 1
            return torch.from_numpy(d["chunks"][self.j - 1]).to(gpu)

    kw = dict(samplerate=int(d["samplerate"]), block_time=float(d["block_time"]), crossfade_time=float(d["crossfade_time"]),
              extra_time=float(d["extra_time"]), threhold=float(d["threhold"]), rms_mix_rate=float(d["rms_mix_rate"]), use_pv=bool(d["use_pv"]), device=gpu)
    host, dev = rvc_amd.RealtimeStream(Stub(), device_gate=False, **kw), rvc_amd.RealtimeStream(Stub(), device_gate=True, **kw)
    assert torch.is_tensor(dev.rms_buffer) and isinstance(host.rms_buffer, np.ndarray)
    for j in range(d["indata"].shape[0]):
        want, got = host.process(d["indata"][j]), dev.process(d["indata"][j])
        assert torch.equal(got, want), j
        assert torch.equal(dev.input_wav, host.input_wav) and torch.equal(dev.input_wav_res, host.input_wav_res) and torch.equal(dev.sola_buffer, host.sola_buffer)
        assert int(dev.last_offset) == int(host.last_offset) and np.array_equal(dev.rms_buffer.cpu().numpy(), host.rms_buffer)


# ---- rvc_infer_batch_hip with the stub feeders ----------------------------------------------------------------------------------------------

E2E_KEYS = [2, -3, 0.35]   # distinct, one fractional


def test_rvc_infer_batch_hip_hands_on_the_per_session_decode(vc_setup, gpu):
    import rvc_amd
    from rvc_amd.pipeline import RMVPE_THRED
    from rvc_amd.realtime import f0_extractor_frame, rvc_infer_batch_hip

    net, index = vc_setup
    net.rows = slice(0, S)
    both = cases.stub_rvc(net, index, gpu, 0)
    rt = rvc_amd.RealtimeVCBatch(net, S, index=index, index_rate=cases.INDEX_RATE, device=gpu, tgt_sr=48000)
    handed, real = [], rt.infer

    def spy(*a, **k):
        handed.append((k["pitch"].clone(), k["pitchf"].clone()))
        return real(*a, **k)

    rt.infer = spy
    n = f0_extractor_frame(cases.BLOCK_16K, "rmvpe", cases.WINDOW)
    for wav in cases.e2e_waves(S, 2):
        w = wav.to(gpu)
        rvc_infer_batch_hip(both, w, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0, keys=E2E_KEYS, sids=[0, 0, 0], rt=rt)
        pitch, pitchf = handed[-1]
        feeder = cases.FramingRMVPE(gpu)
        hidden = feeder._mel2hidden(feeder.mel_extractor(w[:, -n:].float(), center=True))
        m = n // cases.WINDOW
        assert pitch.shape == pitchf.shape == (S, m) and pitch.dtype == torch.int64 and pitchf.dtype == torch.float32
        for s in range(S):
            wp, wpf = rvc_amd.glue.rmvpe_f0(hidden[s].float().contiguous(), m, E2E_KEYS[s], RMVPE_THRED)
            assert torch.equal(pitch[s], wp[0]) and torch.equal(pitchf[s], wpf[0]), s
        assert float(pitchf.max()) > 0 and not torch.equal(pitchf[0], pitchf[1])
    assert both.f0_gen.rmvpe.batches == [S, S]


# ---- launch counts ----------------------------------------------------------------------------------------------------------------------

def _launches(fn, gpu):
    """Kernels and device-to-device copies ``fn`` enqueues, by torch.profiler (as tests/test_gpu_rt_formant.py counts them)."""
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
    net.rows = slice(0, S)


def test_rvc_infer_batch_hip_launch_count_does_not_depend_on_s(vc_setup, pinned, gpu):
    from rvc_amd.realtime import rvc_infer_batch_hip

    net, index = vc_setup
    _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)   # (the profiler's own start-up)
    counts = {}
    for n in (2, 3):
        net.rows = slice(0, n)
        rvc = cases.stub_rvc(net, index, gpu, 0)
        waves = [w.to(gpu) for w in cases.e2e_waves(n, 2)]
        step = lambda w: rvc_infer_batch_hip(rvc, w, cases.BLOCK_16K, cases.SKIP_HEAD, cases.RETURN_LENGTH, "rmvpe", 1.0, keys=E2E_KEYS[:n], sids=[0] * n)  # noqa: E731
        step(waves[0])
        counts[n] = _launches(lambda: step(waves[1]), gpu)
        assert sum("k_f0_post_ragged" in k for k in counts[n]) == 1 and sum("k_rmvpe_decode" in k for k in counts[n]) == 1
        assert not any("k_f0_post" in k and "ragged" not in k for k in counts[n])   # no decode per session
    assert len(counts[2]) == len(counts[3]), _diff(counts[2], counts[3])


def _feeder_bank(net, index, gpu, n, **kw):
    import rvc_amd

    net.rows = slice(0, n)
    rvc = cases.stub_rvc(net, index, gpu, 0)
    bank = rvc_amd.RealtimeBank(rvc, sessions=n, device=gpu, **dict(BANK_KW, **kw))
    for s in range(n):
        bank.set_key(s, E2E_KEYS[s])
    x = _gated_blocks(n, 3, bank.block_frame, bank.zc, seed=n)
    bank.process(x[0])
    bank.process(x[1])
    return bank, lambda: bank.process(x[2])


def test_whole_bank_step_launch_count_does_not_depend_on_s(vc_setup, pinned, gpu):
    """``RealtimeBank.process`` with threhold -40, the device gate and the stub feeders: S = 2 and S = 3 issue the same number of launches."""
    net, index = vc_setup
    _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)
    counts = {}
    for n in (2, 3):
        bank, step = _feeder_bank(net, index, gpu, n, threhold=THREHOLD, device_gate=True)
        counts[n] = _launches(step, gpu)
        assert sum("k_input_gate_batch" in k for k in counts[n]) == 1 and sum("k_gate_stage_batch" in k for k in counts[n]) == 1
        assert sum("k_f0_post_ragged" in k for k in counts[n]) == 1
    assert len(counts[2]) == len(counts[3]), _diff(counts[2], counts[3])


def test_gate_off_issues_the_launches_of_a_bank_without_the_argument(vc_setup, pinned, gpu):
    net, index = vc_setup
    _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)
    plain = _launches(_feeder_bank(net, index, gpu, S, threhold=-60)[1], gpu)
    with_arg = _launches(_feeder_bank(net, index, gpu, S, threhold=-60, device_gate=True)[1], gpu)
    assert plain == with_arg, _diff(plain, with_arg)
    assert not any("k_input_gate_batch" in k or "k_gate_stage_batch" in k for k in with_arg)
