"""The RMVPE f0 estimator wholly on HIP (csrc/rmvpe.hip, rvc_amd.rmvpe): log-mel front end, head, fractional key, the chain and its switch.

  * log-mel against the fp64 oracle of tests/rmvpe_cases.py (rvc/f0/mel.py:58-71 over rvc/f0/stft.py:165-180 restated).  ``round_half``: every
    element within ONE fp16 ulp, the frames of the zero gap bit-equal to log(fp16(1e-5)) -- a condition the reference's own fp32 path meets
    (tests/test_cpu_rmvpe.py).  fp32: the max abs error per signal at most 4 x the error of the torch fp32 path on the same input, computed
    here on the CPU (the margin allows another, equally valid evaluation order and twiddle source; the pure tone, whose quiet bins are the fp32
    cancellation floor, goes through this bar only);
  * the head against fp64: an error no larger than that of torch's own ``Linear`` + ``Sigmoid`` on the GPU, ``.half()`` and fp32 respectively;
  * a fractional key against the oracle restatement of the reference's decode; integer keys against the golden fixture, bit for bit;
  * the chain against the torch fp32 network (error no larger than the torch ``.half()`` chain's), ``.f0`` against the decode of its own
    salience, the refusals, the switch in ``_rmvpe_on_device`` and ``rvc_infer_hip``, and the realtime graph replay.
"""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import rmvpe_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---------------------------------------------------------------- log-mel

class _Mel:
    """A bare ``rvcmi_mel`` handle."""

    def __init__(self, basis, gpu, n_fft=rc.N_FFT, hop=rc.HOP, win=rc.N_FFT, clamp=rc.CLAMP):
        from rvc_amd import _lib

        self.L, self.gpu, self.h = _lib.lib(), gpu, C.c_void_p()
        b = basis.float().contiguous()
        self.rc = self.L.rvcmi_mel_create(n_fft, hop, win, int(b.shape[0]), C.c_void_p(b.data_ptr()), clamp, 0, C.byref(self.h))

    def __del__(self):
        if self.h:
            self.L.rvcmi_mel_destroy(self.h)

    def __call__(self, wav, half, T_pad=None, out=None):
        """wav [B, n] on the CPU -> (return code, [B, T_pad, 128] on the CPU)"""
        B, n = wav.shape
        T = int(self.L.rvcmi_mel_frames(self.h, n))
        T_pad = rc.pad32(max(T, 1)) if T_pad is None else T_pad
        x = wav.to(self.gpu).contiguous()
        out = torch.full((B, T_pad, 128), float("nan"), device=self.gpu) if out is None else out
        code = self.L.rvcmi_mel_forward(self.h, B, n, C.c_void_p(x.data_ptr()), int(half), T_pad, C.c_void_p(out.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream(self.gpu).cuda_stream))
        torch.cuda.synchronize()
        return code, out.cpu()


@functools.lru_cache(maxsize=None)
def _bank(name):
    return rc.htk_bank() if name == "htk" else rc.dense_bank()


@functools.lru_cache(maxsize=None)
def _oracle(kind, n, bank, half):
    """(oracle in the network's layout [T_pad, 128], torch fp32 path likewise, zero-gap frames) -- computed once, never changed."""
    x = rc.signal(kind, n)
    T_pad = rc.pad32(n // rc.HOP + 1)
    o64 = rc.padded_layout(rc.log_mel(x[None], _bank(bank), torch.float64, half), T_pad)[0]
    o32 = rc.padded_layout(rc.log_mel(x[None], _bank(bank), torch.float32, half), T_pad)[0]
    return o64, o32, rc.zero_frames(x)


def _check_half(got, kind, n, bank):
    want, _, gap = _oracle(kind, n, bank, True)
    T = n // rc.HOP + 1
    assert got.shape == want.shape and torch.isfinite(got).all()
    assert torch.equal(got, got.half().float()), "values that are not fp16 numbers"
    u = rc.half_ulps(got[:T], want[:T])
    print("log-mel half %s/%s n=%d: %d of %d elements not bit-equal, max %d ulp" % (kind, bank, n, int((u > 0).sum()), u.numel(), int(u.max())))
    assert int(u.max()) <= 1, "%s n=%d: %d elements beyond one fp16 ulp of the oracle" % (kind, n, int((u > 1).sum()))
    assert float(got[T:].abs().max()) == 0 if T < got.shape[0] else True, "pad frames must be exactly 0"
    if kind == "voiced" and bool(gap.any()):
        floor = float(torch.log(torch.tensor(rc.CLAMP).half()))
        assert bool((got[:T][gap] == floor).all()), "the zero gap is not log(fp16(1e-5)) bit for bit"


def _check_fp32(got, kind, n, bank):
    """-> (error of the HIP path, error of the torch fp32 path), both max abs against the fp64 oracle"""
    want, t32, _ = _oracle(kind, n, bank, False)
    T = n // rc.HOP + 1
    assert got.shape == want.shape and torch.isfinite(got).all()
    e_hip, e_torch = float((got[:T].double() - want[:T]).abs().max()), float((t32[:T].double() - want[:T]).abs().max())
    print("log-mel fp32 %s/%s n=%d: HIP %.3g, torch fp32 %.3g" % (kind, bank, n, e_hip, e_torch))
    assert e_torch > 0 and e_hip <= 4 * e_torch, "%s n=%d: HIP error %.3g against 4 x torch fp32's %.3g" % (kind, n, e_hip, e_torch)
    assert float(got[T:].abs().max()) == 0 if T < got.shape[0] else True, "pad frames must be exactly 0"
    return e_hip, e_torch


@pytest.mark.parametrize("n", rc.LENGTHS)
def test_log_mel_matches_the_oracle(n, gpu):
    mel = _Mel(_bank("htk"), gpu)
    assert mel.rc == 0 and int(mel.L.rvcmi_mel_frames(mel.h, n)) == n // rc.HOP + 1
    for kind in ("voiced", "noise", "quiet", "sine"):
        x = rc.signal(kind, n)[None]
        if kind != "sine":
            code, got = mel(x, True)
            assert code == 0
            _check_half(got[0], kind, n, "htk")
        code, got = mel(x, False)
        assert code == 0
        _check_fp32(got[0], kind, n, "htk")


def test_log_mel_batch_of_two_different_rows(gpu):
    mel = _Mel(_bank("htk"), gpu)
    n = 5120
    x = torch.stack((rc.signal("voiced", n), rc.signal("noise", n)))
    for half in (True, False):
        code, got = mel(x, half)
        assert code == 0 and got.shape == (2, 64, 128)
        for row, kind in enumerate(("voiced", "noise")):
            (_check_half if half else _check_fp32)(got[row], kind, n, "htk")
        code1, one = mel(x[1:], half)
        assert torch.equal(one[0], got[1]), "a row's result depends on the batch"


def test_log_mel_is_bit_identical_from_run_to_run_and_serves_a_longer_pad(gpu):
    mel = _Mel(_bank("htk"), gpu)
    x = rc.signal("voiced", 48077)[None]
    a = mel(x, True)[1]
    torch.empty(1 << 22, device=gpu).normal_()
    b = mel(x, True)[1]
    assert torch.equal(a, b)
    code, c = mel(x, True, T_pad=331)   # any T_pad >= T, tile-ragged too
    assert code == 0 and torch.equal(c[0, :301], a[0, :301]) and float(c[0, 301:].abs().max()) == 0


@pytest.mark.parametrize("n", (5120, 48077))
def test_log_mel_with_a_dense_bank(n, gpu):
    """No band structure to exploit: the same bars."""
    mel = _Mel(_bank("dense"), gpu)
    for kind in ("voiced", "noise", "quiet"):
        x = rc.signal(kind, n)[None]
        _check_half(mel(x, True)[1][0], kind, n, "dense")
        _check_fp32(mel(x, False)[1][0], kind, n, "dense")


def test_log_mel_refusals_leave_the_output_untouched(gpu):
    from rvc_amd import _lib

    mel = _Mel(_bank("htk"), gpu)
    for n in (512, 100):
        assert int(mel.L.rvcmi_mel_frames(mel.h, n)) == 0
        code, out = mel(torch.zeros(1, n), True, T_pad=32)
        assert code == _lib.ERR_INVALID and bool(torch.isnan(out).all())
    code, out = mel(torch.zeros(1, 5120), True, T_pad=32)       # 33 frames do not fit
    assert code == _lib.ERR_INVALID and bool(torch.isnan(out).all())
    assert _Mel(torch.rand(80, 513), gpu).rc == _lib.ERR_INVALID           # n_mels != 128
    assert _Mel(torch.rand(128, 501), gpu, n_fft=1000, win=1000).rc == _lib.ERR_INVALID
    assert _Mel(_bank("htk"), gpu, win=512).rc == _lib.ERR_INVALID
    assert _Mel(_bank("htk"), gpu, hop=0).rc == _lib.ERR_INVALID
    code, out = _Mel(_bank("htk"), gpu, hop=1)(rc.signal("noise", 600)[None], False, T_pad=601)   # any hop >= 1
    assert code == 0 and bool(torch.isfinite(out).all())


# ---------------------------------------------------------------- head

@pytest.mark.parametrize("M", (1, 31, 64, 301))
def test_head_is_no_worse_than_torch(M, gpu):
    from rvc_amd import _lib

    g = torch.Generator().manual_seed(M)
    torch.manual_seed(7)
    net = torch.nn.Sequential(torch.nn.Linear(512, 360), torch.nn.Sigmoid()).eval()
    y = torch.tanh(torch.randn(M, 512, generator=g))
    with torch.no_grad():
        want = torch.sigmoid(y.double() @ net[0].weight.double().T + net[0].bias.double())
        w, b, yd = net[0].weight.detach().to(gpu).contiguous(), net[0].bias.detach().to(gpu).contiguous(), y.to(gpu)
        for half in (True, False):
            out = torch.full((M, 360), float("nan"), device=gpu)
            _lib.check(_lib.lib().rvcmi_rmvpe_head(C.c_void_p(yd.data_ptr()), M, C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), int(half),
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
            ref_net = torch.nn.Sequential(torch.nn.Linear(512, 360), torch.nn.Sigmoid()).eval()
            ref_net.load_state_dict(net.state_dict())
            ref_net = ref_net.to(gpu)
            t = ref_net.half()(yd.half()) if half else ref_net(yd)
            torch.cuda.synchronize()
            e_hip, e_torch = float((out.cpu().double() - want).abs().max()), float((t.cpu().double() - want).abs().max())
            print("head M=%d %s: HIP %.3g, torch %.3g" % (M, "half" if half else "fp32", e_hip, e_torch))
            assert bool(torch.isfinite(out).all()) and e_hip <= e_torch, (M, half, e_hip, e_torch)


# ---------------------------------------------------------------- fractional key

def _salience(n, seed):
    rng = np.random.default_rng(seed)
    sal = (rng.random((n, 360), dtype=np.float32) * 0.02).astype(np.float32)
    centre = (150 + 100 * np.sin(np.arange(n) / 40.0)).astype(int)
    voiced = (np.arange(n) % 90) >= 20
    for w_ in range(-4, 5):
        sal[np.arange(n)[voiced], centre[voiced] + w_] += np.float32(0.9 * np.exp(-0.5 * (w_ / 2.0) ** 2))
    return sal


def test_fractional_key_matches_the_reference_decode(gpu):
    import rvc_amd
    from oracle import glue_oracle

    sal = _salience(400, 3)
    for key in (1.5, -0.35, 0.05):
        ref_p, ref_f = glue_oracle.rmvpe_f0(sal, 411, key, 0.03)
        pitch, pitchf = rvc_amd.glue.rmvpe_f0(torch.from_numpy(sal).to(gpu), 411, key, 0.03)
        assert np.array_equal(pitch[0].cpu().numpy(), ref_p), key
        assert np.allclose(pitchf[0].cpu().numpy(), ref_f, rtol=1e-6, atol=0), key
    whole_p, _ = glue_oracle.rmvpe_f0(sal, 411, 1, 0.03)
    assert not np.array_equal(rvc_amd.glue.rmvpe_f0(torch.from_numpy(sal).to(gpu), 411, 1.5, 0.03)[0][0].cpu().numpy(), whole_p), "the key was truncated"
    rng = np.random.default_rng(5)
    f0 = rng.uniform(40, 1300, 500)
    f0[rng.random(500) < 0.2] = 0.0
    for key in (-0.35, 1.5):
        ref_c, ref_f = glue_oracle.post_process(f0.copy(), key)
        pitch, pitchf = rvc_amd.glue.f0_post(torch.from_numpy(f0).to(gpu), key)
        assert np.array_equal(pitch[0].cpu().numpy(), ref_c.astype(np.int64)), key
        assert np.allclose(pitchf[0].cpu().numpy(), ref_f.astype(np.float32), rtol=1e-6, atol=0), key
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.glue.f0_post(torch.from_numpy(f0).to(gpu), float("nan"))


def test_integer_keys_still_reproduce_the_golden_fixture(gpu):
    import rvc_amd
    from conftest import load_golden
    from rvc_amd import _lib

    d = load_golden("glue_f0")
    for c in sorted({k.split("::")[0] for k in d}):
        n, p_len, key = (int(v) for v in d[c + "::meta"])
        sal = torch.from_numpy(d[c + "::salience"]).to(gpu)
        pitch, pitchf = rvc_amd.glue.rmvpe_f0(sal, p_len, key, 0.03)
        assert np.array_equal(pitch[0].cpu().numpy(), d[c + "::pitch"]), c
        assert np.allclose(pitchf[0].cpu().numpy(), d[c + "::pitchf"], rtol=1e-6, atol=0), c
        # the integer entry point of the C ABI and the float one with an integral key: the same bits
        scratch, p2, f2 = torch.empty(n, device=gpu, dtype=torch.float64), torch.empty_like(pitch[0]), torch.empty_like(pitchf[0])
        _lib.check(_lib.lib().rvcmi_glue_rmvpe_f0(C.c_void_p(sal.data_ptr()), n, 360, 0.03, p_len, key, C.c_void_p(scratch.data_ptr()),
                                                  C.c_void_p(p2.data_ptr()), C.c_void_p(f2.data_ptr()), C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
        assert torch.equal(p2, pitch[0]) and torch.equal(f2, pitchf[0]), c


# ---------------------------------------------------------------- the chain

@functools.lru_cache(maxsize=None)
def _standin(half):
    return rc.RmvpeStandIn(torch.device("cuda:0"), half)


def _wav(n, seed=0):
    return rc.signal("voiced", n, seed) + 0.3 * rc.signal("noise", n, seed + 1)


@pytest.mark.parametrize("n", (5120, 48077))
def test_salience_against_the_torch_fp32_network(n, gpu):
    """Error against the torch fp32 chain (mel in fp32, network in fp32) no larger than that of the torch ``.half()`` chain."""
    import rvc_amd

    r32, r16 = _standin(False), _standin(True)
    hip = rvc_amd.RMVPEHIP.from_reference(r16)
    assert hip is not None and hip.is_half
    wav = _wav(n).to(gpu)
    T = n // rc.HOP + 1
    with torch.no_grad():
        ref = r32._mel2hidden(r32.mel_extractor(wav[None], center=True))[0].float()
        half = r16._mel2hidden(r16.mel_extractor(wav[None], center=True))[0].float()
    got = hip.salience(wav)
    assert got.shape == (T, 360) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    e_hip, e_half = float((got - ref).abs().max()), float((half - ref).abs().max())
    r_hip, r_half = float((got - ref).pow(2).mean().sqrt()), float((half - ref).pow(2).mean().sqrt())
    print("salience n=%d: HIP max %.3g rms %.3g | torch .half() max %.3g rms %.3g" % (n, e_hip, r_hip, e_half, r_half))
    assert e_half > 0 and e_hip <= e_half and r_hip <= r_half
    assert float(ref.max()) - float(ref.min()) > 0.05, "the seeded network's salience is flat: the comparison would see nothing"
    m = hip.mel(wav)
    assert m.shape == (1, rc.pad32(T), 128) and float(m[0, T:].abs().max() if T < m.shape[1] else 0) == 0
    assert torch.equal(hip.salience(wav), got)


def test_f0_is_the_decode_of_its_own_salience(gpu):
    import rvc_amd

    hip = rvc_amd.RMVPEHIP.from_reference(_standin(True))
    wav = _wav(48077).to(gpu)
    sal = hip.salience(wav)
    for key in (0, 1.5):
        pitch, pitchf = hip.f0(wav, 300, key)
        want = rvc_amd.glue.rmvpe_f0(sal, 300, key, 0.03)
        assert pitch.shape == (1, 300) and pitch.dtype == torch.int64 and torch.equal(pitch, want[0]) and torch.equal(pitchf, want[1])
    with pytest.raises(rvc_amd.RvcmiError):
        hip.f0(wav.cpu(), 300, 0)            # CPU input: no fallback
    with pytest.raises(rvc_amd.RvcmiError):
        hip.salience(wav[:400])              # shorter than the reflection pad


def test_unsupported_objects_give_none_and_stay_untouched(gpu):
    import rvc_amd

    def untouched(r, fn):
        mods = [(n, id(m)) for n, m in r.model.named_modules()] if isinstance(r.model, torch.nn.Module) else None
        keys = set(vars(r))
        out = fn()
        assert set(vars(r)) == keys and (mods is None or mods == [(n, id(m)) for n, m in r.model.named_modules()])
        return out

    ok = _standin(True)
    assert untouched(ok, lambda: rvc_amd.RMVPEHIP.from_reference(ok)) is not None     # the supported one is not mutated either
    assert isinstance(ok.model.fc[0].gru, torch.nn.GRU) and not isinstance(ok.model.unet, rvc_amd.UNetHIP)
    small = rc.uc.key_list(2, 1, 1, 16)
    odd_gru = rc.RmvpeStandIn(gpu, True, model=rc.E2EStandIn(keys=small, gru_hidden=128))
    assert untouched(odd_gru, lambda: rvc_amd.RMVPEHIP.from_reference(odd_gru)) is None
    odd_unet = rc.RmvpeStandIn(gpu, True, model=rc.E2EStandIn(keys=rc.uc.key_list(2, 1, 1, 24)))
    assert untouched(odd_unet, lambda: rvc_amd.RMVPEHIP.from_reference(odd_unet)) is None
    odd_mel = rc.RmvpeStandIn(gpu, True, model=rc.E2EStandIn(keys=small))
    odd_mel.mel_extractor.mel_basis = torch.rand(80, 513, device=gpu)
    assert untouched(odd_mel, lambda: rvc_amd.RMVPEHIP.from_reference(odd_mel)) is None
    cpu = rc.RmvpeStandIn(torch.device("cpu"), False, model=rc.E2EStandIn(keys=small))
    assert untouched(cpu, lambda: rvc_amd.RMVPEHIP.from_reference(cpu)) is None
    onnx = types.SimpleNamespace(device="privateuseone:0", is_half=False, mel_extractor=rc.MelStandIn(False), model=object())
    assert untouched(onnx, lambda: rvc_amd.RMVPEHIP.from_reference(onnx)) is None
    reduced = rc.RmvpeStandIn(gpu, True, model=rc.E2EStandIn(keys=small))            # another U-Net geometry the kernels DO serve
    assert untouched(reduced, lambda: rvc_amd.RMVPEHIP.from_reference(reduced)) is not None


class _Raises:
    def __init__(self, inner=None):
        for k in ("n_fft", "hop_length", "win_length", "clamp", "mel_basis", "is_half"):
            if inner is not None:
                setattr(self, k, getattr(inner, k))

    def __call__(self, *a, **k):
        raise AssertionError("the torch path was called")


def test_switch_routes_the_f0_step(gpu, monkeypatch):
    import rvc_amd
    import rvc_amd.pipeline as rp

    monkeypatch.delenv("RVCMI_RMVPE_GRU", raising=False)
    monkeypatch.delenv("RVCMI_RMVPE_UNET", raising=False)
    r = rc.RmvpeStandIn(gpu, True)
    me = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=r, is_half=True, device=gpu))
    wav = _wav(5120).to(gpu)
    hip = rvc_amd.RMVPEHIP.from_reference(r)
    want = hip.f0(wav, 32, 2)
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "0")
    off = rp._rmvpe_on_device(me, wav, 32, 2)                 # off: the old way, through the object's own mel extractor and network
    assert r.mel_extractor.calls == 1 and r.hidden_calls == 1 and not hasattr(me.f0_gen, "_rvcmi_rmvpe_hip")
    assert off[0].shape == want[0].shape
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "1")
    mel, r.mel_extractor, r._mel2hidden = r.mel_extractor, _Raises(r.mel_extractor), _Raises()
    on = rp._rmvpe_on_device(me, wav, 32, 2)
    assert torch.equal(on[0], want[0]) and torch.equal(on[1], want[1])
    assert me.f0_gen._rvcmi_rmvpe_hip[0] is r and rp._rmvpe_on_device(me, wav.cpu().numpy(), 32, 2)[0].shape == (1, 32)
    frac = rp._rmvpe_on_device(me, wav, 32, 1.5)
    assert torch.equal(frac[0], hip.f0(wav, 32, 1.5)[0])
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "0")
    with pytest.raises(AssertionError, match="the torch path was called"):
        rp._rmvpe_on_device(me, wav, 32, 2)
    r.mel_extractor = mel


def test_realtime_entry_keeps_a_fractional_key_on_the_device(gpu, monkeypatch):
    """``rvc_infer_hip`` with ``formant_shift = 0.5`` (key 1.5): with the switch on no ``_get_f0`` call, and the decoder receives the f0 of key
    1.5; with the switch off the object's own estimator, as before."""
    import rvc_amd
    from oracle import synth
    from rvc_amd.realtime import f0_extractor_frame, rvc_infer_hip

    monkeypatch.delenv("RVCMI_RT_GRAPH", raising=False)
    seen, host_calls = {}, []

    class Net:
        def infer(self, phone, lengths, sid, pitch=None, pitchf=None, skip_head=None, return_length=None, return_length2=None):
            seen.update(pitch=pitch.cpu(), pitchf=pitchf.cpu())
            return torch.zeros(1, 1, (return_length2 or return_length) * 480, device=phone.device)

    block16k, win, n_in = 4096, 160, 160 * 118
    r = rc.RmvpeStandIn(gpu, True)  # (its own: the switched-off call below swaps the network's GRU in place, as it always has)

    def host_f0(x, key, method="rmvpe"):
        host_calls.append(float(key))
        m = int(x.shape[0]) // win
        pf = synth.make_f0(1, m)[0]
        return synth.make_pitch(pf[None])[0].to(gpu), pf.to(gpu)

    me = types.SimpleNamespace(index=None, net_g=Net(), index_rate=0.0, device=gpu, if_f0=1, tgt_sr=48000, f0_up_key=2, formant_shift=0.5, window=win,
                               is_half=False, version="v2", hubert=synth.FakeHubert(768, 5), f0_gen=types.SimpleNamespace(rmvpe=r, is_half=True, device=gpu),
                               _get_f0=host_f0)
    wav_in = torch.from_numpy(synth.make_audio16k(n_in, 3)).to(gpu)
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "1")
    out = rvc_infer_hip(me, wav_in, block16k, 40, 25, "rmvpe", 1.0)
    assert out.shape == (25 * 480,) and host_calls == []
    n = f0_extractor_frame(block16k, "rmvpe", win)
    m = n // win
    pitch, pitchf = rvc_amd.RMVPEHIP.from_reference(r).f0(wav_in[-n:], m, 1.5)
    p_len = n_in // win
    assert torch.equal(seen["pitch"][0, p_len - (m - 4):], pitch[0, 3:-1].cpu())
    rl2 = int(np.ceil(25 * pow(2, 0.5 / 12)))  # rtrvc.py:190-191, 218-219: with a formant shift the decoder's pitchf is (pitchf * return_length2) / return_length
    assert rl2 == 26
    assert torch.allclose(seen["pitchf"][0, p_len - (m - 4):], pitchf[0, 3:-1].cpu() * rl2 / 25, rtol=1e-6, atol=0)
    whole = rvc_amd.RMVPEHIP.from_reference(r).f0(wav_in[-n:], m, 1)
    assert not torch.equal(whole[1], pitchf) or float(pitchf.max()) == 0, "key 1.5 and key 1 must differ where anything is voiced"
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "0")
    rvc_infer_hip(me, wav_in, block16k, 40, 25, "rmvpe", 1.0)
    assert host_calls == [1.5]


def test_realtime_f0_graph_replay_equals_eager(gpu, monkeypatch):
    """``realtime._rmvpe_f0_graphed`` with the switch on: captured once after the eager warm-up blocks, the replay bit-equal to the eager chain,
    for an integer and for a fractional key (each its own graph: the key's factor is baked in)."""
    import rvc_amd.pipeline as rp
    from rvc_amd import realtime as rt

    monkeypatch.delenv("RVCMI_RT_GRAPH", raising=False)
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "1")
    n = rt.f0_extractor_frame(4096, "rmvpe", 160)
    p_len = n // 160
    r = rc.RmvpeStandIn(gpu, True)
    r.mel_extractor, r._mel2hidden = _Raises(r.mel_extractor), _Raises()
    me = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=r, is_half=True, device=gpu))
    g = torch.Generator().manual_seed(1)
    for key in (0, 1.5):
        for i in range(rt.RT_GRAPH_AFTER + 1):
            wav = (0.1 * (i + 1) * torch.randn(n, generator=g) + _wav(n, i)).to(gpu)
            pitch, pitchf = rt._rmvpe_f0_graphed(me, wav, p_len, key)
            pitch, pitchf = pitch.clone(), pitchf.clone()
            entry = me._rvcmi_f0_graphs[(n, p_len, key, str(wav.device))]
            assert ("graph" in entry) == (i >= rt.RT_GRAPH_AFTER - 1), (key, i, list(entry))
            want = rp._rmvpe_on_device(me, wav, p_len, key)
            assert torch.equal(pitch, want[0]) and torch.equal(pitchf, want[1]), "key %s block %d: the replay differs from the eager chain" % (key, i)
    assert len(me._rvcmi_f0_graphs) == 2
