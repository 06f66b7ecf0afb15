"""The RMVPE front end without a GPU: the fp64 oracle of tests/rmvpe_cases.py against the same lines in fp32 (what the reference executes),
the condition the GPU test sets shown to be one the reference's own path meets, the fixtures' own properties, and the host side of
``rvc_amd.rmvpe`` (the switch, the recogniser's refusals, the bindings)."""
import os
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import rmvpe_cases as rc  # noqa: E402


def test_bank_and_signals_are_what_the_tests_assume():
    b = rc.htk_bank()
    assert b.shape == (128, 513) and b.dtype == torch.float32 and float(b.min()) >= 0 and int((b.sum(1) == 0).sum()) == 0
    nz = b != 0
    first, last = nz.float().argmax(1), 512 - nz.flip(1).float().argmax(1)
    assert all(bool(nz[m, first[m]: last[m] + 1].all()) for m in range(128)), "a triangular filter is one contiguous band"
    assert int((last - first + 1).max()) < 64 and int(first[0]) >= 1 and int(last[-1]) >= 511   # 30 Hz .. 8000 Hz
    assert torch.equal(b, rc.htk_bank()) and not torch.equal(b, rc.htk_bank(seed=1))
    d = rc.dense_bank()
    assert d.shape == (128, 513) and float(d.min()) >= 0 and int((d == 0).sum()) < 8
    for n, T in zip(rc.LENGTHS, (4, 32, 33, 301)):
        assert n // rc.HOP + 1 == T
        x = rc.signal("voiced", n)
        assert x.dtype == torch.float32 and x.shape == (n,)
        z = rc.zero_frames(x)
        assert z.shape == (T,)
        if n >= 5037:
            assert int(z.sum()) >= 10 and not bool(z[0])
    assert float(rc.signal("quiet", 5120).abs().max()) < 1e-3 and rc.pad32(33) == 64 and rc.pad32(32) == 32
    h = torch.tensor([-1.0, -0.0, 0.0, 1.0, 1.0009765625], dtype=torch.float32)
    assert rc.half_ulps(h, h).tolist() == [0] * 5 and int(rc.half_ulps(h[3:4], h[4:5])) == 1 and int(rc.half_ulps(h[1:2], h[2:3])) == 0


@pytest.mark.parametrize("n", rc.LENGTHS)
def test_reference_fp32_path_is_within_one_fp16_ulp_of_the_oracle(n):
    """The GPU test's ``round_half`` condition, for the reference's own evaluation (fp32 on the CPU): no log-mel element more than one fp16 step
    from the fp64 oracle, the frames of the zero gap bit-equal to log(fp16(1e-5)); and the fp32 figures the measured bar is taken from."""
    bank = rc.htk_bank()
    floor = torch.log(torch.tensor(rc.CLAMP).half())
    for kind in ("voiced", "noise", "quiet"):
        x = rc.signal(kind, n)[None]
        want = rc.log_mel(x, bank, torch.float64, True)
        got = rc.log_mel(x, bank, torch.float32, True)
        assert want.dtype == got.dtype == torch.float16 and want.shape == (1, 128, n // rc.HOP + 1)
        u = rc.half_ulps(got, want)
        assert int(u.max()) <= 1, "%s n=%d: %d elements beyond one fp16 ulp" % (kind, n, int((u > 1).sum()))
        assert float((u > 0).float().mean()) < 1e-3
        if kind == "voiced":
            z = rc.zero_frames(x[0])
            assert torch.equal(got[0][:, z], floor.expand(128, int(z.sum()))) and torch.equal(want[0][:, z], floor.expand(128, int(z.sum())))
        e = float((rc.log_mel(x, bank, torch.float32, False).double() - rc.log_mel(x, bank, torch.float64, False)).abs().max())
        print("reference fp32 log-mel error, %s n=%d: %.3g" % (kind, n, e))
        assert 0 < e < 1e-3


def test_padded_layout_is_the_network_input():
    x = rc.signal("noise", 5120)[None]
    m = rc.log_mel(x, rc.htk_bank(), torch.float32, False)
    p = rc.padded_layout(m, 64)
    assert p.shape == (1, 64, 128) and torch.equal(p[0, :33], m[0].T) and float(p[0, 33:].abs().max()) == 0
    st = rc.MelStandIn(False)
    assert torch.equal(st(x, center=True), m) and st.calls == 1


def test_switch_follows_install_and_the_environment_overrides(monkeypatch):
    import rvc_amd.rmvpe as rr

    monkeypatch.delenv("RVCMI_RMVPE_HIP", raising=False)
    assert rr.rmvpe_on() is False                         # default: off
    monkeypatch.setattr(rr, "RMVPE_HIP", True)            # what install(rmvpe_hip=True) sets
    assert rr.rmvpe_on() is True
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "0")
    assert rr.rmvpe_on() is False
    monkeypatch.setattr(rr, "RMVPE_HIP", False)
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "1")
    assert rr.rmvpe_on() is True
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "yes")          # not 0 / 1: install's value
    assert rr.rmvpe_on() is False
    import inspect

    import rvc_amd

    assert inspect.signature(rvc_amd.install).parameters["rmvpe_hip"].default is False and rvc_amd.RMVPEHIP is rr.RMVPEHIP


def test_cpu_onnx_and_foreign_objects_are_left_alone():
    import rvc_amd

    small = rc.E2EStandIn(keys=rc.uc.key_list(2, 1, 1, 16))
    cpu = rc.RmvpeStandIn(torch.device("cpu"), False, model=small)
    before = {k: v.clone() for k, v in cpu.model.state_dict().items()}
    mods = [type(m) for m in cpu.model.modules()]
    assert rvc_amd.RMVPEHIP.from_reference(cpu) is None   # a CPU model: there is no CPU fallback, and nothing to swap
    assert [type(m) for m in cpu.model.modules()] == mods and all(torch.equal(v, before[k]) for k, v in cpu.model.state_dict().items())
    assert set(vars(cpu)) == {"device", "is_half", "mel_extractor", "model", "hidden_calls"}
    onnx = types.SimpleNamespace(device="privateuseone:0", is_half=False, mel_extractor=rc.MelStandIn(False), model=object())
    assert rvc_amd.RMVPEHIP.from_reference(onnx) is None
    session = types.SimpleNamespace(device="cuda:0", is_half=False, mel_extractor=rc.MelStandIn(False), model=object())  # not a torch module
    assert rvc_amd.RMVPEHIP.from_reference(session) is None
    assert rvc_amd.RMVPEHIP.from_reference(object()) is None
    other_mel = rc.RmvpeStandIn(torch.device("cpu"), False, model=small)
    other_mel.mel_extractor.n_fft = other_mel.mel_extractor.win_length = 2048
    assert rvc_amd.RMVPEHIP.from_reference(other_mel) is None


def test_bindings_cover_the_new_entry_points():
    from rvc_amd import _lib

    names = {s[0] for s in _lib.SYMBOLS}
    new = {"rvcmi_mel_create", "rvcmi_mel_destroy", "rvcmi_mel_frames", "rvcmi_mel_forward", "rvcmi_rmvpe_head", "rvcmi_glue_rmvpe_f0_key",
           "rvcmi_glue_f0_post_key"}
    assert new <= names and "rmvpe.hip" in _lib.SOURCES
    header = open(os.path.join(os.path.dirname(HERE), "include", "rvcmi.h")).read()
    L = _lib.lib()
    for n in new:
        assert n + "(" in header and hasattr(L, n)
    assert L.rvcmi_mel_frames(None, 5120) == 0             # no handle: no frames
