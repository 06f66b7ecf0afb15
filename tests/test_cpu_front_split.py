"""The front's ``"fp16x2"`` operand mode on the CPU: the arithmetic (tests/front_split_cases.py restates
csrc/front_split_kernels.hpp on the oracle), the (hi, lo') split itself (csrc/split_f16.hpp, through a stand-alone C++ program built
with -fsanitize=address,undefined; nothing of it is loaded into Python), and the parts of the Python interface that need no GPU."""
import os
import subprocess

import numpy as np
import pytest
import torch

import front_split_cases as fs
from oracle import front_oracle, synth
from oracle.front_oracle import FrontConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_fp16x2_is_fp32_grade_on_T100():
    """T = 100, seed 1234, against the fp64 run of the oracle: the emulated fp16x2 z error is at most 8 times the fp32 oracle's own
    error and at least 100 times below the emulated fp16-operand error (today's arithmetic)."""
    cfg = FrontConfig()
    w = synth.make_front_weights(cfg, 1234)
    T = 100
    phone = synth.make_phone(1, T, 768, 1234)
    pitch = synth.make_pitch(synth.make_f0(1, T))
    lengths, sid = torch.tensor([T]), torch.tensor([0])
    nz = torch.randn(1, 192, T, generator=torch.Generator().manual_seed(8))
    args = (cfg, w, phone, pitch, lengths, sid, nz)
    z64 = fs.run_front("fp32", *args, dtype=torch.float64)
    e32 = fs.rms(fs.run_front("fp32", *args), z64)
    e16 = fs.rms(fs.run_front("fp16", *args), z64)
    e2 = fs.rms(fs.run_front("fp16x2", *args), z64)
    print("z RMS against the fp64 oracle: fp32 %.3e, fp16 operands %.3e, fp16x2 %.3e (%.2f x fp32, fp16 / fp16x2 = %.0f)"
          % (e32, e16, e2, e2 / e32, e16 / e2))
    assert 1e-7 < e32 < 1e-5, e32
    assert e2 <= 8 * e32, "emulated fp16x2: %.3e against fp32's %.3e" % (e2, e32)
    assert e2 * 100 <= e16, "emulated fp16x2 %.3e is not 100 x below fp16 operands' %.3e" % (e2, e16)


def test_emulate_restores_the_oracle_even_when_the_block_raises():
    F0, att0 = front_oracle.F, front_oracle.attention
    with pytest.raises(RuntimeError):
        with fs.emulate("fp16x2", {}):
            assert front_oracle.F is not F0 and front_oracle.attention is not att0
            raise RuntimeError("inside")
    assert front_oracle.F is F0 and front_oracle.attention is att0
    with fs.emulate("fp32", {}):
        assert front_oracle.F is F0
    assert front_oracle.F is F0 and front_oracle.attention is att0


def _split_cases():
    g = torch.Generator().manual_seed(5)
    sweep = 0.03 + (torch.rand(4096, generator=g) - 0.5) * 0.03
    near = 6.103515625e-05 * (1.0 + (torch.rand(1024, generator=g) - 0.5))  # both sides of fp16's smallest normal number
    edge = torch.tensor([0.0, -0.0, 1.0, -1.0, 65504.0, -65504.0, 65503.99, 6.103515625e-05, -6.103515625e-05, 6.1e-5, 0.0300001, 3.14159265])
    return torch.cat([edge, sweep, -sweep, near, -near, torch.randn(4096, generator=g) * 3]).float()


def test_split_round_trip_is_within_2_to_minus_21():
    x = _split_cases()
    hi, lo = fs.split(x)
    assert torch.equal(hi, hi.half().float()) and torch.equal(lo, lo.half().float())  # both are fp16 values
    j = hi.double() + lo.double() / 2048.0
    normal = (x.abs() >= 6.103515625e-05) & (x.abs() <= 65504.0)
    rel = ((j - x.double()).abs() / x.double().abs().clamp_min(1e-30))[normal]
    assert float(rel.max()) <= 2.0 ** -21, float(rel.max())
    assert float((j - x.double()).abs()[~normal].max()) <= 2.0 ** -36  # zeros and subnormal hi: the rest is kept by lo'
    assert torch.equal(fs.join(hi, lo)[:2], torch.zeros(2)) and torch.signbit(hi[1])
    # plain fp16 rounding of the same values, for scale: about 2^-11
    assert float(((x.half().double() - x.double()).abs() / x.double().abs().clamp_min(1e-30))[normal].max()) > 2.0 ** -13


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("split_f16") / "split_f16_main")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "split_f16_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def test_host_split_selfcheck_under_sanitizers(prog):
    r = subprocess.run([prog, "selfcheck"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "selfcheck ok" in r.stdout, r.stdout


def test_host_split_equals_the_emulator_bit_for_bit(prog, tmp_path):
    """What the weight packers store (csrc/split_f16.hpp) is what the emulator computes with torch's fp16 rounding."""
    x = torch.cat([_split_cases(), torch.tensor([70000.0, -1e30, 1e-8, 2.0 ** -25, 2.0 ** -24 * 1.5])]).float()
    src, out = tmp_path / "x.f32", tmp_path / "pairs.bin"
    x.numpy().tofile(str(src))
    r = subprocess.run([prog, "split", str(src), str(out)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "split ok: %d values" % x.numel() in r.stdout, r.stdout
    rec = np.fromfile(str(out), dtype=np.dtype([("hi", "<u2"), ("lo", "<u2"), ("join", "<f4")]))
    hi, lo = fs.split(x)
    assert np.array_equal(rec["hi"], hi.half().numpy().view(np.uint16))
    assert np.array_equal(rec["lo"], lo.half().numpy().view(np.uint16))
    assert np.array_equal(rec["join"], fs.join(hi, lo).numpy())


def test_interface_without_a_gpu(monkeypatch):
    import rvc_amd
    from rvc_amd import _lib, synthesizer

    assert _lib.OPERANDS["fp16x2"] == 3
    hdr = open(os.path.join(ROOT, "include", "rvcmi.h")).read()
    assert "RVCMI_OPERAND_F16X2 = 3" in hdr
    cfg = FrontConfig()
    with pytest.raises(ValueError):  # there is still no fp32 front (checked before the device)
        rvc_amd.FrontHIP(vars(cfg), {}, device="cpu", operand="fp32")
    with pytest.raises(ValueError, match="front-only"):
        rvc_amd.NSFGeneratorHIP({}, {}, device="cpu", operand="fp16x2")
    monkeypatch.delenv("RVCMI_FRONT_OPERAND", raising=False)
    assert synthesizer.front_operand_choice(None) is None and synthesizer.FRONT_OPERAND is None  # default off
    assert synthesizer.front_operand_choice("fp16x2") == "fp16x2"
    monkeypatch.setenv("RVCMI_FRONT_OPERAND", "fp16x2")
    assert synthesizer.front_operand_choice(None) == "fp16x2"
    assert synthesizer.front_operand_choice("fp16") == "fp16"  # the argument wins
    monkeypatch.setenv("RVCMI_FRONT_OPERAND", "0")
    assert synthesizer.front_operand_choice(None) is None
    with pytest.raises(ValueError):
        synthesizer.front_operand_choice("fp32")
