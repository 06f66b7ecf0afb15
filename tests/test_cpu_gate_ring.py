"""The dirty-frame rule of the bank's noise reduction (csrc/gate_ring.hpp, exported as rvcmi_glue_gate_ring_plan and read by Python through
``glue.gate_ring_plan``) against a numpy brute force that compares the samples of every STFT frame before and after a roll, and the
host-only planner driven by a stand-alone C++ program (tests/host/gate_ring_main.cpp, built here with -fsanitize=address,undefined together
with csrc/error.cpp; nothing of it is loaded into Python)."""
import os
import subprocess

import numpy as np
import pytest

from rvc_amd import glue, stream_geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "retrieval-based-voice-conversion-webui_amd", "csrc")

GEOMETRIES = [(8, 2), (8, 3), (16, 4), (64, 16), (12, 5), (20, 20), (10, 1)]


def frames(x: np.ndarray, n_fft: int, hop: int) -> np.ndarray:
    """The samples of the 1 + L // hop frames of torch.stft(center=True, zero padding): [F, n_fft]."""
    xp = np.concatenate([np.zeros(n_fft // 2), x, np.zeros(n_fft // 2)])
    return np.stack([xp[f * hop: f * hop + n_fft] for f in range(1 + len(x) // hop)])


def changed_frames(n_fft, hop, L, shift, tail, rng):
    """Roll a buffer of L non-zero samples left by ``shift``, rewrite its last ``tail`` samples; frame f CHANGED when its samples differ
    from those of frame f + shift / hop before the roll (the frame whose ring slot it inherits), or when there is no such frame."""
    before = rng.uniform(1.0, 2.0, L)
    after = before.copy()
    if shift > 0:
        after[: max(L - shift, 0)] = before[shift:]
    t = min(max(tail, shift), L)
    if t > 0:
        after[L - t:] = rng.uniform(3.0, 4.0, t)
    fb, fa = frames(before, n_fft, hop), frames(after, n_fft, hop)
    F = fa.shape[0]
    if shift % hop:
        return np.ones(F, dtype=bool)   # no frame of the previous call starts where this one does
    d = shift // hop
    return np.array([f + d >= F or not np.array_equal(fa[f], fb[f + d]) for f in range(F)])


def dirty(plan) -> np.ndarray:
    f = np.arange(plan["Fn"])
    return (f < plan["head"]) | (f >= plan["back"])


def lengths(n_fft, hop):
    """Every L from n_fft / 2 + 1 to 40 hop + 1 where that is at most 120 values; else the lengths around the frame and hop edges and every
    k-th of the rest."""
    lo, hi = n_fft // 2 + 1, 40 * hop + 1
    if hi - lo < 120:
        return list(range(lo, hi + 1))
    edges = {lo, lo + 1, n_fft - 1, n_fft, n_fft + 1, n_fft + hop, 2 * n_fft + 3, 7 * hop, 7 * hop + 1, 23 * hop - 1, hi - 1, hi}
    return sorted((edges | set(range(lo, hi + 1, (hi - lo) // 60))) & set(range(lo, hi + 1)))


@pytest.mark.parametrize("n_fft, hop", GEOMETRIES)
def test_rule_against_brute_force(n_fft, hop):
    rng = np.random.default_rng(n_fft * 100 + hop)
    cases = 0
    for L in lengths(n_fft, hop):
        for shift in [0, hop, 2 * hop, 5 * hop, 30 * hop, 2 * hop + 1]:
            for extra in (0, hop, 2 * hop, 1):
                tail = shift + extra
                plan = glue.gate_ring_plan(L, n_fft, hop, shift, tail)
                assert plan["Fn"] == 1 + L // hop and plan["K"] == n_fft // 2 + 1
                d, c = dirty(plan), changed_frames(n_fft, hop, L, shift, tail, rng)
                assert plan["n_dirty"] == int(d.sum())
                assert not (c & ~d).any(), "a changed frame was called clean: %r" % ((n_fft, hop, L, shift, tail, plan),)
                if shift % hop == 0 and extra % hop == 0:
                    assert np.array_equal(c, d), "the rule is not the changed set: %r" % ((n_fft, hop, L, shift, tail, plan),)
                if shift % hop or tail > L:
                    assert d.all()
                assert plan["advance"] == (0 if d.all() else shift // hop)
                cases += 1
    assert cases >= 150


def test_every_unusable_shift_is_the_cold_arithmetic():
    for shift, tail in ((-16, 0), (-1, 5), (7, 7), (16, 641), (656, 656)):
        plan = glue.gate_ring_plan(640, 64, 16, shift, tail)
        assert plan["head"] == plan["back"] == plan["Fn"] == plan["n_dirty"] == 41 and plan["advance"] == 0


@pytest.mark.parametrize("sr", [48000, 44100, 40000])
def test_gui_geometries(sr):
    g = stream_geometry(sr)
    zc, blk, nn = g["zc"], g["block_frame"], g["input_wav_len"]
    plan = glue.gate_ring_plan(nn, 4 * zc, zc, blk, blk)
    assert (plan["Fn"], plan["n_dirty"], plan["advance"]) == (282, 29, blk // zc)
    assert glue.gate_ring_plan(nn, 4 * zc, zc, blk, blk + 2 * zc)["n_dirty"] == 31   # the host input gate rewrites 2 zc more


def test_refusals():
    from rvc_amd import _lib
    for nn, n_fft, hop in ((0, 8, 2), (100, 9, 2), (100, 4098, 16), (100, 8, 0), (100, 8, 9)):
        with pytest.raises(_lib.RvcmiError):
            glue.gate_ring_plan(nn, n_fft, hop, 0, 0)
    L = _lib.lib()
    assert L.rvcmi_glue_gate_ring_plan(100, 8, 2, 0, 0, None) == _lib.ERR_INVALID
    assert L.rvcmi_glue_spectral_gate_ring_bytes(0, 100, 8, 2) == 0 and L.rvcmi_glue_spectral_gate_ring_scratch_bytes(1, 100, 9, 2) == 0
    assert L.rvcmi_glue_spectral_gate_ring_bytes(64, 281 * 480, 1920, 480) == 64 * 282 * 961 * 16   # 4.3 MB per session and gate at 48 kHz


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gate_ring") / "gate_ring_main")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "gate_ring_main.cpp"), os.path.join(CSRC, "error.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("gate ring ok"), r.stdout
    return r.stdout


@pytest.mark.parametrize("case", ["gui plan", "gui plan, input gate on", "a tail shorter than the shift counts as the shift",
                                  "off-hop / negative shift, tail > nn, shift > nn: every frame dirty", "a buffer shorter than a frame: every frame dirty",
                                  "shift 0, tail 0: nothing dirty", "shift 0, tail 16: the back only", "dirty list", "ring slots follow the roll and wrap",
                                  "negative and huge bases", "ring bytes", "scratch layout", "refused: S = 0 / S too large", "refused: odd n_fft",
                                  "refused: n_fft > 4096", "refused: hop outside [1, n_fft]", "refused: empty signals", "refused: too many frames"])
def test_host_planner(out, case):
    assert "ok %s\n" % case in out, out


def test_the_header_is_host_only():
    src = open(os.path.join(CSRC, "gate_ring.hpp")).read()
    assert "hip/" not in src and '#include "common.hpp"' not in src
