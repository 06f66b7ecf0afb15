"""k_rb_stream (csrc/rb_stream_kernels.hpp) skips, in a strip's FIRST step, the leading column tiles of every conv that only fill the pipeline: their
rows lie in front of everything the strip stores and of every later pair's halo.  That changes what the kernel executes, not what it computes, so every
GPU check here is BIT-equality of two code paths on the same device, inputs and handle: option RS_FILL = 0 (every tile, as in every later step) against
the default, and plans with other strip boundaries (RS_C0) against each other.  A row's value does not depend on the strip or step that produced it.

All cases are v2_48k (k = 3, 7, 11 with dilations 1, 3, 5 in every stage).  With RB_STREAM = 1, T = 24 is 2 880 rows at stage 1 (C = 128, whole
resblocks: up to 15 strips of two steps per resblock) and 288 rows at stage 0 (C = 256, the pair-level form of the same kernel); T = 2 is 240 rows at
stage 1: one strip whose first step is its only one and starts in front of the sequence (r0 < 0).

Not tested, on purpose: inputs that saturate fp16 to inf inside a skipped tile.  A skipped tile's values are never read.

The one CPU test holds the first-tile table (tools/model_rb_stream.py fill_tile, the arithmetic of rs_fill_tile) against a brute-force walk of which
rows a stored row depends on.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import nsf_cases as nc  # noqa: E402

gpu_test = pytest.mark.gpu


def _gen(c, gpu, lengths=None):
    import rvc_amd

    cfg, x, w = nc.CONFIGS[c.cfg], nc.inputs(c), nc.weights(c.cfg, c.seed, c.wgain)
    gen = rvc_amd.NSFGeneratorHIP(vars(cfg), w, device=gpu, operand=c.operand, max_B=c.B, max_T=c.T)
    for k, v in c.opts:
        gen.set_option(k, v)
    z = x["z"].to(gpu).clone()
    kw = {"noise": x["noise"].to(gpu)}
    if lengths is not None:
        for b, n in enumerate(lengths):
            z[b, :, n:] = 0
        kw["lengths"] = torch.tensor(lengths)
    args = (z, x["f0"].to(gpu), x["g"].to(gpu))
    return gen, (lambda: gen(*args, **kw).cpu()), (lambda what: gen.debug_tap(what, *args, noise=kw["noise"]))


def _skip_equals_no_skip(gen, run, taps=()):
    """-> the default's outputs, after asserting that RS_FILL = 0 gives the same bits"""
    got = {"wave": run(), **{t: taps[t]() for t in taps}}
    gen.set_option("RS_FILL", 0)
    want = {"wave": run(), **{t: taps[t]() for t in taps}}
    gen.set_option("RS_FILL", None)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()) and got[k].abs().max() > 0
        assert torch.equal(got[k], want[k]), "%s: skipping the fill tiles changed the result, max %.3e" % (k, nc.err(got[k], want[k])[1])
    assert torch.equal(run(), got["wave"])  # (the default is back)
    return got


def _names(gen, run):
    gen.profile(True)
    run()
    names = {s["name"] for s in gen.profile_read()}
    gen.profile(False)
    return names


@gpu_test
@pytest.mark.parametrize("small", (1, 0))
@pytest.mark.parametrize("T", (24, 2))
def test_skip_equals_no_skip(T, small, gpu):
    """T = 24: several strips of few steps; T = 2: the first step is the only one and r0 < 0.  RS_SMALL = 1: steps of 192 rows and the lean K loop
    (kconv); RS_SMALL = 0: steps of 256 rows and the ring K loop (conv_run)"""
    c = nc.Case("v2_48k", 1, T, 300 + 2 * T + small, nc.O(RB_STREAM=1, RS_SMALL=small))
    gen, run, tap = _gen(c, gpu)
    assert "rb_stream_c128" in _names(gen, run)
    _skip_equals_no_skip(gen, run)


@gpu_test
def test_skip_equals_no_skip_stage1_tap(gpu):
    c = nc.Case("v2_48k", 1, 24, 310, nc.STREAM)
    gen, run, tap = _gen(c, gpu)
    _skip_equals_no_skip(gen, run, {"stage1": lambda: tap("stage1")})


@gpu_test
def test_skip_equals_no_skip_ragged_batch(gpu):
    """B = 2 with lengths (24, 5): item 1 ends inside the first strips, its later strips hold no row"""
    c = nc.Case("v2_48k", 2, 24, 311, nc.STREAM)
    gen, run, _ = _gen(c, gpu, lengths=(24, 5))
    out = _skip_equals_no_skip(gen, run)["wave"]
    upp = nc.CONFIGS[c.cfg].upp
    assert out.shape == (2, 1, 24 * upp) and not out[1, 0, 5 * upp:].any()


@gpu_test
def test_skip_equals_no_skip_bf16(gpu):
    c = nc.Case("v2_48k", 1, 24, 312, nc.STREAM, "bf16")
    gen, run, _ = _gen(c, gpu)
    _skip_equals_no_skip(gen, run)


@gpu_test
def test_other_plans_same_bits(gpu):
    """RS_C0 moves the strip boundaries, hence the first steps; the planning constant must not show in a single bit.  At T = 24 and B = 1 the grid
    has more slots than strips worth cutting and every RS_C0 plans the same strips, so this case is B = 16, T = 18 (2 160 rows per item, 16 slots per
    item on 256 CUs), where RS_C0 = 2.0 / 3.8 / 6.0 plan 10 + 4 + 2 / 6 + 4 + 5 / 6 + 5 + 5 strips of 2 to 7 steps.  That the plans differ is
    REPORTED: the strips and strip lengths of the very forwards that are compared (``gen.last_plan()``)."""
    c = nc.Case("v2_48k", 16, 18, 313, nc.STREAM)
    gen, run, tap = _gen(c, gpu)
    outs, plans = [], []
    for c0 in (2.0, 3.8, 6.0):
        gen.set_option("RS_C0", c0)
        wave = run()
        r = gen.last_plan()[1]
        assert (r["path"], r["C"], r["n_rb"]) == ("STREAM", 128, 3), r
        plans.append(tuple(sorted(zip(r["k"], r["tiles"], r["strip_len"]))))
        outs.append((wave, tap("stage1")))
    gen.set_option("RS_C0", None)
    assert len(set(plans)) == 3, plans
    assert bool(torch.isfinite(outs[0][0]).all()) and outs[0][0].abs().max() > 0
    for wave, s1 in outs[1:]:
        assert torch.equal(wave, outs[0][0]) and torch.equal(s1, outs[0][1])
    _skip_equals_no_skip(gen, run)


@gpu_test
def test_stamped_forward_same_bits(gpu):
    """RS_STAMPS = 1 (dev: the kernel's stamped branch, a synchronisation and a printed breakdown per launch) at T = 2 leaves every bit alone"""
    c = nc.Case("v2_48k", 1, 2, 315, nc.STREAM)
    gen, run, _ = _gen(c, gpu)
    wave = run()
    assert gen.last_plan()[1]["path"] == "STREAM"
    gen.set_option("RS_STAMPS", 1)
    try:
        stamped = run()
    finally:
        gen.set_option("RS_STAMPS", None)
    assert bool(torch.isfinite(wave).all()) and wave.abs().max() > 0 and torch.equal(stamped, wave)


@gpu_test
def test_pair_level_c256_skip_equals_no_skip(gpu):
    """stage 0 (C = 256) through the pair-level form of the kernel (ND = 1).  That form measured no gain from the skip and is built without it (DESIGN.md
    4.2), so what this holds is that RS_FILL leaves the pair level alone while stage 1 behind it skips"""
    c = nc.Case("v2_48k", 1, 24, 314, nc.STREAM)
    gen, run, tap = _gen(c, gpu)
    names = _names(gen, run)
    assert "rb_stream1_c256" in names, sorted(names)
    _skip_equals_no_skip(gen, run, {"stage0": lambda: tap("stage0")})


def test_fill_tile_table_against_brute_force():
    """fill_tile == the first tile of the step-0 window holding a row that a stored row depends on (walked tap by tap), for every pair and conv of
    k = 3, 7, 11 x dilations (1, 3, 5), each dilation alone (the pair-level form), and a strip at S0 = 0 (r0 < 0), where the rows in front of the sequence
    -- masked to zero whatever was computed -- may only move the first needed tile BACK, never forward"""
    import model_rb_stream as model

    for k in (3, 7, 11):
        for dils in ((1, 3, 5), (1,), (3,), (5,)):
            for NJ in (6, 8, 3, 4):
                for m in range(len(dils)):
                    for conv2 in (0, 1):
                        jt0 = model.fill_tile(k, list(dils), m, conv2)
                        for S0, S1 in ((0, 400), (960, 1500), (4097, 4129)):
                            assert min(jt0, NJ) == model.fill_tile_brute(k, list(dils), m, conv2, S0, S1, NJ), (k, dils, m, conv2, S0)  # (NJ: no tile of the window)
                        assert min(jt0, NJ) <= model.fill_tile_brute(k, list(dils), m, conv2, 0, 400, NJ, nonneg=True)
                        assert jt0 >= m + 1  # (the 32-row lag alone: what the kernel's smallest instantiation per pair relies on)
    # the table of the three resblocks of v2_48k: 14 / 13 / 12 conv-tiles of a first step's 36
    table = {k: [[model.fill_tile(k, [1, 3, 5], m, c) for c in (0, 1)] for m in range(3)] for k in (11, 7, 3)}
    assert table == {11: [[1, 1], [2, 2], [4, 4]], 7: [[1, 1], [2, 2], [3, 4]], 3: [[1, 1], [2, 2], [3, 3]]}, table
