"""k_rb_stream's lean-K-loop instantiations (C = 128, whole resblocks, 192-row steps) run their K loops on v_mfma_f32_16x16x32 (csrc/mfma_conv.hpp
kconv16, csrc/rb_stream_kernels.hpp SH = 16, option RS_MFMA = 16 / 32).  The hardware then sums 32 products per instruction instead of 16: a permuted
summation order of the K loop, the liberty tests/nsf_cases.py derived the MFMA layers' bars for (FACTOR 4) -- so the stage is held to the SAME bars against
the layer oracle, and everything that only changes what the new path executes (fill skip, strips, batch) is held to bit-equality inside it.

All cases are v2_48k with RB_STREAM = 1, RS_SMALL = 1, RS_KL = 2.  T = 24 is 2 880 rows at stage 1 (strips of several steps), T = 1, 2, 3 are single
strips of one step that starts in front of the sequence (r0 < 0).  Which shape ran is REPORTED by the forward whose output is compared
(``gen.last_plan()``: ``stream_mfma``).
"""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nsf_cases as nc  # noqa: E402

gpu_test = pytest.mark.gpu

LEAN = dict(RB_STREAM=1, RS_SMALL=1, RS_KL=2)
LAYERS = ("stage1", "post")  # the stage the kernel computes, and the waveform (conv_post's oracle on the device's last stage)


def _case(T, seed, operand="fp16", B=1, **opts):
    return nc.Case("v2_48k", B, T, seed, nc.O(**LEAN, **opts), operand, layers=LAYERS, want=((1, "STREAM"),))


def _runner(c, gen, gpu):
    x = nc.inputs(c)
    args = (x["z"].to(gpu), x["f0"].to(gpu), x["g"].to(gpu))
    noise = x["noise"].to(gpu)
    return (lambda: gen(*args, noise=noise).cpu()), (lambda what: gen.debug_tap(what, *args, noise=noise))


def _shape_and_plan(gen, run):
    """-> (the MFMA shape stage 1's launch ran on, its (k, strips, strip length) per resblock, the waveform) of ONE plain forward, as it reports itself"""
    wave = run()
    r = gen.last_plan()[1]
    assert (r["path"], r["C"], r["stream_nj"], r["n_rb"]) == ("STREAM", 128, 6, 3), r
    return r["stream_mfma"], tuple(sorted(zip(r["k"], r["tiles"], r["strip_len"]))), wave


@functools.lru_cache(maxsize=None)
def _device_case(c, gpu):
    """device_case once per case: its record (every layer of LAYERS against the oracle at the derived bars), waveform and handle"""
    return nc.device_case(c, torch.device(gpu))


def _within_bars(c, gpu):
    rec, wave, gen = _device_case(c, str(gpu))
    for r in rec["layers"]:
        print("%s %s: rms %.3e (bar %.3e, floor %.3e)  max %.3e (bar %.3e, floor %.3e)" % (
            rec["case"], r["layer"], r["rms"], r["bar_rms"], r["floor_rms"], r["max"], r["bar_max"], r["floor_max"]))
    run, _ = _runner(c, gen, gpu)
    assert rec["plan"][1]["stream_mfma"] == 16, rec["plan"][1]  # (reported by the forward device_case compared)
    shape, _, wave_s = _shape_and_plan(gen, run)
    assert shape == 16, shape
    assert torch.equal(wave_s, wave)
    assert {r["layer"] for r in rec["layers"]} == set(LAYERS)
    for r in rec["layers"]:
        assert r["within_bars"], r
    return rec, wave, gen, run


@gpu_test
@pytest.mark.parametrize("T", (24, 1, 2, 3))
def test_stage1_and_waveform_within_bars(T, gpu):
    _within_bars(_case(T, 400 + T), gpu)


@gpu_test
def test_bf16_within_bars(gpu):
    _within_bars(_case(24, 430, "bf16"), gpu)


@gpu_test
def test_fp32_rows_within_bars(gpu):
    """X0_F16_NOSTREAM = 1: X0 stays fp32, the instantiation whose step IO moves fp32 rows"""
    _within_bars(_case(24, 431, X0_F16_NOSTREAM=1), gpu)


@gpu_test
def test_fp32_streams_within_bars(gpu):
    _within_bars(_case(24, 432, Y_F16=0), gpu)


@gpu_test
@pytest.mark.parametrize("T", (24, 2))
def test_fill_skip_same_bits(T, gpu):
    """RS_FILL = 0 (every tile of a strip's first step) against the default, both on the 16x16x32 shape; and a second call"""
    c = _case(T, 400 + T)
    _, wave, gen, run = _within_bars(c, gpu)
    _, tap = _runner(c, gen, gpu)
    s1 = tap("stage1")
    gen.set_option("RS_FILL", 0)
    try:
        shape, _, wave0 = _shape_and_plan(gen, run)
        s10 = tap("stage1")
    finally:
        gen.set_option("RS_FILL", None)
    assert shape == 16
    assert torch.equal(wave0, wave) and torch.equal(s10, s1)
    assert torch.equal(run(), wave) and torch.equal(tap("stage1"), s1)


@gpu_test
def test_stamped_forward_same_bits(gpu):
    """RS_STAMPS = 1 (dev: the kernel's stamped branch, a synchronisation and a printed breakdown per launch) leaves every bit of the output alone"""
    _, wave, gen, run = _within_bars(_case(2, 402), gpu)
    gen.set_option("RS_STAMPS", 1)
    try:
        stamped = run()
    finally:
        gen.set_option("RS_STAMPS", None)
    assert torch.equal(stamped, wave)


@gpu_test
def test_ragged_batch_items_equal_single_calls(gpu):
    """B = 2 with lengths (24, 5): each item bit-equal to its own single call (5 frames = 600 rows at stage 1: one strip)"""
    import rvc_amd

    c = _case(24, 433, B=2)
    cfg, x, w = nc.CONFIGS[c.cfg], nc.inputs(c), nc.weights(c.cfg, c.seed, c.wgain)
    gen = rvc_amd.NSFGeneratorHIP(vars(cfg), w, device=gpu, operand=c.operand, max_B=c.B, max_T=c.T)
    for k, v in c.opts:
        gen.set_option(k, v)
    lengths = (24, 5)
    z, f0, g, noise = x["z"].to(gpu).clone(), x["f0"].to(gpu), x["g"].to(gpu), x["noise"].to(gpu)
    for b, n in enumerate(lengths):
        z[b, :, n:] = 0
    run = lambda: gen(z, f0, g, noise=noise, lengths=torch.tensor(lengths)).cpu()
    shape, _, out = _shape_and_plan(gen, run)
    assert shape == 16 and out.shape == (2, 1, 24 * cfg.upp) and bool(torch.isfinite(out).all())
    for b, n in enumerate(lengths):
        one = gen(z[b:b + 1, :, :n].contiguous(), f0[b:b + 1, :n].contiguous(), g[b:b + 1], noise=noise[b:b + 1, :n * cfg.upp].contiguous()).cpu()
        assert one.abs().max() > 0
        assert torch.equal(out[b, 0, :n * cfg.upp], one[0, 0]), "item %d differs from its single call, max %.3e" % (b, nc.err(out[b, 0, :n * cfg.upp], one[0, 0])[1])
        assert not out[b, 0, n * cfg.upp:].any()


@gpu_test
def test_other_plans_same_bits(gpu):
    """RS_C0 = 2.0 / 3.8 / 6.0 at B = 16, T = 18 plan different strips (as each forward reports them, as in tests/test_gpu_rb_stream_fill.py);
    the rows they produce on the 16x16x32 shape are the same bits"""
    import rvc_amd

    c = _case(18, 434, B=16)
    cfg, w = nc.CONFIGS[c.cfg], nc.weights(c.cfg, c.seed, c.wgain)
    gen = rvc_amd.NSFGeneratorHIP(vars(cfg), w, device=gpu, operand=c.operand, max_B=c.B, max_T=c.T)
    for k, v in c.opts:
        gen.set_option(k, v)
    run, tap = _runner(c, gen, gpu)
    outs, plans = [], []
    for c0 in (2.0, 3.8, 6.0):
        gen.set_option("RS_C0", c0)
        shape, plan, wave = _shape_and_plan(gen, run)
        assert shape == 16
        plans.append(plan)
        outs.append((wave, tap("stage1")))
    gen.set_option("RS_C0", None)
    assert len(set(plans)) == 3, plans
    assert bool(torch.isfinite(outs[0][0]).all()) and outs[0][0].abs().max() > 0
    for wave, s1 in outs[1:]:
        assert torch.equal(wave, outs[0][0]) and torch.equal(s1, outs[0][1])


@gpu_test
def test_rs_mfma_32_is_the_other_path_and_agrees(gpu):
    """RS_MFMA = 32 on the same handle runs the 32x32x16 instantiation; its stage-1 tap and the 16x16x32 one differ by no more than the stage's bar
    (they need be neither equal nor different bits: the two shapes sum the same products in another order)"""
    c = _case(24, 424)
    rec, wave, gen, run = _within_bars(c, gpu)
    _, tap = _runner(c, gen, gpu)
    s16 = tap("stage1")
    gen.set_option("RS_MFMA", 32)
    try:
        shape, _, wave32 = _shape_and_plan(gen, run)
        s32 = tap("stage1")
    finally:
        gen.set_option("RS_MFMA", None)
    assert shape == 32
    assert bool(torch.isfinite(s32).all()) and bool(torch.isfinite(wave32).all())
    bar = next(r for r in rec["layers"] if r["layer"] == "stage1")
    rms, mx = nc.err(s32, s16)
    print("stage1, RS_MFMA = 32 against 16: rms %.3e (bar %.3e)  max %.3e (bar %.3e)" % (rms, bar["bar_rms"], mx, bar["bar_max"]))
    assert rms <= bar["bar_rms"] and mx <= bar["bar_max"]
    shape, _, again = _shape_and_plan(gen, run)
    assert shape == 16 and torch.equal(again, wave)  # (the default is back)


@gpu_test
def test_refused_option_value_leaves_the_default(gpu):
    c = _case(24, 424)
    _, wave, gen, run = _within_bars(c, gpu)
    for bad in (8, 0, 64, 16.5):
        with pytest.raises(Exception):
            gen.set_option("RS_MFMA", bad)
    shape, _, again = _shape_and_plan(gen, run)
    assert shape == 16 and torch.equal(again, wave)
    gen.set_option("RS_MFMA", 16)  # (the accepted values)
    gen.set_option("RS_MFMA", None)
