"""The checker of the generator's kernels checked (no GPU): oracle/nsf_layer_oracle.py is the reference's generator, and the per-layer bars
tests/nsf_cases.py derives from it tell the kernels' documented design from the layers that look like it.

  * With the operand rounding off, the layers composed are ``nsf_oracle.generator_forward`` and its taps: in float32 closer to it than its own distance
    to the float64 evaluation (measured: bit-equal but for the stage sums' division), for every config, without f0 too; and they reproduce the
    committed ``dec_*`` goldens (written by the real reference modules) to the 5e-6 max-abs tests/test_cpu_oracle.py holds nsf_oracle to.
  * The named wrong variants of a layer stand clear of that layer's bars (RMS or max-abs, whichever the defect shows in), each on the smallest
    stage that exercises it (that every OTHER layer stays inside its bars is checked end to end in the gap test below).  Logic defects reach 10x a bar, precision-sized ones 2x.  Measured
    (v2_48k, T = 24, x the decisive bar): resblock lrelu slope 0.01: 31-60, dilated conv's padding off by one row: 360-680, a missing conv bias: 17-45, one row
    per 128 of a conv 10 % off: 25-28 (max-abs; 5-6 in RMS), ups / noise-conv padding off by one, x / num_kernels skipped or doubled, missing ups bias,
    slope 0.01 before ups, slope 0.1 / no division before conv_post, missing conv_pre bias or cond: 1e3-1e6; X0 rounded to fp16 where the plan keeps fp32:
    137-206; the last of ELEVEN taps of one dilated conv x 0.97 -- 3 % of 9 % of one conv's weights, precision-sized -- 4.9-5.3 with fp32 streams, 3.2 with fp16.
    DROPPED: "the residual added from the rounded operand instead of the fp32 stream" reaches only 0.3-0.4x the bars on the stage sum (1.5x the floor: one extra
    fp16 rounding of x per pair level is what the floor's own flips amount to); a per-resblock tap would gain sqrt(3) at most.  It is printed, not asserted.
    DROPPED on the fp16-stream stages: the tile-row variant (k_rb_full has no 128-row tile; 4-5x its bars there).
  * The gap that is closed: the 0.97-tap and the tile-row variants PASS the old criteria (waveform RMS <= 1e-3 against the unrounded oracle, every stage tap
    <= 2e-3 relative RMS) and FAIL the per-layer bars.
  * The perturbed evaluations (K-loop order, tanhf, the one contractible multiply-add) stay within half of every bar.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import nsf_cases as nc  # noqa: E402
from conftest import golden_config_and_weights, golden_names, load_golden  # noqa: E402
from oracle import nsf_layer_oracle as lo  # noqa: E402
from oracle import nsf_oracle  # noqa: E402

REF_CASES = tuple(nc.Case(name, 1 + (i % 2), 7 + i, 200 + i) for i, name in enumerate(nc.CONFIGS))


@pytest.mark.parametrize("c", REF_CASES, ids=nc.case_id)
def test_unrounded_layers_are_the_reference(c):
    cfg, x, w = nc.CONFIGS[c.cfg], nc.inputs(c), nc.weights(c.cfg, c.seed)
    ref = {}
    with torch.no_grad():
        ref["post"] = nsf_oracle.generator_forward(cfg, w, x["z"], x["f0"], x["g"], x["noise"], taps=ref)
        har = ref.get("har")
        t32, t64 = {}, {}
        t32["post"] = lo.Layers(cfg, w, "f32", None).forward(x["z"], x["g"], har, t32)
        t64["post"] = lo.Layers(cfg, w, "f64", None).forward(x["z"], x["g"], har, t64)
    assert set(t32) == set(ref) - {"har"}
    for k in t32:
        want = ref[k] * cfg.num_kernels if k.startswith("stage") else ref[k]
        assert t32[k].shape == want.shape, k
        e32, d = nc.err(t32[k], want), nc.err(t64[k], want)  # d: the fp32 reference's own distance to the fp64 evaluation
        print("%s %s: composed f32 vs reference %.2e RMS %.2e max; reference vs f64 %.2e RMS %.2e max" % (nc.case_id(c), k, *e32, *d))
        assert e32[0] <= d[0] and e32[1] <= 2 * d[1], k
        assert d[0] <= 3e-6 * max(1.0, float(want.abs().max())), k  # (the 3e-6 class of test_sine_source_and_stage_taps_fp32)


@pytest.mark.parametrize("name", golden_names("dec_"))
def test_unrounded_layers_reproduce_the_reference_goldens(name):
    d = load_golden(name)
    cfg, w = golden_config_and_weights(d)
    z, g = torch.from_numpy(d["z"]), torch.from_numpy(d["g"])
    n_res = None if int(d["n_res"]) < 0 else int(d["n_res"])
    har = None
    with torch.no_grad():
        if cfg.use_f0:
            har = nsf_oracle.har_source(w, torch.from_numpy(d["f0"]), cfg.upp, cfg.sr, torch.from_numpy(d["noise"]))
        if n_res is not None:  # the realtime interpolation in front of the layers (nsf.py:155-162), as generator_forward does it
            if har is not None and n_res * cfg.upp != har.shape[-1]:
                har = F.interpolate(har, size=n_res * cfg.upp, mode="linear")
            if n_res != z.shape[-1]:
                z = F.interpolate(z, size=n_res, mode="linear")
        for arith in ("f32", "f64"):
            out = lo.Layers(cfg, w, arith, None).forward(z, g, har)
            assert out.shape == d["out"].shape
            e = nc.err(out, d["out"])
            print("%s %s: %.2e RMS %.2e max-abs vs the golden" % (name, arith, *e))
            assert e[1] < 5e-6


# ---- the bars reject the lookalikes -------------------------------------------------------------------------------------------------------

SEP = nc.DEFAULT[2]  # v2_48k, T = 24: stages 0 and 1 on the SPLIT path (fp32 X0 and Y), stages 2 and 3 on k_rb_full (fp16 X0 and Y)
LOGIC, PRECISION = 10, 2
VARIANTS = (
    [("pre", v, LOGIC) for v in ("no_bias", "no_cond")]
    + [(s, v, f) for s in ("stage0", "stage1") for v, f in (("tap097", PRECISION), ("tile_row", LOGIC), ("slope001", LOGIC), ("pad_off1", LOGIC), ("no_bias", LOGIC))]
    # fp16 streams (k_rb_full): the 0.97 tap still clears the precision class; "tile_row" is DROPPED there (no 128-row tile exists in k_rb_full, and one row in 128
    # reaches 4-5x its bars, under the logic class)
    + [("stage2", "tap097", PRECISION)] + [("stage2", v, LOGIC) for v in ("slope001", "pad_off1", "no_bias")]
    + [("up0", v, LOGIC) for v in ("tpad_off1", "npad_off1", "no_bias", "slope001")] + [("up0", "x0_rounded", PRECISION)]
    + [("up1", v, LOGIC) for v in ("div_skipped", "div_twice", "tpad_off1", "npad_off1", "no_bias", "slope001")] + [("up1", "x0_rounded", PRECISION)]
    + [("up2", v, LOGIC) for v in ("div_skipped", "div_twice", "tpad_off1", "npad_off1", "no_bias")]
    + [("post", v, LOGIC) for v in ("slope01", "div_skipped")])


def _ratio(e, b):
    return max(e[0] / b["bar_rms"], e[1] / b["bar_max"])


@pytest.mark.parametrize("name,variant,factor", VARIANTS, ids=["%s-%s" % v[:2] for v in VARIANTS])
def test_the_bars_separate_the_design_from_its_lookalikes(name, variant, factor):
    ch = nc.cpu_chain(SEP)
    b = ch["bars"][name]
    with torch.no_grad():
        y = lo.apply_layer(nc.make_layers(SEP, ch["paths"], "f32"), name, ch["taps"], variant)
    e = nc.err(y, b["y"])
    print("%s %s: RMS %.2e = %.1f x bar_rms (%.1f x floor), max-abs %.2e = %.1f x bar_max (%.1f x floor)" % (
        name, variant, e[0], e[0] / b["bar_rms"], e[0] / b["floor_rms"], e[1], e[1] / b["bar_max"], e[1] / b["floor_max"]))
    assert _ratio(e, b) >= factor, "%s/%s is only %.2f x its bars" % (name, variant, _ratio(e, b))


def test_the_dropped_variant_is_reported():
    ch = nc.cpu_chain(SEP)
    for name in ("stage0", "stage2"):
        b = ch["bars"][name]
        with torch.no_grad():
            y = lo.apply_layer(nc.make_layers(SEP, ch["paths"], "f32"), name, ch["taps"], "res_from_operand")
        e = nc.err(y, b["y"])
        print("%s res_from_operand (NOT separable on the stage sum): %.2f x bar_rms, %.2f x bar_max, %.1f x floor_rms" % (
            name, e[0] / b["bar_rms"], e[1] / b["bar_max"], e[0] / b["floor_rms"]))
        assert np.isfinite(e).all()


@pytest.mark.parametrize("variant", ["tap097", "tile_row"])
def test_the_old_criteria_accept_what_the_layer_bars_reject(variant):
    """The gap this file closes.  The stand-in for a device with the defect in stage 1: the rounded fp32 evaluation, end to end, with the variant."""
    c = SEP
    cfg, x, w, ch = nc.CONFIGS[c.cfg], nc.inputs(c), nc.weights(c.cfg, c.seed), nc.cpu_chain(c)
    ref, taps = {}, {}
    with torch.no_grad():
        wave_ref = nsf_oracle.generator_forward(cfg, w, x["z"], x["f0"], x["g"], x["noise"], taps=ref)
        wave = nc.make_layers(c, ch["paths"], "f32").forward(x["z"], x["g"], ch["taps"]["har"], taps, {"stage1": variant})
    # old: the waveform's RMS bar (tests/test_gpu_generator.py BAR["fp16"]) and the stage taps' relative RMS bar (test_mfma_stage_taps_fp16)
    wave_rms = nc.err(wave, wave_ref)[0]
    rel = {}
    for i in range(len(cfg.upsample_rates)):
        want = ref["stage%d" % i] * cfg.num_kernels
        rel[i] = nc.err(taps["stage%d" % i], want)[0] / float(want.double().pow(2).mean().sqrt())
    print("%s in stage1: waveform RMS %.2e (old bar 1e-3), stage taps relative RMS %s (old bar 2e-3)" % (variant, wave_rms, ["%.2e" % r for r in rel.values()]))
    assert wave_rms <= 1e-3 and max(rel.values()) <= 2e-3, "the old criteria already reject %s" % variant
    # new: stage 1 against its oracle on the tap in front of it -- and only stage 1
    taps.update(z=x["z"], g=x["g"], har=ch["taps"]["har"], post=wave)
    for name in nc.layer_list(c):
        b = nc.layer_bars(c, ch["paths"], name, taps)
        e = nc.err(taps[name], b["y"])
        print("  %-6s %.2f x bar_rms %.2f x bar_max" % (name, e[0] / b["bar_rms"], e[1] / b["bar_max"]))
        if name == "stage1":
            assert _ratio(e, b) >= 2, "stage1 with %s passes the per-layer bars" % variant
        else:
            assert e[0] <= b["bar_rms"] and e[1] <= b["bar_max"], name


# ---- the kernels' liberties stay inside half the bars ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", nc.CPU_TABLE, ids=nc.case_id)
def test_perturbations_stay_inside_half_the_bars(c):
    ch = nc.cpu_chain(c)
    worst = {"mfma": 0.0, "post": 0.0}
    for seed in (1, 2):
        for name in nc.layer_list(c):
            b = ch["bars"][name]
            ly = nc.make_layers(c, ch["paths"], "f32", {"reorder": True, "tanh": 4, "fma": True, "seed": seed})
            with torch.no_grad():
                y = lo.apply_layer(ly, name, ch["taps"])
            e = nc.err(y, b["y"])
            share = (e[0] / b["bar_rms"], e[1] / b["bar_max"])
            ratio = (e[0] / b["floor_rms"] if b["floor_rms"] else 0.0, e[1] / b["floor_max"] if b["floor_max"] else 0.0)
            print("%s seed %d %-6s: %.2f / %.2f x floor (RMS / max-abs) = %.2f / %.2f of the bar" % (nc.case_id(c), seed, name, *ratio, *share))
            assert share[0] <= 0.5 and share[1] <= 0.5, "%s: the perturbed evaluation takes %.2f / %.2f of the bars" % (name, *share)
            k = nc.kind_of(name)
            f = nc.FACTOR[k]
            if f * b["floor_rms"] >= b["add_rms"]:
                worst[k] = max(worst[k], ratio[0])
            if f * b["floor_max"] >= b["add_max"]:
                worst[k] = max(worst[k], ratio[1])
    print("%s: largest ratio where the floor decides the bar: %s" % (nc.case_id(c), worst))
