"""The checker of the front's kernels checked (no GPU): oracle/front_layer_oracle.py is the reference's front, and the per-segment bars
tests/front_layer_cases.py derives from it tell the kernels' documented design from what looks like it.

  * With the operand rounding off, the segments composed are ``front_oracle.infer_front`` and its taps (the float64 composition differs from the float64
    reference only by the float32 constants the kernels hold: sqrtf(192), sqrtf(96), 0.66666f, 1e-5f), for the shipped config, window 15 / flow kernel 7,
    v1's 256 input channels, no f0 and a flow_head; and they reproduce the committed ``front_*`` goldens (written by the real reference modules), z and
    all five taps on every row, to the 2e-5 max-abs tests/test_cpu_oracle.py holds front_oracle to.
  * The perturbed evaluations (K-loop order, the split forms' partial sums, the online softmax's tile order, the hardware exp) stay within half of
    every bar, on every case of CPU_TABLE.
  * The gap that is closed: five planted defects PASS today's criteria (z <= 5e-3 RMS against the unrounded oracle, the five taps of tests/test_gpu_front.py
    at their bars) and FAIL their own segment's bars by >= 2x, while every other segment stays inside its bars.  Measured (x the decisive bar): the outermost
    relative key of layer 2 dropped 18.0, the outermost relative value of layer 4 dropped 18.0, the last tap of ffn_layers.3.conv_1 x 0.99 / x 0.995 70.8 / 35.6,
    the last tap of flow.flows.2.enc.in_layers.1 x 0.99 4.7 (z 2.7-4.8e-3 against today's 5e-3).
  * Lookalikes, reported with their ratio whichever side they fall on and NOT asserted on: LayerNorm eps 1e-3 in all twelve norms -- accepted today (z 1.99e-3),
    7.7-13.1x the bars of layer<i> and 2.3-3.6x of attn1..5 but 1.8x of attn0: does not stand clear everywhere; 2/3 for 0.66666 -- accepted today, 9.3x;
    hidden rows not masked before conv_2 1236x, the skip sum not reset at ``first`` 1331x, the gc slice of the wrong layer 854x, slope 0.01 in emb 1e5x (today's
    criteria reject these four too).
  * A hidden value of the FFN within 2 float32 ulps of a rounding midpoint passes rounded either way (the tie-aware comparison of layer<i>); the same flip of a
    value that is NOT a near-tie fails, and so does the near-tie's flip without the tie-aware comparison.
  * An odd flow_n_flows handed out in the device's channel order (the k_fr_out defect this work found and fixed) fails the bar of "out".

The stand-in for a device with a defect: the ROUNDED float32 evaluation, composed end to end, with the variant in one segment.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import front_layer_cases as fc  # noqa: E402
from conftest import golden_names, load_golden  # noqa: E402
from oracle import front_layer_oracle as flo  # noqa: E402
from oracle import front_oracle, synth  # noqa: E402
from oracle.front_oracle import FrontConfig  # noqa: E402

REF_CASES = (fc.Case("ref-default", 2, 50, lengths=(50, 41)), fc.Case("ref-head6", 1, 40, fh=6, seed=5),
             fc.Case("ref-w15-k7", 2, 37, lengths=(37, 1), cfg=fc.O(window_size=15, flow_kernel_size=7), seed=6),
             fc.Case("ref-v1", 1, 33, cfg=fc.O(in_channels=256), seed=7), fc.Case("ref-no-f0", 1, 33, cfg=fc.O(use_f0=False), seed=8),
             fc.Case("ref-3-flows", 1, 20, cfg=fc.O(flow_n_flows=3, flow_n_layers=2, n_layers=2), seed=9))


def _reference(c, dtype):
    """front_oracle.infer_front in ``dtype`` -> taps channels-last, "out" = z * x_mask; the flow taps are not among the reference's."""
    cfg, x, w = fc.config(c), fc.inputs(c), fc.weights(c)
    w = {k: v.to(dtype) if v.is_floating_point() else v for k, v in w.items()}
    raw = {}
    with torch.no_grad():
        z, m1, _ = front_oracle.infer_front(cfg, w, x["phone"].to(dtype), x["pitch"], x["lengths"], x["sid"], x["noise"].to(dtype), c.fh or None, raw)
    out = {k: v.transpose(1, 2) for k, v in raw.items() if k not in ("m", "logs")}
    out["out"] = z * m1
    return out


@pytest.mark.parametrize("c", REF_CASES, ids=fc.case_id)
def test_unrounded_segments_are_the_reference(c):
    x = fc.inputs(c)
    ref32, ref64 = _reference(c, torch.float32), _reference(c, torch.float64)
    t32, t64 = {}, {}
    with torch.no_grad():
        fc.make_segments(c, "f32", operand=None).forward(x["phone"], x["pitch"], x["lengths"], x["g"], x["noise"], c.fh, t32)
        fc.make_segments(c, "f64", operand=None).forward(x["phone"], x["pitch"], x["lengths"], x["g"], x["noise"], c.fh, t64)
    for k in ref64:
        name = k
        want = ref64[k]
        scale = max(1.0, float(want.abs().max()))
        e64, e32, d = fc.err(t64[name], want), fc.err(t32[name], want), fc.err(ref32[k], want)  # d: the fp32 reference's own distance to the fp64 one
        print("%s %s: composed f64 vs reference f64 %.2e RMS %.2e max; composed f32 %.2e / %.2e; reference f32 %.2e / %.2e" % (c.name, k, *e64, *e32, *d))
        assert t64[name].shape == want.shape, k
        assert e64[1] <= 2e-7 * scale, k          # the float32 constants: 2^-24 relative each
        assert e32[0] <= 2 * d[0] + 1e-7 * scale and e32[1] <= 3 * d[1] + 1e-6 * scale, k


@pytest.mark.parametrize("name", golden_names("front_"))
def test_unrounded_segments_reproduce_the_reference_goldens(name):
    d = load_golden(name)
    cfg = FrontConfig(in_channels=int(d["in_channels"]))
    w = synth.make_front_weights(cfg, int(d["seed"]))
    assert synth.weights_sha256(w) == d["weights_sha256"]
    fh = max(int(d["flow_head"]), 0)
    for arith in ("f32", "f64"):
        taps = {}
        with torch.no_grad():
            z = flo.Segments(cfg, w, arith, None).forward(torch.from_numpy(d["phone"]), torch.from_numpy(d["pitch"]), torch.from_numpy(d["lengths"]),
                                                          torch.from_numpy(d["g"]), torch.from_numpy(d["noise"]), fh, taps)
        taps["z"] = z
        for k in ("emb", "attn0", "layer0", "layer5", "z_p", "z"):
            assert taps[k].shape == d[k].shape, (k, taps[k].shape, d[k].shape)
            e = fc.err(taps[k], d[k])
            print("%s %s %s: %.2e RMS %.2e max-abs vs the golden" % (name, arith, k, *e))
            assert e[1] < 2e-5, k


# ---- the kernels' liberties stay inside half the bars ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", fc.CPU_TABLE, ids=fc.case_id)
def test_perturbations_stay_inside_half_the_bars(c):
    ch = fc.cpu_chain(c)
    worst = dict.fromkeys(fc.KINDS, 0.0)
    for seed in (1, 2):
        sg = fc.make_segments(c, "f32", {**fc.PERTURB, "seed": seed})
        for name in flo.segment_names(fc.config(c)):
            b = ch["bars"][name]
            with torch.no_grad():
                full = flo.apply_segment(sg, name, {**fc.inputs(c), **ch["taps"]})
            y = fc.compared(c, name, full)
            want = fc.tie_resolved(c, name, ch["taps"], full)[0] if fc.kind_of(name) == "ffn" else b["y"]  # as the GPU test compares layer<i>
            e = fc.err(y, want)
            share = (e[0] / b["bar_rms"], e[1] / b["bar_max"])
            ratio = (e[0] / b["eff_rms"] if b["eff_rms"] else 0.0, e[1] / b["eff_max"] if b["eff_max"] else 0.0)
            print("%s seed %d %-7s: %.2f / %.2f x floor (RMS / max-abs) = %.2f / %.2f of the bar; own floor %.2e / %.2e, floor used %.2e / %.2e" % (
                c.name, seed, name, *ratio, *share, b["floor_rms"], b["floor_max"], b["eff_rms"], b["eff_max"]))
            assert share[0] <= 0.5 and share[1] <= 0.5, "%s: the perturbed evaluation takes %.2f / %.2f of the bars" % (name, *share)
            k = fc.kind_of(name)
            if fc.FACTOR[k] * b["eff_rms"] >= b["add_rms"]:
                worst[k] = max(worst[k], ratio[0])
            if fc.FACTOR[k] * b["eff_max"] >= b["add_max"]:
                worst[k] = max(worst[k], ratio[1])
    print("%s: largest ratio where the floor decides the bar: %s" % (c.name, worst))
    for k, v in worst.items():
        assert v <= fc.PERTURB_WORST[k] + 0.005, "%s reaches %.2f x the floor: PERTURB_WORST / FACTOR of front_layer_cases.py are out of date" % (k, v)


# ---- the bars reject the planted defects that today's criteria accept -------------------------------------------------------------------------

C = fc.CPU_MAIN
OLD_TAPS = (("emb", 2e-3), ("attn0", 4e-3), ("layer0", 4e-3), ("layer5", 5e-3), ("z_p", 5e-3))  # tests/test_gpu_front.py
EPS_EVERYWHERE = {k: "eps" for i in range(6) for k in ("attn%d" % i, "ffn%d" % i)}
# (id, the segment that carries the defect, the variants)
DEFECTS = (
    ("relk-edge-layer2", "attn2", {"attn2": "relk_edge"}),        # the outermost relative KEY dropped: a band edge off by one
    ("relv-edge-layer4", "attn4", {"attn4": "relv_edge"}),        # the outermost relative VALUE dropped
    ("ffn3-tap-x0.99", "layer3", {"ffn3": ("tap", 0.99)}),        # one tap of ffn_layers.3.conv_1 x 0.99
    ("ffn3-tap-x0.995", "layer3", {"ffn3": ("tap", 0.995)}),
    ("flow1-tap-x0.99", "flow1", {"flow1": ("tap", 0.99)}),       # one tap of flow.flows.2.enc.in_layers.1 x 0.99
)
LOOKALIKES = (
    ("eps-1e-3-in-all-norms", None, EPS_EVERYWHERE),
    ("hidden-rows-not-masked", "layer2", {"ffn2": "hidden_unmasked"}),
    ("gc-slice-of-the-wrong-layer", "flow2", {"flow2": "gc_wrong_layer"}),
    ("slope-0.01-in-emb", "emb", {"emb": "slope001"}),
    ("two-thirds", "z_p", {"z_p": "two_thirds"}),
)


def _defective_run(variants, skip_stale=None):
    """The rounded float32 front with ``variants``, end to end -> its taps ("out" = z).  ``skip_stale`` = f: coupling f starts its skip sum from what coupling
    f + 1 left in the buffer (the skip sum not reset at ``first``)."""
    x, taps = fc.inputs(C), {}
    sg = fc.make_segments(C, "f32", variants=variants)
    inp = {k: x[k] for k in ("phone", "pitch", "lengths", "g", "noise", "flow_head")}
    with torch.no_grad():
        for name in flo.segment_names(fc.config(C)):
            extra = {}
            if skip_stale is not None and name == "flow%d" % skip_stale:
                prev = "flow%d" % (skip_stale + 1)
                extra["skip0"] = sg.flow(skip_stale + 1, taps[flo.feed_of(fc.config(C), prev)], x["lengths"], x["g"], C.fh, want_skip=True)
            taps[name] = flo.apply_segment(sg, name, {**inp, **taps, **extra})
    return taps


def _old_criteria(taps):
    ref = _reference(C, torch.float64)
    got = {"z": fc.err(taps["out"], ref["out"])[0]}
    got.update({k: fc.err(taps[k], ref[k])[0] for k, _ in OLD_TAPS})  # on every row, as the golden test compares them (the padding rows agree too)
    ok = got["z"] <= 5e-3 and all(got[k] <= bar for k, bar in OLD_TAPS)
    return got, ok


def _per_segment(taps):
    """{segment: the larger of error / bar (RMS, max-abs)} with every segment's oracle applied to the defective run's own previous tap"""
    out = {}
    for name in flo.segment_names(fc.config(C)):
        b = fc.segment_bars(C, name, taps, got=taps[name])
        e = fc.err(fc.compared(C, name, taps[name]), b["y"])
        out[name] = (max(e[0] / b["bar_rms"], e[1] / b["bar_max"]), e[0] / b["floor_rms"] if b["floor_rms"] else 0.0, e[1] / b["floor_max"] if b["floor_max"] else 0.0)
    return out


def test_the_clean_run_passes_both():
    taps = _defective_run({})
    old, ok = _old_criteria(taps)
    seg = _per_segment(taps)
    print("clean: old criteria %s; per segment x bar: %s" % ({k: "%.2e" % v for k, v in old.items()}, {k: "%.2f" % v[0] for k, v in seg.items()}))
    assert ok and all(v[0] <= 1.0 for v in seg.values())


@pytest.mark.parametrize("what,where,variants", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_the_old_criteria_accept_what_the_segment_bars_reject(what, where, variants):
    taps = _defective_run(variants)
    old, ok = _old_criteria(taps)
    print("%s: old criteria: %s" % (what, ", ".join("%s %.2e" % kv for kv in old.items())))
    assert ok, "today's criteria already reject %s" % what
    seg = _per_segment(taps)
    for name, (share, fr, fm) in seg.items():
        print("  %-7s %.2f x its bar (%.1f x floor RMS, %.1f x floor max-abs)" % (name, share, fr, fm))
    assert seg[where][0] >= 2.0, "%s: %s is only %.2f x its bars" % (what, where, seg[where][0])
    for name, (share, _, _) in seg.items():
        assert name == where or share <= 1.0, "%s: segment %s leaves its bars (%.2f x) though the defect sits in %s" % (what, name, share, where)


@pytest.mark.parametrize("what,where,variants", LOOKALIKES + (("skip-sum-not-reset", "flow1", None),), ids=[d[0] for d in LOOKALIKES] + ["skip-sum-not-reset"])
def test_the_lookalikes_are_reported(what, where, variants):
    taps = _defective_run(variants or {}, skip_stale=1 if variants is None else None)
    old, ok = _old_criteria(taps)
    seg = _per_segment(taps)
    hit = {n: v for n, v in seg.items() if (where is None and fc.kind_of(n) in ("attn", "ffn")) or n == where}
    worst = max(v[0] for v in hit.values())
    clear = min(v[0] for v in hit.values()) >= 2.0
    print("%s: today's criteria %s it (z %.2e); its segment(s) reach %.2f - %.2f x their bars: %s" % (
        what, "ACCEPT" if ok else "reject", old["z"], min(v[0] for v in hit.values()), worst,
        "stands clear" if clear else "does NOT stand clear of the bars everywhere -- not asserted on"))
    for n, v in hit.items():
        print("  %-7s %.2f x its bar (%.1f x floor RMS, %.1f x floor max-abs)" % (n, *v))
    assert np.isfinite(worst)
    assert all(v[0] <= 1.0 for n, v in seg.items() if n not in hit), "a segment without the variant leaves its bars"


def test_an_odd_flow_count_in_physical_order_fails_the_out_bar():
    """The defect found in k_fr_out (by test_unrounded_segments_are_the_reference's 3-flow case; fixed: its ``rev`` argument), restated: with flow_n_flows = 3 the last coupling leaves the stream with its
    channel axis reversed; handing that out as z passes no bar of "out" (its floor is 0: the segment only moves values)."""
    c = REF_CASES[-1]
    assert fc.config(c).flow_n_flows % 2 == 1
    x, taps = fc.inputs(c), {}
    with torch.no_grad():
        fc.make_segments(c, "f32").forward(x["phone"], x["pitch"], x["lengths"], x["g"], x["noise"], c.fh, taps)
        bad = flo.apply_segment(fc.make_segments(c, "f32", variants={"out": "physical_order"}), "out", {**x, **taps})
    b = fc.segment_bars(c, "out", taps)
    good, wrong = fc.err(taps["out"], b["y"]), fc.err(bad, b["y"])
    print("out, 3 flows: logical order %.2e / %.2e, physical order %.2e / %.2e (bars %.2e / %.2e)" % (*good, *wrong, b["bar_rms"], b["bar_max"]))
    assert good == (0.0, 0.0)
    assert wrong[0] >= 2 * b["bar_rms"] and wrong[1] >= 2 * b["bar_max"]


def test_a_near_tie_passes_rounded_either_way_and_nothing_else_does(monkeypatch):
    """What the first GPU run met in "layer2" with bf16 operands, restated: conv_1's bias of one channel is set so that the LARGEST hidden value of the layer
    lands on the midpoint between two bf16 values (to the float32 rounding of the bias).  A device that rounds it down and one that rounds it up both pass
    the tie-aware comparison at (almost) no error, while against the plain oracle one of the two carries the whole flip (printed as a share of the bars).  Rounding
    a hidden value that is NOT a near-tie the other way is not absorbed: its error under the tie-aware comparison is the plain one."""
    c = fc.Case("near-tie", 2, 65, lengths=(65, 40), operand="bf16", seed=4242)  # (a seed of its own: its pooled sibling is no other case's)
    i, name = 2, "layer2"
    x, taps = fc.inputs(c), dict(fc.cpu_chain(c)["taps"])
    bias = "enc_p.encoder.ffn_layers.%d.conv_1.bias" % i
    w = dict(fc.weights(c))
    with torch.no_grad():
        head = flo.Segments(fc.config(c), w, "f64", c.operand).ffn_head(i, taps["attn2"], x["lengths"])
        b_, t_, j_ = (int(k) for k in (head["hid"] == head["hid"].max()).nonzero()[0])
        hid, hr = head["hid"][b_, t_, j_], head["hr"][b_, t_, j_]
        mid = hr + 2.0 ** (math.floor(math.log2(float(hr))) - 8)  # half a bf16 ulp above hr
        w[bias] = w[bias].clone()
        w[bias][j_] = float(w[bias][j_].double() + (mid - hid))
    orig = fc.weights
    monkeypatch.setattr(fc, "weights", lambda case: w if case.name == c.name else orig(case))  # this case's oracle and floor see the planted bias
    sg = fc.make_segments(c, "f64")
    with torch.no_grad():
        head = sg.ffn_head(i, taps["attn2"], x["lengths"])
        assert (b_, t_, j_) in head["ties"], "the planted value is not a near-tie: %r" % (head["ties"],)
        devices = {"nearest": sg.ffn_tail(i, head), "the other way": sg.ffn_tail(i, head, [(b_, t_, j_)])}
        far = next(idx for idx in ((b_, t, j_) for t in range(c.T)) if idx not in head["ties"] and float(head["hid"][idx]) > 2.0)
        devices["not-a-tie"] = sg.ffn_tail(i, head, [far])
    plain, out = fc.segment_bars(c, name, taps), {}
    for what, dev in devices.items():
        b = fc.segment_bars(c, name, taps, got=dev)
        e, e0 = fc.err(fc.compared(c, name, dev), b["y"]), fc.err(fc.compared(c, name, dev), plain["y"])
        out[what] = (e, e0, max(e[0] / b["bar_rms"], e[1] / b["bar_max"]), max(e0[0] / b["bar_rms"], e0[1] / b["bar_max"]))
        print("hidden[%d, %d, %d] = %.4f, the device rounds %s: tie-aware %.2e / %.2e = %.3f x the bars (%d near-ties, %d taken the other way); plain oracle %.2e / %.2e = %.3f x" % (
            b_, t_, j_, float(head["hid"][b_, t_, j_]), what, *e, out[what][2], b["ties"], b["ties_flipped"], *e0, out[what][3]))
    assert out["nearest"][2] <= 0.01 and out["the other way"][2] <= 0.01
    assert out["the other way"][1][1] >= 100 * max(out["the other way"][0][1], 1e-12)  # against the plain oracle the whole flip is there
    assert out["not-a-tie"][0] == out["not-a-tie"][1] and out["not-a-tie"][0][1] >= 0.1 * out["the other way"][1][1]  # not absorbed
