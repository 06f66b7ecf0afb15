"""The host part of the device input gate: ``realtime.input_gate_cutoffs`` turns the gate's comparison behind a log10 into two
float32 RMS cutoffs, and the rule the device evaluates with them (``input_gate_cases.device_rule``, a numpy statement of
``rvcmi_glue_input_gate_batch``) gives the very block ``realtime.input_gate`` gives.  No GPU."""
import numpy as np
import pytest

import input_gate_cases as gc


def _f32_neighbours(v, k):
    """The k float32 values on either side of ``v`` (and ``v``), non-negative and finite ones only, ascending."""
    b = int(np.array([v], np.float32).view(np.uint32)[0])
    bits = np.arange(max(b - k, 0), min(b + k, 0x7F7FFFFF) + 1, dtype=np.uint32)
    return bits.view(np.float32)


@pytest.mark.parametrize("threhold", gc.CUTOFF_THRESHOLDS)
def test_cutoffs_are_the_predicate_of_amplitude_to_db(threhold):
    """For the 2000 float32 neighbours on either side of each cutoff: ``r < cut`` is ``db(r) < threhold`` (with the 80 dB subtracted for cut_b),
    ``db`` being ``amplitude_to_db`` on the single value."""
    from rvc_amd.realtime import amplitude_to_db, input_gate_cutoffs

    cut_a, cut_b = input_gate_cutoffs(threhold)
    assert 0 < cut_a < cut_b < np.inf and np.float32(cut_a) == cut_a and np.float32(cut_b) == cut_b
    for r in _f32_neighbours(cut_a, 2000):
        assert bool(r < np.float32(cut_a)) == bool((amplitude_to_db(np.array([r], np.float32)) < threhold)[0]), r
    for r in _f32_neighbours(cut_b, 2000):
        clipped = (amplitude_to_db(np.array([r], np.float32)) - np.float32(80.0)).astype(np.float32)
        assert bool(r < np.float32(cut_b)) == bool((clipped < threhold)[0]), r
    assert input_gate_cutoffs(threhold) == (cut_a, cut_b)


@pytest.mark.parametrize("zc,blk", gc.GEOMETRIES)
@pytest.mark.parametrize("threhold", gc.CUTOFF_THRESHOLDS[:5])
def test_device_rule_equals_input_gate(zc, blk, threhold):
    """Three consecutive blocks per case (the state carries): levels within +-2 dB of the threshold, then one loud sample (the 80 dB clip
    keeps every frame), then a NaN (no frame quiet)."""
    from rvc_amd.realtime import input_gate, input_gate_cutoffs

    cut_a, cut_b = input_gate_cutoffs(threhold)
    rng = np.random.default_rng(zc * 1000 + blk + int(-threhold * 100))
    buf_host, buf_rule = np.zeros(4 * zc, np.float32), np.zeros(4 * zc, np.float32)
    zeroed = kept = 0
    for kind in ("levels", "levels", "loud", "levels", "nan", "levels"):
        x = gc.stretches(rng, blk, zc, threhold, loud=(blk // 2, gc.loud_value(threhold)) if kind == "loud" else None,
                         nan_at=blk // 3 if kind == "nan" else None)
        want = input_gate(x.copy(), buf_host, zc, threhold)
        got, buf_rule = gc.device_rule(x, buf_rule, zc, cut_a, cut_b)
        assert np.array_equal(got, want, equal_nan=True), (kind, int((got != want).sum()))
        assert np.array_equal(buf_rule, buf_host, equal_nan=True)
        if kind == "levels":
            zeroed += int((want == 0).sum() >= zc)
            kept += int((want != 0).sum() >= zc)
    assert zeroed and kept   # the inputs do fall on both sides of the gate


def test_cutoff_ends():
    """At or below the -100 dB floor of ``amplitude_to_db`` (amin = 1e-5) nothing is quiet: cut_a == 0.  Above every level a finite
    float32 square reaches, the cutoffs sit where the square overflows: every such RMS is quiet.  -60, the GUI's "gate off" value, is an
    ordinary threshold for the function (the callers do not gate at or below it)."""
    from rvc_amd.realtime import input_gate_cutoffs

    assert input_gate_cutoffs(-100.5)[0] == 0.0 and input_gate_cutoffs(-1000.0) == (0.0, 0.0)
    cut_a, cut_b = input_gate_cutoffs(-60.0)
    assert abs(cut_a / 1e-3 - 1) < 1e-5 and abs(cut_b / 10.0 - 1) < 1e-5
    big = float(np.sqrt(np.float64(np.finfo(np.float32).max)))
    for c in input_gate_cutoffs(400.0) + input_gate_cutoffs(float("inf")):
        assert abs(c / big - 1) < 1e-6
    assert input_gate_cutoffs(float("nan")) == (0.0, 0.0)   # nothing is below NaN


def test_bisection_ends():
    """``_first_true``: +inf when not even +inf satisfies the predicate, 0 when everything does, and the exact boundary in between."""
    from rvc_amd.realtime import _first_true

    none = _first_true(lambda r: False)
    assert np.isinf(none) and none > 0 and none.dtype == np.float32
    assert _first_true(lambda r: True) == 0.0
    assert np.isinf(_first_true(lambda r: bool(np.isinf(r))))            # only +inf itself
    edge = np.float32(0.3)
    assert _first_true(lambda r: r >= edge) == edge and _first_true(lambda r: r > edge) == np.nextafter(edge, np.float32(1))
