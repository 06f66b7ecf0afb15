"""The excitation in front of the generator's layers (csrc/nsf_source_kernels.hpp: k_phase_scan, k_sine_source, k_interp_linear, launched by excitation() and
conv_pre() of csrc/nsf.hip) against the oracles of oracle/source_oracle.py, over the cases of tests/source_cases.py.  tests/test_gpu_nsf_layers.py takes "har" from
the device, so a wrong excitation passes every layer test; this file is what holds it.

  * "har" (``debug_tap``) lies inside ``har_interval`` on EVERY sample of every case: the phase is bit-determined (tests/test_cpu_source.py: no frame is excluded),
    sinf and tanhf get 4 ulp each, everything else is float32 arithmetic with one rounding per operation.  The worst distance from the interval's centre is printed
    in float32 ulps with the frame and sample where it occurs.  The operand type does not enter the excitation: the fp32 and the fp16 handle return the same bits.
  * "har" under ``n_res`` against ``interp_admissible`` of the device's own plain tap of the same inputs (only the interpolation is compared, as the layer tests
    compare only their layer); n_res == T is the plain tap bit for bit.
  * z under ``n_res``: the "pre" tap of an fp32-operand handle against the fp64 conv_pre + cond on each admissible interpolation of z, at the bars
    tests/nsf_cases.py derives for that layer.

A per-item ``n_res`` and ``lengths`` cannot be tapped: tests/test_gpu_nsf_nres_ragged.py and tests/test_gpu_generator.py tie them bit for bit to single-item calls,
and those single-item calls are what the oracles here hold.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import source_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _handles_end_with_the_module():
    yield
    sc.release_handles()


@pytest.mark.parametrize("c", sc.HAR_CASES, ids=sc.case_id)
def test_har_lies_inside_the_interval(c, gpu):
    r, _ = sc.device_har_case(c, gpu)
    print("%s: outside %d of %d, worst %.2f ulp from the centre at %s, %.2f of the way to the interval's edge; interval width median %.2e max %.2e" % (
        r["case"], r["outside"], r["samples"], r["worst_ulp"], r["worst_at"], r["worst_share"], r["width_median"], r["width_max"]))
    assert r["outside"] == 0, "%d samples outside the interval, first (item, frame, sample) %s" % (r["outside"], r["first_outside"])


def test_the_operand_type_does_not_enter_the_excitation(gpu):
    c = [c for c in sc.HAR_CASES if c.B == 3 and c.T == 258][0]
    a = sc.device_tap(c, sc.handle(c.cfg, c.linear, "fp16", gpu), gpu)
    b = sc.device_tap(c, sc.handle(c.cfg, c.linear, "fp32", gpu), gpu)
    assert a.any() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("c", sc.INTERP_CASES + sc.INTERP_IDENTITY, ids=sc.case_id)
def test_har_under_n_res_is_an_admissible_interpolation(c, gpu):
    r, plain, got = sc.device_interp_case(c, gpu)
    if c.n_res == c.T:
        assert r["bit_equal_to_plain"], "n_res == T must not interpolate at all"
        return
    print("%s: outside %d of %d; bit-equal to torch's float32 %.4f, to <index rounding>_<output rounding> %s (the two index roundings differ on %d samples of a row)" % (
        r["case"], r["outside"], r["samples"], r["equal_torch_f32"], {k[6:]: "%.4f" % v for k, v in r.items() if k.startswith("equal_") and k != "equal_torch_f32"},
        r["index_roundings_differ_per_row"]))
    assert r["outside"] == 0


@pytest.mark.parametrize("c", sc.INTERP_Z_CASES, ids=sc.case_id)
def test_z_under_n_res_meets_the_bars_of_pre(c, gpu):
    r = sc.device_z_case(c, gpu)
    for e in r["candidates"]:
        print("%s: pre vs f64 oracle on the %s index: RMS %.3e max %.3e (floor %.3e / %.3e, bars %.3e / %.3e)" % (
            r["case"], e["index"], e["rms"], e["max"], e["floor_rms"], e["floor_max"], e["bar_rms"], e["bar_max"]))
    assert any(e["within_bars"] for e in r["candidates"])
