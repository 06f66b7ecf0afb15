"""The generator's kernels (csrc/nsf.hip and the family headers it launches, rb_stream_kernels.hpp), LAYER BY LAYER against the fp64 oracle that rounds where they round
(oracle/nsf_layer_oracle.py), at the bars tests/nsf_cases.py derives from that oracle's own fp32 noise floor -- an RMS bar and a max-abs bar per layer.

Layer n's oracle is applied to the tap the device itself produced for layer n - 1 ("har", "pre", "up<i>", "stage<i>" of ``debug_tap``; the last layer's
output is the waveform of a plain forward), so a failing layer names the kernel: conv_pre, k_ups (+ the noise conv's route), the ResBlock path the case
pins (SPLIT, PAIR, STREAM, FULL with each of its tile classes), conv_post's two kernels.  What ran is reported by the compared forward itself
(``gen.last_plan()``) and asserted: against the case's ``want``, the restated planning rules and the profiler's kernel names (tests/nsf_cases.py check_plan).
Every tap is fetched twice and must be bit-equal; the plain forward is run before and after the tap calls and must be bit-equal too.  The tap calls end a
forward early and copy what the kernels stored; that they ARE the real run is pinned by the last layer: conv_post's oracle applied to the "stage<last>"
tap must give the plain forward's waveform to a few fp32 ulps (the bar of "post").

The coarse end-to-end checks stay where they were (tests/test_gpu_generator.py: 1e-3 RMS on the waveform, 2e-3 relative on the stage taps).
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nsf_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu


def _within_bars(r):
    """Prints every layer's ratios to its floor, then asserts both bars of every layer."""
    print("%s: paths %s kernels %s plan %s" % (r["case"], r["paths"], r["kernels"], r["plan"]))
    bad = []
    for e in r["layers"]:
        what = e["layer"] if e["item"] is None else "%s[%d]" % (e["layer"], e["item"])
        print("  %-9s HIP vs f64 oracle RMS %.3e max %.3e = %s x floor_rms, %s x floor_max (floor %.3e / %.3e, bars %.3e / %.3e)" % (
            what, e["rms"], e["max"], "%.2f" % e["rms_ratio"] if e["rms_ratio"] is not None else "-",
            "%.2f" % e["max_ratio"] if e["max_ratio"] is not None else "-", e["floor_rms"], e["floor_max"], e["bar_rms"], e["bar_max"]))
        if not e["within_bars"]:
            bad.append("%s: RMS %.3e (bar %.3e) max %.3e (bar %.3e)" % (what, e["rms"], e["bar_rms"], e["max"], e["bar_max"]))
    assert not bad, "%s on %s: %s" % (r["case"], r["paths"], "; ".join(bad))


@pytest.mark.parametrize("c", nc.TABLE, ids=nc.case_id)
def test_every_layer_against_its_fp16_operand_oracle(c, gpu):
    _within_bars(nc.device_case(c, gpu)[0])


@pytest.mark.parametrize("c", nc.BATCH_CASES, ids=nc.case_id)
def test_batch_items_against_their_own_oracle_and_their_single_calls(c, gpu):
    r, wave, gen = nc.device_case(c, gpu, items=True)
    _within_bars(r)
    x, cfg = nc.inputs(c), nc.CONFIGS[c.cfg]
    assert not torch.equal(wave[0], wave[1])
    for b in range(c.B):
        z, g = x["z"][b:b + 1].to(gpu), x["g"][b:b + 1].to(gpu)
        if cfg.use_f0:
            one = gen(z, x["f0"][b:b + 1].to(gpu), g, noise=x["noise"][b:b + 1].to(gpu)).cpu()
        else:
            one = gen(z, g).cpu()
        assert torch.equal(one[0], wave[b]), "item %d differs from its single-item call: rms %.3e" % (b, nc.err(one[0], wave[b])[0])
