"""The front's kernels in their default arithmetic (fp16 / bf16 operands; csrc/front.hip, front_kernels.hpp), SEGMENT BY SEGMENT against the float64
oracle that rounds where they round (oracle/front_layer_oracle.py), at the bars tests/front_layer_cases.py derives on the CPU -- an RMS bar and a
max-abs bar per segment.

Segment n's oracle is applied to the tap the device itself produced for segment n - 1 ("emb", "attn<i>", "layer<i>", "z_p", "flow<f>" of ``debug_tap``;
the last segment's output is z of a plain forward), so a failing segment names the kernels: enc_emb; enc_qkv + enc_attn + enc_o_ln; the FFN form the case pins
(fused k_fr_ffn, split k_fr_ffn_part + k_fr_ffn_ln, or the two conv launches); enc_proj_zp; flow_pre + the WN form the case pins (k_fr_wn, or the gate launch
-- channel split or tap split -- + the res_skip launch) + flow_post; front_out.  What ran is observed from the profiler's kernel names and asserted; one
name covers both tile heights and "flow_wn_gate" both split modes, so the tile height and the split mode are as computed (csrc/front.hip restated in
front_layer_cases.expected_forms), not observed -- every record says so.  Every tap is fetched twice and must be bit-equal; the plain forward runs before
and after the tap calls and must be bit-equal too; the "flow0" tap, transposed and masked, must be the forward's z bit for bit.

"layer<i>" is compared tie-aware: a hidden activation the oracle finds within 2 float32 ulps of the midpoint between two operand values is taken rounded the
way the device has it (front_layer_cases.tie_resolved); every figure line says how many there were.  The bars are not touched.

Encoder taps are compared on the rows below the length (the LayerNorm outputs behind it are arbitrary by design; that they do not leak is
tests/test_gpu_front.py's); "z_p", "flow<f>" and z on every row, and must be exactly 0 at or beyond the length.

The coarse end-to-end checks stay where they were (tests/test_gpu_front.py: 5e-3 RMS on z, five taps at 2e-3 - 5e-3).
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import front_layer_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu


def _within_bars(r):
    """Prints every segment's figures, then asserts both bars of every segment."""
    print("\n%s: forms %s (observed: %s; as computed only: %s) kernels %s" % (r["case"], r["forms"], r["forms_observed"], r["forms_computed_only"], r["kernels"]))
    bad = []
    for e in r["segments"]:
        print("  %-7s HIP vs f64 oracle RMS %.3e max %.3e = %s x floor_rms, %s x floor_max (own floor %.3e / %.3e, floor used %.3e / %.3e, bars %.3e / %.3e)%s" % (
            e["segment"], e["rms"], e["max"], "%.2f" % e["rms_ratio"] if e["rms_ratio"] is not None else "-",
            "%.2f" % e["max_ratio"] if e["max_ratio"] is not None else "-", e["floor_rms"], e["floor_max"], e["eff_rms"], e["eff_max"], e["bar_rms"], e["bar_max"],
            " near-ties of the hidden activation: %d, %d rounded away from nearest" % (e["ties"], e["ties_flipped"]) if e["ties"] else ""))
        if not e["within_bars"]:
            bad.append("%s: RMS %.3e (bar %.3e) max %.3e (bar %.3e)" % (e["segment"], e["rms"], e["bar_rms"], e["max"], e["bar_max"]))
    assert not bad, "%s: %s" % (r["case"], "; ".join(bad))


@pytest.mark.parametrize("c", fc.TABLE, ids=fc.case_id)
def test_every_segment_against_its_rounded_fp64_oracle(c, gpu):
    _within_bars(fc.device_case(c, gpu)[0])


@pytest.mark.parametrize("c", fc.BATCH_CASES, ids=fc.case_id)
def test_batch_items_are_their_single_clips(c, gpu):
    """Forms pinned: an item of the batch is the same clip run alone, bit for bit, on the rows it has."""
    r, z, fr = fc.device_case(c, gpu)
    _within_bars(r)
    x = fc.inputs(c)
    assert not torch.equal(z[0], z[1])
    for b in range(c.B):
        one = fr(x["phone"][b:b + 1].to(gpu), x["pitch"][b:b + 1].to(gpu), x["lengths"][b:b + 1].to(gpu), x["g"][b:b + 1].to(gpu), c.fh,
                 noise=x["noise"][b:b + 1].to(gpu)).cpu()
        assert torch.equal(one[0], z[b]), "item %d differs from its single-clip call: rms %.3e" % (b, fc.err(one[0], z[b])[0])


def test_wn_channel_split_is_the_one_launch_form_bit_for_bit(gpu):
    """FR_WN_SPLIT = 1 (gate + res_skip launches, channel pairs over 3x the blocks) against 0 (k_fr_wn): the same K loops and epilogues, every flow tap and z
    bit-equal -- at a tile edge, ragged."""
    base = fc.Case("wn-split", 2, 33, lengths=(33, 20), opts=fc.O(FR_NJ=1, FR_FFN_SPLIT=1, FR_WN_SPLIT=0), segments=fc.FLOW)
    r0, z0, fr = fc.device_case(base, gpu)
    x = fc.inputs(base)
    args = tuple(x[k].to(gpu) for k in ("phone", "pitch", "lengths", "g"))
    taps0 = {f: fr.debug_tap("flow%d" % f, *args, 0, noise=x["noise"].to(gpu)) for f in range(4)}
    r1, z1, fr1 = fc.device_case(base._replace(name="wn-split1", opts=fc.O(FR_NJ=1, FR_FFN_SPLIT=1, FR_WN_SPLIT=1)), gpu)
    _within_bars(r0)
    _within_bars(r1)
    assert r0["forms_observed"]["wn"] == "one_launch" and r1["forms_observed"]["wn"] == "two_launches"
    for f in range(4):
        assert torch.equal(taps0[f], fr1.debug_tap("flow%d" % f, *args, 0, noise=x["noise"].to(gpu))), "flow%d differs between FR_WN_SPLIT 0 and 1" % f
    assert torch.equal(z0, z1)
