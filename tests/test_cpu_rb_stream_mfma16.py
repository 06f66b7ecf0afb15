"""The lane maps of k_rb_stream on v_mfma_f32_16x16x32 (csrc/mfma_conv.hpp kconv16, csrc/rb_stream_kernels.hpp SH = 16), on the host model
tools/model_rb_stream_mfma16.py: what the K loop multiplies, which LDS slots its B reads touch, and that the lane-held tiles of the step schedule
(publish, T pick-up and deposit, residual shift by two tiles, two-tile carry, dual write, H tail, fill skip from tile 2 (m + 1)) give ResBlock1's rows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))

import model_rb_stream_mfma16 as model  # noqa: E402


def test_row_and_chunk_maps_are_permutations():
    assert sorted(model.mfma16_row(n) for n in range(16)) == list(range(16))
    assert sorted(model.mfma16_chunk(q) for q in range(4)) == list(range(4))
    # the A gather: 16 lanes of a K-block are one whole 256-byte run of the packed fragment
    for q in range(4):
        offs = [model.mfma16_loff(16 * q + n) for n in range(16)]
        assert offs == list(range(offs[0], offs[0] + 256, 16)) and offs[0] % 256 == 0


@pytest.mark.parametrize("k,dil", ((3, 1), (7, 3), (11, 5)))
def test_every_product_formed_exactly_once(k, dil):
    """every (output channel, input channel, tap) product of every output row, from the existing packed weight layout and the LDS image"""
    cnt = model.kloop_products(k, dil)
    assert cnt.shape == (32, model.R, model.C, k) and (cnt == 1).all()


def test_fill_skip_tiles_form_nothing():
    cnt = model.kloop_products(3, 1, jt0=4)
    assert (cnt[:, :64] == 0).all() and (cnt[:, 64:] == 1).all()


def test_b_reads_touch_16_distinct_slots_per_lane_group():
    groups = model.bank_slots()
    assert len(groups) == 11 * 4 * model.NT * 4
    for slots in groups:
        assert len(set(slots)) == 16, slots
    # the natural assignment (row = lane % 16, K-block = lane // 16 in channel order) does conflict: the check can fail
    assert all(len(set(slots)) < 16 for slots in model.bank_slots(natural=True))


@pytest.mark.parametrize("k", (3, 7, 11))
@pytest.mark.parametrize("L,strips", ((700, 2), (90, 1)))
def test_lane_held_schedule_reproduces_the_resblock(k, L, strips):
    """several strips of several steps, and one strip whose only step starts in front of the sequence; the fill-skip tiles of every first step are NaN"""
    got, ref = model.strip_case(k, [1, 3, 5], L, strips)
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() < 2e-4
