"""The quiet-point search that cuts a long input (infer/modules/vc/pipeline.py:219-236), host side: the fixtures of
tools/make_golden_cuts.py (the reference's own statements, executed) against the host restatement ``pipeline._cut_points``, the
host formula ``glue.cut_count``, and what the built library and ``glue.cut_points`` must do without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import cut_cases
from make_golden_cuts import sha, window_sums


@pytest.mark.parametrize("name", cut_cases.names())
def test_host_cut_points_reproduce_the_reference(name):
    """``_cut_points`` on every fixture case: the cuts, and the window sums bit for bit (their sha256; the stored sums where the
    fixture keeps them).  The expected values were produced by the reference's statements, not by this restatement."""
    import rvc_amd.pipeline as rp

    c = cut_cases.load(name)
    pad = np.pad(c.audio, (c.window // 2, c.window // 2), mode="reflect")
    assert rp._cut_points(c.state(), c.audio, pad) == c.opt_ts
    assert (len(c.opt_ts) > 0) == c.searched()
    if c.searched():
        audio_sum = np.zeros_like(c.audio)
        for i in range(c.window):
            audio_sum += np.abs(pad[i: i - c.window])
        sums = window_sums(audio_sum, (c.t_center, c.t_query), c.n)
        assert sums.size == sum(c.lengths())
        assert sha(sums) == c.sums_sha256
        if c.sums is not None:
            assert np.array_equal(sums.view(np.int64), c.sums.view(np.int64))


def test_the_fixture_holds_every_case_the_search_has():
    names = cut_cases.names()
    for geometry in ("q10_c60", "q6_c38", "q5_c30"):
        for secs in (70, 200, 305):
            assert "prod_%s_%ds" % (geometry, secs) in names
    for n in ("suite_50000", "order_sensitive", "zeros_in_tile", "zeros_straddle_tiles", "tie_first_and_last_tile", "min_at_first",
              "min_at_last", "at_threshold", "above_threshold", "just_above_t_center", "right_reflection", "subnormal"):
        assert n in names
    c = cut_cases.load("min_at_last")
    assert c.n < c.t_center * 2 + c.t_query  # its last search window is cut off by the end of the signal
    c = cut_cases.load("subnormal")
    quiet = np.abs(c.audio[3300:3700])
    assert 0 < quiet.min() and quiet.max() < np.finfo(np.float64).tiny


def test_the_order_sensitive_case_is_order_sensitive():
    """Every window of the period-160 signal holds the same values, so a sum that is only mathematically equal -- numpy's pairwise
    ``sum`` here -- picks another minimum.  If it did not, the fixture could not fail a kernel that adds in its own order."""
    c = cut_cases.load("order_sensitive")
    p = np.abs(np.pad(c.audio, (c.window // 2, c.window // 2), mode="reflect"))
    pairwise = np.lib.stride_tricks.sliding_window_view(p, c.window)[: c.n].sum(axis=1)
    t = c.t_center
    lo, hi = t - c.t_query, t + c.t_query
    assert np.allclose(pairwise[lo:hi], pairwise[lo], rtol=1e-12)  # equal up to rounding ...
    assert lo + int(np.argmin(pairwise[lo:hi])) != c.opt_ts[0]     # ... and a different argmin


def test_cut_count_is_the_length_of_the_reference_range():
    import rvc_amd

    for t_center in (1, 7, 160, 16000, 480000):
        for n in (0, 1, t_center - 1, t_center, t_center + 1, 2 * t_center, 2 * t_center + 1, 5 * t_center + 3, 19200000):
            assert rvc_amd.glue.cut_count(n, t_center) == len(range(t_center, n, t_center)), (n, t_center)
    assert rvc_amd.cut_count is rvc_amd.glue.cut_count and rvc_amd.cut_points is rvc_amd.glue.cut_points


def test_library_exports_the_entry_points_and_sizes_their_scratch():
    import rvc_amd

    L = rvc_amd._lib.lib()
    assert hasattr(L, "rvcmi_glue_cut_points") and hasattr(L, "rvcmi_glue_cut_points_scratch_bytes")
    assert {"rvcmi_glue_cut_points", "rvcmi_glue_cut_points_scratch_bytes"} <= {s[0] for s in rvc_amd._lib.SYMBOLS}
    sb = L.rvcmi_glue_cut_points_scratch_bytes
    assert sb(4880000, 160, 960000, 160000) == 5 * 313 * 16  # five cuts, ceil(320000 / 1024) tiles, a (double, int64) pair each
    assert sb(9000, 160, 4000, 1100) == 2 * 3 * 16
    assert sb(4000, 160, 4000, 1100) == 0                     # n <= t_center: no cut, no scratch
    for bad in ((9000, 161, 4000, 1100), (9000, 0, 4000, 1100), (9000, 1026, 4000, 1100), (160, 160, 100, 50), (9000, 160, 4000, 4001),
                (9000, 160, 0, 0), (9000, 160, 4000, 0), (-1, 160, 4000, 1100)):
        assert sb(*bad) == 0, bad
    # the call itself refuses them before it looks at a pointer or launches anything (so this runs without a GPU)
    null = C.c_void_p(None)
    for bad in ((9000, 161, 4000, 1100), (9000, 1026, 4000, 1100), (160, 160, 100, 50), (9000, 160, 4000, 4001)):
        n, w, tc, tq = bad
        assert L.rvcmi_glue_cut_points(null, n, w, tc, tq, null, 1 << 20, null, null, null) == rvc_amd._lib.ERR_INVALID, bad
    assert L.rvcmi_glue_cut_points(null, 9000, 160, 4000, 1100, null, 1, null, null, null) == rvc_amd._lib.ERR_INVALID  # 2 cuts, room for 1
    assert b"2 cuts" in L.rvcmi_last_error()


def test_cut_points_rejects_cpu_and_non_fp64_tensors():
    import rvc_amd

    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.glue.cut_points(torch.zeros(9000, dtype=torch.float64), 160, 4000, 1100)
    for dt in (torch.float32, torch.float16, torch.int64):  # a silent cast would change the sums
        with pytest.raises(TypeError):
            rvc_amd.glue.cut_points(torch.zeros(9000, dtype=dt), 160, 4000, 1100)
