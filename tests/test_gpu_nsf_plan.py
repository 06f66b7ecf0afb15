"""``rvcmi_nsf_last_plan`` / ``gen.last_plan()`` (include/rvcmi.h): a forward keeps, per stage it reached, the record of how it ran the stage's
ResBlocks -- written by the forward from the values it launched with.  What the records must say is worked out here from the planner's documented
rules (tests/nsf_cases.py: ``expected_paths``, ``full_tile_counts``, ``pair_tile_counts``), never read back from the library.  All cases are v2_48k
(k = 11, 7, 3; stages of C = 256, 128, 64, 32 with 12, 120, 240, 480 rows per frame)."""
import ctypes as C
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nsf_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

CFG = nc.CONFIGS["v2_48k"]


def _gen(c, gpu):
    import rvc_amd

    x, w = nc.inputs(c), nc.weights(c.cfg, c.seed, c.wgain)
    gen = rvc_amd.NSFGeneratorHIP(vars(CFG), w, device=gpu, operand=c.operand, max_B=c.B, max_T=c.T)
    for k, v in c.opts:
        gen.set_option(k, v)
    args = (x["z"].to(gpu), x["f0"].to(gpu), x["g"].to(gpu))
    noise = x["noise"].to(gpu)
    return gen, (lambda: gen(*args, noise=noise).cpu()), (lambda what: gen.debug_tap(what, *args, noise=noise))


def _tiles(r):
    return dict(zip(r["k"], r["tiles"]))


def test_default_plan_a_tap_and_a_fresh_handle(gpu):
    """B = 1, T = 24 with no option: SPLIT, SPLIT, FULL 256, FULL 256 with the tile counts of the 256-row class; a forward that ended at the "up1" tap
    reports two stages (of stage 1, whose ResBlocks did not run, no tiles), the next plain forward four again; before any forward: nothing"""
    c = nc.Case("v2_48k", 1, 24, 500)
    gen, run, tap = _gen(c, gpu)
    assert gen.last_plan() == []
    wave = run()
    plan = gen.last_plan()
    rows = nc.stage_rows(CFG, c.T)
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert [(r["path"], r["C"], r["B"], r["rows"], r["num_cus"]) for r in plan] == [
        ("SPLIT", 256, 1, rows[0], ncu), ("SPLIT", 128, 1, rows[1], ncu), ("FULL", 64, 1, rows[2], ncu), ("FULL", 32, 1, rows[3], ncu)], plan
    assert [(r["x0_half"], r["y_half"]) for r in plan] == [(False, False), (False, False), (True, True), (True, True)]
    for r in plan[:2]:
        assert (r["tile_rows"], r["n_rb"], r["k"], r["tiles"], r["pair_streamed"]) == (0, 0, [], [], 0), r
    for r, L in zip(plan[2:], rows[2:]):
        assert (r["tile_rows"], r["tile_waves"], r["k"]) == (256, 4, [11, 7, 3]) and _tiles(r) == nc.full_tile_counts(CFG, L, 256), r
    up1 = tap("up1")
    assert up1.shape == (1, 128, rows[1])
    tapped = gen.last_plan()
    assert len(tapped) == 2 and tapped[0] == plan[0] and tapped[1] == plan[1], tapped
    assert torch.equal(run(), wave) and gen.last_plan() == plan


def test_forced_stream_reports_its_strips(gpu):
    """T = 2 with RB_STREAM = 1: stage 1 (240 rows at C = 128) on the streaming kernel, three jobs, whose strips cover the rows"""
    c = nc.Case("v2_48k", 1, 2, 501, nc.STREAM)
    gen, run, _ = _gen(c, gpu)
    run()
    r = gen.last_plan()[1]
    L = nc.stage_rows(CFG, c.T)[1]
    assert (r["path"], r["C"], r["rows"], r["n_rb"], r["k"]) == ("STREAM", 128, L, 3, [11, 7, 3]), r
    assert len(r["tiles"]) == len(r["strip_len"]) == 3 and all(n >= 1 and n * s >= L for n, s in zip(r["tiles"], r["strip_len"])), r
    assert (r["stream_nj"], r["stream_mfma"], r["stream_fill_skip"], r["x0_half"], r["y_half"]) == (6, 16, True, True, True), r
    r0 = gen.last_plan()[0]  # (stage 0, C = 256: pair by pair, every level taken by the forced streaming kernel)
    assert (r0["path"], r0["pair_streamed"]) == ("PAIR", 0b111), r0


def test_pair_reports_its_tiles(gpu):
    """T = 10 with RB_STREAM = 0 and NO_RB_SPLIT = 1: stage 0 (120 rows at C = 256) pair by pair on k_rb_pair, ceil(L / (128 - (k - 1))) tiles"""
    c = nc.Case("v2_48k", 1, 10, 502, nc.PAIR)
    gen, run, _ = _gen(c, gpu)
    run()
    r = gen.last_plan()[0]
    L = nc.stage_rows(CFG, c.T)[0]
    assert (r["path"], r["C"], r["rows"], r["tile_rows"], r["pair_streamed"], r["x0_half"], r["y_half"]) == ("PAIR", 256, L, 128, 0, False, False), r
    assert _tiles(r) == {k: -(-L // (128 - (k - 1))) for k in (11, 7, 3)} == nc.pair_tile_counts(CFG, L), r


def test_too_small_a_capacity_is_an_error_and_writes_nothing(gpu):
    from rvc_amd import _lib

    c = nc.Case("v2_48k", 1, 2, 503)
    gen, run, _ = _gen(c, gpu)
    run()
    buf, n = (_lib.NsfStagePlan * 4)(), C.c_int(-7)
    C.memset(buf, 0xA5, C.sizeof(buf))
    before = bytes(buf)
    for cap in (3, 0, -1):
        assert _lib.lib().rvcmi_nsf_last_plan(gen._handle, buf, cap, C.byref(n)) == -1  # RVCMI_ERR_INVALID
        assert b"capacity" in _lib.lib().rvcmi_last_error()
        assert bytes(buf) == before and n.value == -7
    assert _lib.lib().rvcmi_nsf_last_plan(gen._handle, buf, 4, C.byref(n)) == 0 and n.value == 4
    assert [_lib.RB_PATHS[r.path] for r in buf] == ["SPLIT", "SPLIT", "FULL", "FULL"]
