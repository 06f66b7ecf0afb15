"""k_rb_full at C <= 32 (csrc/rb_full_kernels.hpp, nsf.hip): two changes of what the kernel executes, neither of what it computes, so every check here is
BIT-equality between two code paths on the same device, inputs and handle.

* Real taps only.  A k-group of the K loop holds 2 taps at C = 32 and 4 at C = 16, and k = 11 / 7 / 3 is packed as 12 / 8 / 4 taps; the default loop
  leaves the last group behind the real taps, option RBF_PAD_TAP = 1 keeps the padded loop.  The skipped products are exact zeros, so the only
  difference the addend can make is -0.0 against +0.0, which ``torch.equal`` counts as equal.
* The 768-row tile class of C = 32 (option RBF32_TALL: 1 always, 0 never, absent = from 4 x num_cus() blocks of 768 rows on).  A taller tile changes
  no element's summation order.  Which class ran is reported by the forward whose output is compared (``gen.last_plan()``), as tests/nsf_cases.py does.

The parity yardstick stays tests/test_gpu_nsf_layers.py and the goldens.
"""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nsf_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu

RBF32T_ROWS = 768


def _gen(c, gpu):
    import rvc_amd

    cfg, x, w = nc.CONFIGS[c.cfg], nc.inputs(c), nc.weights(c.cfg, c.seed, c.wgain)
    gen = rvc_amd.NSFGeneratorHIP(vars(cfg), w, device=gpu, operand=c.operand, max_B=c.B, max_T=c.T)
    args = (x["z"].to(gpu), x["f0"].to(gpu), x["g"].to(gpu))
    noise = x["noise"].to(gpu)
    return gen, (lambda: gen(*args, noise=noise).cpu()), (lambda what: gen.debug_tap(what, *args, noise=noise))


def _stage3(gen, run):
    """-> (the waveform of a plain forward, the tile rows and {k: tiles} that forward reports for stage 3: k_rb_full at C = 32)"""
    wave = run()
    r = gen.last_plan()[3]
    assert (r["path"], r["C"]) == ("FULL", 32), r
    return wave, r["tile_rows"], dict(zip(r["k"], r["tiles"]))


@pytest.mark.parametrize("operand", ("fp16", "bf16"))
@pytest.mark.parametrize("T", (24, 55))
def test_real_taps_equal_the_padded_loop_c32(T, operand, gpu):
    """v2_48k stage 3 (C = 32): T = 24 runs on the 256-row class, T = 55 on the 384-row class with several tiles per kernel size"""
    c = nc.Case("v2_48k", 1, T, 200 + T, operand=operand)
    gen, run, tap = _gen(c, gpu)
    wave, rows, tiles = _stage3(gen, run)
    L = nc.stage_rows(nc.CONFIGS[c.cfg], T)[3]
    assert rows == (256 if T == 24 else 384) and tiles == nc.full_tile_counts(nc.CONFIGS[c.cfg], L, rows), (rows, tiles)
    got = {"stage3": tap("stage3"), "wave": wave}
    gen.set_option("RBF_PAD_TAP", 1)
    want = {"stage3": tap("stage3"), "wave": run()}
    gen.set_option("RBF_PAD_TAP", None)
    for k in got:
        assert bool(torch.isfinite(got[k]).all()) and got[k].abs().max() > 0
        assert torch.equal(got[k], want[k]), "%s: real taps differ from the padded loop, max %.3e" % (k, nc.err(got[k], want[k])[1])
    assert torch.equal(run(), got["wave"])  # (the default is back)


@pytest.mark.parametrize("T", (3, 16))
def test_real_taps_equal_the_padded_loop_c32_and_c16(T, gpu):
    """v1_32k: stage 3 is C = 32 (two taps per k-group), stage 4 is C = 16 (four)"""
    c = nc.Case("v1_32k", 1, T, 210 + T)
    gen, run, tap = _gen(c, gpu)
    gen.profile(True)
    run()
    names = {s["name"] for s in gen.profile_read()}
    gen.profile(False)
    assert {"rb_full_c32", "rb_full_c16"} <= names, sorted(names)
    got = {"stage3": tap("stage3"), "stage4": tap("stage4"), "wave": run()}
    gen.set_option("RBF_PAD_TAP", 1)
    want = {"stage3": tap("stage3"), "stage4": tap("stage4"), "wave": run()}
    for k in got:
        assert bool(torch.isfinite(got[k]).all()) and got[k].abs().max() > 0
        assert torch.equal(got[k], want[k]), "%s: real taps differ from the padded loop, max %.3e" % (k, nc.err(got[k], want[k])[1])


@pytest.mark.parametrize("T", (1, 2, 3))
def test_tall_tiles_equal_the_default_class(T, gpu):
    """RBF32_TALL = 1 at 480 rows (the sequence ends inside the first 768-row tile), 960 (two k = 11 tiles, the second mostly beyond the end) and 1 440
    (three k = 11 tiles, two k = 3 tiles)"""
    c = nc.Case("v2_48k", 1, T, 220 + T)
    cfg = nc.CONFIGS[c.cfg]
    gen, run, tap = _gen(c, gpu)
    gen.set_option("RBF32_TALL", 0)
    want = {"stage3": tap("stage3")}
    want["wave"], rows0, tiles0 = _stage3(gen, run)
    gen.set_option("RBF32_TALL", 1)
    got = {"stage3": tap("stage3")}
    got["wave"], rows, tiles = _stage3(gen, run)
    assert (rows0, rows) == (nc.RBF_SMALL_ROWS, RBF32T_ROWS)
    L = nc.stage_rows(cfg, T)[3]
    halo = {k: nc._rbf_halo(k, d) for k, d in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)}
    assert halo == {3: 12, 7: 36, 11: 60}
    assert tiles == {k: -(-L // (RBF32T_ROWS - 2 * h)) for k, h in halo.items()}, tiles
    assert tiles0 == nc.full_tile_counts(cfg, L, nc.RBF_SMALL_ROWS), tiles0  # (a launch this short: the 256-row class when the tall one is off)
    assert tiles != tiles0
    for k in got:
        assert bool(torch.isfinite(got[k]).all()) and got[k].abs().max() > 0
        assert torch.equal(got[k], want[k]), "%s: 768-row tiles differ from the default class, max %.3e" % (k, nc.err(got[k], want[k])[1])


def test_tall_tiles_ragged_batch(gpu):
    """B = 2, items of 3 and 1 frames: item 1 ends inside the first tile, whose two later k = 11 tiles hold no row of it"""
    import rvc_amd

    cfg = nc.CONFIGS["v2_48k"]
    lens, T = (3, 1), 3
    c = nc.Case("v2_48k", 2, T, 230)
    x, w = nc.inputs(c), nc.weights(c.cfg, c.seed)
    gen = rvc_amd.NSFGeneratorHIP(vars(cfg), w, device=gpu, operand="fp16", max_B=2, max_T=T)
    Z, F, G, N = x["z"].to(gpu).clone(), x["f0"].to(gpu), x["g"].to(gpu), x["noise"].to(gpu)
    for b, n in enumerate(lens):
        Z[b, :, n:] = 0
    outs = {}
    for tall in (1, 0):
        gen.set_option("RBF32_TALL", tall)
        out = outs[tall] = gen(Z, F, G, noise=N, lengths=torch.tensor(lens)).cpu()
        assert out.shape == (2, 1, T * cfg.upp) and bool(torch.isfinite(out).all())
        for b, n in enumerate(lens):
            one = gen(Z[b:b + 1, :, :n].contiguous(), F[b:b + 1, :n].contiguous(), G[b:b + 1].contiguous(),
                      noise=N[b:b + 1, :n * cfg.upp].contiguous()).cpu()
            assert one.abs().max() > 0
            assert torch.equal(one[0, 0], out[b, 0, :n * cfg.upp]), "RBF32_TALL = %d: item %d differs from its single-item call" % (tall, b)
            assert not out[b, 0, n * cfg.upp:].any(), "RBF32_TALL = %d: rows behind the end of item %d are not zero" % (tall, b)
    assert torch.equal(outs[0], outs[1])


def test_tall_tiles_auto_rule(gpu):
    """plan_stage restated: the 768-row class from 4 x num_cus() blocks on.  T = 80 (38 400 rows at stage 3) is 60 + 56 + 52 = 168 blocks of 768 rows:
    with no option set the 384-row class stays, and RBF32_TALL = 1 reports the other class and other counts"""
    c = nc.Case("v2_48k", 1, 80, 240)
    cfg = nc.CONFIGS[c.cfg]
    gen, run, _ = _gen(c, gpu)
    L = nc.stage_rows(cfg, c.T)[3]
    ncu = torch.cuda.get_device_properties(gpu).multi_processor_count
    assert sum(nc.full_tile_counts(cfg, L, RBF32T_ROWS).values()) == 168 < 4 * ncu
    wave, rows, tiles = _stage3(gen, run)
    assert rows == 384 and tiles == nc.full_tile_counts(cfg, L, 384), (rows, tiles)
    assert nc.expected_paths(cfg, c.B, c.T, c.opts, ncu)[3] == "FULL384"
    gen.set_option("RBF32_TALL", 1)
    wave_tall, rows_tall, tiles_tall = _stage3(gen, run)
    assert rows_tall == RBF32T_ROWS and tiles_tall == nc.full_tile_counts(cfg, L, RBF32T_ROWS) != tiles, (rows_tall, tiles_tall)
    assert torch.equal(wave, wave_tall)


@pytest.mark.parametrize("key", ("RBF32_TALL", "RBF_PAD_TAP"))
def test_option_values_other_than_0_and_1_are_rejected(key, gpu):
    import rvc_amd

    c = nc.Case("v2_48k", 1, 2, 250)
    gen, run, _ = _gen(c, gpu)
    wave = run()
    for bad in (2, -1, 0.5):
        with pytest.raises(rvc_amd._lib.RvcmiError):
            gen.set_option(key, bad)
    assert torch.equal(run(), wave)  # nothing was pinned by the refused calls
    for ok in (0, 1, None):
        gen.set_option(key, ok)
