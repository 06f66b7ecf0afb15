"""The GUI's input gate on the device (``rvcmi_glue_input_gate_batch`` / ``glue.input_gate_batch``) against
``realtime.input_gate`` per session: output rows and updated buffers bit for bit over three consecutive blocks (the state carries), rows
that are tails of longer strided buffers, silence, the 80 dB clip and a NaN."""
import functools

import numpy as np
import pytest
import torch

import input_gate_cases as gc

pytestmark = pytest.mark.gpu

GEOMETRIES = ((160, 160), (160, 480), (441, 2205), (480, 12000))
HEAD, PAD = 37, 11   # samples in front of every destination row / behind every row of the other buffers


def _draw(S, zc, blk, threhold, seed):
    """(the rms buffers before the first block [S, 4 zc], [3 blocks][S, blk]).  The buffers start filled, as in a running stream: from zeros a
    session's first calls are all-quiet or all-kept whatever the block (every frame of a short block then sees the same loud hop).  Session 0 levels around the threshold; session 1 (if any) digital silence in block 0, then levels; session 2 one
    loud sample in block 1 (the 80 dB clip keeps all its frames) and a NaN in block 2."""
    rng = np.random.default_rng(seed)
    buf0 = np.stack([gc.stretches(rng, 4 * zc, zc, threhold) for _ in range(S)])
    if S > 1:
        buf0[1] = 0
    out = []
    for b in range(3):
        rows = [gc.stretches(rng, blk, zc, threhold) for _ in range(S)]
        if S > 1 and b == 0:
            rows[1][:] = 0
        if S > 2 and b == 1:
            rows[2][blk // 2] = np.float32(gc.loud_value(threhold))
        if S > 2 and b == 2:
            rows[2][blk // 3] = np.float32("nan")
        out.append(np.stack(rows))
    return buf0, out


def _host(S, zc, threhold, buf0, blocks):
    """The host oracle over the blocks: per block (want [S, blk + 2 zc], buffers after it [S, 4 zc], frames zeroed, frames kept); the frame
    counts restate the oracle's own decision (``amplitude_to_db(frame_rms_np(...)[2:]) < threhold``)."""
    from rvc_amd.realtime import amplitude_to_db, frame_rms_np, input_gate

    buf, out = buf0.copy(), []
    for x in blocks:
        quiet = np.stack([amplitude_to_db(frame_rms_np(np.append(buf[s], x[s]), 4 * zc, zc)[2:]) < threhold for s in range(S)])
        want = np.stack([input_gate(x[s].copy(), buf[s], zc, threhold) for s in range(S)])
        out.append((want, buf.copy(), int(quiet.sum()), int((~quiet).sum())))
    return out


@functools.lru_cache(maxsize=None)
def _case(S, zc, blk, threhold):
    """The first seed (a fixed search order) whose blocks, by the HOST oracle alone, make every call zero at least one frame and keep at
    least one -> (blocks, what the host gate gives)."""
    for seed in range(1000 * zc + blk, 1000 * zc + blk + 400):
        buf0, blocks = _draw(S, zc, blk, threhold, seed)
        host = _host(S, zc, threhold, buf0, blocks)
        if all(z > 0 and k > 0 for _, _, z, k in host):
            return buf0, blocks, host
    raise AssertionError("no seed gives blocks on both sides of the gate")


@pytest.mark.parametrize("threhold", [-55, -40, -20])
@pytest.mark.parametrize("zc,blk", GEOMETRIES)
@pytest.mark.parametrize("S", [1, 3])
def test_device_gate_equals_the_host_gate(S, zc, blk, threhold, gpu):
    import rvc_amd
    from rvc_amd.realtime import input_gate_cutoffs

    m = blk + 2 * zc
    cuts = input_gate_cutoffs(threhold)
    buf0, blocks, host = _case(S, zc, blk, threhold)
    big_dst = torch.full((S, HEAD + m), 7.0, device=gpu)
    big_buf = torch.full((S, 4 * zc + PAD), 7.0, device=gpu)
    big_buf[:, : 4 * zc] = torch.from_numpy(buf0).to(gpu)
    dst, dev_buf = big_dst[:, HEAD:], big_buf[:, : 4 * zc]
    assert S == 1 or not dst.is_contiguous()
    for b, (x, (want, want_buf, zeroed, kept)) in enumerate(zip(blocks, host)):
        assert zeroed > 0 and kept > 0   # by the host oracle, the call zeroes at least one frame and keeps at least one
        big_x = torch.full((S, blk + PAD), 7.0, device=gpu)
        big_x[:, :blk] = torch.from_numpy(x).to(gpu)
        got = rvc_amd.glue.input_gate_batch(big_x[:, :blk], dev_buf, dst, zc, *cuts)
        assert got is dst
        assert np.array_equal(dst.cpu().numpy(), want, equal_nan=True), "block %d: %d samples differ" % (b, int((dst.cpu().numpy() != want).sum()))
        assert np.array_equal(dev_buf.cpu().numpy(), want_buf, equal_nan=True), "block %d: the rms buffers differ" % b
        assert bool((big_dst[:, :HEAD] == 7.0).all()) and bool((big_buf[:, 4 * zc:] == 7.0).all())   # heads and pads untouched


def test_the_clip_and_the_nan_keep_every_frame(gpu):
    """The special sessions do what they are there for: with the loud sample in the block no frame of that session is zeroed although most
    are below the threshold; with the NaN likewise."""
    import rvc_amd
    from rvc_amd.realtime import input_gate, input_gate_cutoffs

    zc, blk, threhold = 160, 1600, -40
    rng = np.random.default_rng(5)
    quiet = (rng.standard_normal((3, blk)) * gc.level(threhold - 10)).astype(np.float32)
    quiet[1, 700] = np.float32(gc.loud_value(threhold))
    quiet[2, 900] = np.float32("nan")
    dst = torch.empty(3, blk + 2 * zc, device=gpu)
    buf = torch.zeros(3, 4 * zc, device=gpu)
    rvc_amd.glue.input_gate_batch(torch.from_numpy(quiet).to(gpu), buf, dst, zc, *input_gate_cutoffs(threhold))
    want = np.stack([input_gate(quiet[s].copy(), np.zeros(4 * zc, np.float32), zc, threhold) for s in range(3)])
    assert np.array_equal(dst.cpu().numpy(), want, equal_nan=True)
    assert (want[0] == 0).all() and (want[1][2 * zc:] != 0).all() and np.array_equal(want[2][2 * zc:], quiet[2], equal_nan=True)


def test_rejections(gpu):
    import rvc_amd
    from rvc_amd import _lib

    L, st = _lib.lib(), _lib.stream_ptr(gpu)
    x, buf, dst, scratch = torch.zeros(2, 500, device=gpu), torch.zeros(2, 640, device=gpu), torch.full((2, 900), 7.0, device=gpu), torch.zeros(4096, device=gpu)
    p = _lib.ptr
    with torch.cuda.device(gpu):
        assert L.rvcmi_glue_input_gate_batch(2, p(x), 500, p(buf), 640, p(dst), 900, 160, 480, 1e-3, 10.0, p(scratch), st) == 0
        dst.fill_(7.0)
        for zc, blk in ((160, 500), (160, 80), (0, 160)):            # blk % zc != 0, blk < zc, zc < 1
            assert L.rvcmi_glue_input_gate_batch(2, p(x), 500, p(buf), 640, p(dst), 900, zc, blk, 1e-3, 10.0, p(scratch), st) == _lib.ERR_INVALID
        assert L.rvcmi_glue_input_gate_batch(0, p(x), 500, p(buf), 640, p(dst), 900, 160, 480, 1e-3, 10.0, p(scratch), st) == _lib.ERR_INVALID
        assert L.rvcmi_glue_input_gate_batch(2, p(x), 500, p(buf), 639, p(dst), 900, 160, 480, 1e-3, 10.0, p(scratch), st) == _lib.ERR_INVALID
        assert L.rvcmi_glue_input_gate_batch(2, p(x), 500, p(buf), 640, p(dst), 799, 160, 480, 1e-3, 10.0, p(scratch), st) == _lib.ERR_INVALID
        assert L.rvcmi_glue_input_gate_batch(2, p(x), 500, p(buf), 640, p(dst), 900, 160, 480, float("nan"), 10.0, p(scratch), st) == _lib.ERR_INVALID
    torch.cuda.synchronize(gpu)
    assert bool((dst == 7.0).all())
    assert L.rvcmi_glue_input_gate_scratch_floats(160, 500) == 0 and L.rvcmi_glue_input_gate_scratch_floats(160, 480) == 640 + 480 + 8
    for blk in (500, 80):
        with pytest.raises(_lib.RvcmiError) as e:
            rvc_amd.glue.input_gate_batch(torch.zeros(2, blk, device=gpu), buf, torch.zeros(2, blk + 320, device=gpu), 160, 1e-3, 10.0)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(ValueError):
        rvc_amd.glue.input_gate_batch(x[:, :480], buf, dst[:, :799], 160, 1e-3, 10.0)
