"""The deep U-Net of the RMVPE f0 network and its head (rvc/f0/deepunet.py, e2e.py:21-29,44-46) on csrc/unet.hip.

  * every primitive bit for bit against torch fp32 on the CPU, on small-integer data for which every fp16 product and fp32 sum is exact (the
    one rounding left, the fp16 store, is applied to the reference too);
  * the whole network against the REAL reference's output (tests/golden/rmvpe_unet_*.npz, made by tools/make_golden_unet.py) and, at other
    sizes, against the functional evaluator of tests/unet_cases.py in fp32 on the CPU.  Tolerance: measured each run, not fixed -- torch's own
    ``.half()`` evaluation of the same network on the GPU (what the reference runs with ``is_half``) has an RMS and a max-abs error against
    that fp32 result; the HIP path's may be at most TWICE those (a different summation order, fp16 storage of the skip tensors);
  * every primitive of the full network on its own, fed the fp16 operands of the fp64 oracle with the kernel's rounding points
    (oracle/unet_oracle.py), against the elementwise bound and the flip share of tests/unet_cases.py; the skip tensors and the output of whole
    forwards against the same oracle at bars derived on the CPU (tests/test_cpu_unet.py);
  * determinism, the module swap, the realtime graph capture with the swap on, and the errors.
"""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import unet_cases as uc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# ---------------------------------------------------------------- primitives, bit for bit

def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


_op = uc.debug_op  # one primitive through ``rvcmi_unet_debug_op``: NCHW fp32 on the CPU in, NCHW fp32 on the CPU out


def _epilogue(y, scale, shift, relu, res):
    y = y * scale[None, :, None, None] + shift[None, :, None, None]
    if relu:
        y = F.relu(y)
    if res is not None:
        y = y + res
    return y


def _same(got, want_fp32, what):
    want = want_fp32.to(torch.float16).float()  # the fp16 store: the ONE rounding of the path (every sum before it is exact)
    assert torch.isfinite(got).all(), what + ": non-finite output (a pixel or channel was not written)"
    assert torch.equal(got, want), "%s: %d of %d values differ, max |d| %.4g" % (what, int((got != want).sum()), got.numel(), float((got - want).abs().max()))


@pytest.mark.parametrize("C,H,W,ksplit", [(16, 5, 7, 0), (32, 9, 6, 0), (64, 5, 7, 0), (64, 3, 4, 3), (512, 3, 4, 0), (512, 3, 4, 1), (512, 1, 4, 7),
                                          (16, 5, 7, 1), (32, 9, 6, 1), (64, 5, 7, 1), (16, 5, 14, 0), (16, 5, 14, 1), (32, 5, 14, 0), (32, 5, 14, 1),
                                          (128, 3, 4, 0), (128, 3, 4, 1), (256, 3, 4, 0), (256, 3, 4, 1)])
def test_conv3x3_is_exact(C, H, W, ksplit, gpu):
    """3x3 convolution + scale / shift + ReLU + residual (added AFTER the ReLU), B = 2, borders in both axes, tiles that do not divide the
    pixel count; the 512-channel cases with the forward's own K split, without one, and with an uneven one.  ``ksplit=1``: the fused epilogue
    with its residual inside k_unet_conv<1, 1> / <2, 1> / <2, 2> (at these sizes the forward's own choice, 0, is always a split for a 3x3 layer);
    W = 14: 140 pixels, two blocks along the pixels for C = 16 and 32, the second one partial; C = 128 / 256: two / four blocks along the
    channels."""
    g = torch.Generator().manual_seed(C + 7 * H + ksplit)
    x, w, res = _ints(g, (2, C, H, W), -3, 3), _ints(g, (C, C, 3, 3), -2, 2), _ints(g, (2, C, H, W), -4, 4)
    scale, shift = 2.0 ** -_ints(g, (C,), 3, 5), _ints(g, (C,), -3, 3)
    want = _epilogue(F.conv2d(x, w, padding=1), scale, shift, True, res)
    assert float((want - shift[None, :, None, None] - res).abs().max()) > 4, "the case would not see a wrong convolution"
    _same(_op(gpu, 0, x, None, res, w, scale, shift, True, C, want.shape, ksplit), want, "conv3x3 C=%d" % C)


def test_first_layer_applies_the_input_batchnorm_before_the_zero_padding(gpu):
    """Cin = 1 behind ``Encoder.bn``: the border taps must see 0, not the BatchNorm's shift; and the 1x1 shortcut of the same unit."""
    g = torch.Generator().manual_seed(3)
    x = _ints(g, (2, 1, 6, 9), -6, 6)
    v = x * 0.5 + 3.0
    w, scale, shift = _ints(g, (16, 1, 3, 3), -2, 2), 2.0 ** -_ints(g, (16,), 0, 2), _ints(g, (16,), -3, 3)
    want = _epilogue(F.conv2d(v, w, padding=1), scale, shift, True, None)
    wrong = _epilogue(F.conv2d(x * 0.5, w, padding=1) + 3.0 * w.sum((1, 2, 3))[None, :, None, None], scale, shift, True, None)
    assert not torch.equal(want, wrong)  # (the folded-shift variant differs on the border)
    _same(_op(gpu, 4, x, None, None, w, scale, shift, True, 16, want.shape, in_scale=0.5, in_shift=3.0), want, "first 3x3")
    w1, b1 = _ints(g, (16, 1, 1, 1), -3, 3), _ints(g, (16,), -3, 3)
    want1 = F.conv2d(v, w1, b1)
    _same(_op(gpu, 5, x, None, None, w1, torch.ones(16), b1, False, 16, want1.shape, in_scale=0.5, in_shift=3.0), want1, "first 1x1")


@pytest.mark.parametrize("C0,C1,Cout,k", [(32, 0, 16, 1), (16, 16, 16, 1), (64, 64, 64, 3), (16, 16, 16, 3), (256, 256, 256, 1),
                                          (48, 48, 48, 3), (48, 48, 48, 1)])
def test_shortcut_and_two_source_read_are_exact(C0, C1, Cout, k, gpu):
    """The 1x1 shortcut with its bias, and a convolution over cat(a, b) read from the two tensors in place.  48 + 48: the second 32-channel
    chunk of K straddles the two tensors."""
    g = torch.Generator().manual_seed(C0 + C1 + k)
    a = _ints(g, (2, C0, 5, 6), -3, 3)
    b = _ints(g, (2, C1, 5, 6), -3, 3) if C1 else None
    w, bias = _ints(g, (Cout, C0 + C1, k, k), -2, 2), _ints(g, (Cout,), -3, 3)
    want = F.conv2d(torch.cat((a, b), 1) if C1 else a, w, bias, padding=k // 2) * 0.125
    got = _op(gpu, 1 if k == 1 else 0, a, b, None, w, torch.full((Cout,), 0.125), bias * 0.125, False, Cout, want.shape)
    _same(got, want, "%dx%d over %d + %d channels" % (k, k, C0, C1))
    if C1:  # the second source is really read: swapping the two changes the result
        assert not torch.equal(want, F.conv2d(torch.cat((b, a), 1), w, bias, padding=k // 2) * 0.125)


def test_pool_is_exact(gpu):
    g = torch.Generator().manual_seed(5)
    x = _ints(g, (2, 48, 6, 10), -9, 9)
    want = F.avg_pool2d(x, (2, 2))
    _same(_op(gpu, 3, x, None, None, None, None, None, False, 48, want.shape), want, "pool")


@pytest.mark.parametrize("Cin,Cout,H,W,ksplit", [(32, 16, 3, 5, 0), (64, 32, 4, 4, 1), (512, 256, 1, 4, 0), (128, 64, 2, 3, 5),
                                                 (32, 16, 3, 1, 0), (64, 32, 2, 1, 1)])
def test_transposed_convolution_is_exact(Cin, Cout, H, W, ksplit, gpu):
    """ConvTranspose2d(3x3, stride 2, padding 1, output_padding 1), weight [Cin, Cout, 3, 3], as four output phases + scale / shift + ReLU.
    W = 1: every tap at x + 1 falls outside the image."""
    g = torch.Generator().manual_seed(Cin + H)
    x, w = _ints(g, (2, Cin, H, W), -3, 3), _ints(g, (Cin, Cout, 3, 3), -2, 2)
    scale, shift = 2.0 ** -_ints(g, (Cout,), 2, 4), _ints(g, (Cout,), -2, 2)
    want = _epilogue(F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1), scale, shift, True, None)
    assert want.shape[2:] == (2 * H, 2 * W)
    _same(_op(gpu, 2, x, None, None, w, scale, shift, True, Cout, want.shape, ksplit), want, "transposed convolution %d -> %d" % (Cin, Cout))


def test_head_writes_the_gru_layout_exactly(gpu):
    """Conv2d(16, 3, 3x3) + bias, written as fp32 [B, T, 3, 128]: the ``.transpose(1, 2).flatten(-2)`` of e2e.py:46."""
    g = torch.Generator().manual_seed(9)
    x, w, bias = _ints(g, (2, 16, 5, 128), -3, 3), _ints(g, (3, 16, 3, 3), -2, 2), _ints(g, (3,), -3, 3)
    want = F.conv2d(x, w, bias, padding=1)
    got = _op(gpu, 6, x, None, None, w, torch.ones(3), bias, False, 3, want.shape, head=True)
    assert torch.equal(got, want)


# ---------------------------------------------------------------- every layer against the fp16-operand fp64 oracle

@pytest.mark.parametrize("ksplit", [0, 1])
def test_every_primitive_teacher_forced_against_the_oracle(ksplit, gpu):
    """Every primitive of the full network at (B, T) = (2, 32) -- both first-layer kernels, 3x3, 1x1, two-source reads, the five transposed
    convolutions, the five pools, the head -- fed the oracle's own fp16 operands, so that nothing has cascaded, against the unrounded fp64
    result: the elementwise bound and the flip share of tests/unet_cases.py (derived on the CPU, tests/test_cpu_unet.py).  Once with the
    forward's own K split at this size, once with the fused epilogue that long inputs run."""
    trace = uc.sweep_trace()
    assert len(trace) == 134
    bad, worst_flips, worst_excess = [], 0.0, 0.0
    for rec in trace:
        got = uc.run_record(gpu, rec, ksplit)
        if not torch.isfinite(got).all():
            bad.append("%s: non-finite output" % rec["name"])
            continue
        ck = uc.prim_check(got, rec)
        worst_flips, worst_excess = max(worst_flips, ck["flips"]), max(worst_excess, ck["excess"])
        if ck["violations"] or ck["flips"] > uc.FLIP_CAP:
            bad.append("%s (kind %d, %s): %d of %d outside the elementwise bound, flip share %.3e, excess %.3e A" % (
                rec["name"], rec["kind"], tuple(rec["y"].shape), ck["violations"], ck["n"], ck["flips"], ck["excess"]))
    print("unet sweep ksplit=%d: largest flip share %.3e (cap %.0e), largest excess %.3e A (gamma %.3e)" % (ksplit, worst_flips, uc.FLIP_CAP, worst_excess,
                                                                                                          uc.GAMMA))
    assert not bad, "%d of %d primitives:\n%s" % (len(bad), len(trace), "\n".join(bad))


@pytest.mark.parametrize("case", uc.WHOLE, ids=uc.case_id)
def test_whole_network_and_skips_against_the_rounded_oracle(case, gpu):
    """``rvcmi_unet_forward`` with the test's own workspace: the skip tensors it leaves there (``uc.skip_offsets``) and the head's output against
    the fp64 oracle with the kernel's rounding points, at the derived bars.  What the per-primitive sweep cannot see is held to account here:
    ``Loader::bn``, the weights' packing at create time, the buffer rotation of ``run()``."""
    want = uc.whole_case(case)
    got = uc.run_whole(gpu, case)
    assert sorted(got) == sorted(want)
    bad = []
    for k in sorted(want):
        b = want[k]
        assert got[k].shape == b["y"].shape, k
        rms, mx = uc.err(got[k], b["y"])
        print("unet %s %s: rms %.3e (floor %.3e, bar %.3e) max %.3e (floor %.3e, bar %.3e)" % (uc.case_id(case), k, rms, b["floor_rms"], b["bar_rms"], mx,
                                                                                            b["floor_max"], b["bar_max"]))
        if not (torch.isfinite(got[k]).all() and rms <= b["bar_rms"] and mx <= b["bar_max"]):
            bad.append("%s: rms %.3e against %.3e, max %.3e against %.3e" % (k, rms, b["bar_rms"], mx, b["bar_max"]))
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------- the whole network

def _err(got, ref):
    e = got.double() - ref.double()
    return float(e.pow(2).mean().sqrt()), float(e.abs().max())


def _hip_out(hip, mel, gpu):
    x = mel.to(gpu).transpose(-1, -2).unsqueeze(1)
    y = hip(x)
    return y.transpose(1, 2).flatten(-2)


def _parity(sd, mel, ref, gpu, tag):
    """-> (hip rms, hip max, half rms, half max); asserts the HIP path within twice the error of torch's own .half() path."""
    import rvc_amd

    hip = rvc_amd.UNetHIP.from_state_dict(sd, gpu)
    with torch.no_grad():
        got = _hip_out(hip, mel, gpu)
        assert got.is_contiguous() and got.dtype == torch.float32 and tuple(got.shape) == tuple(ref.shape)
        half = uc.forward(uc.to(sd, gpu, torch.float16), mel.to(gpu).half())
    torch.cuda.synchronize()
    (r, m), (hr, hm) = _err(got.cpu(), ref), _err(half.float().cpu(), ref)
    print("unet parity %s: HIP rms %.4e max %.4e | torch .half() rms %.4e max %.4e | ref rms %.4f" % (tag, r, m, hr, hm, float(ref.pow(2).mean().sqrt())))
    assert torch.isfinite(got).all() and hr > 0
    assert r <= 2 * hr and m <= 2 * hm, "%s: HIP rms %.4e max %.4e against twice torch .half()'s rms %.4e max %.4e" % (tag, r, m, hr, hm)
    return r, m, hr, hm


def test_full_network_matches_the_real_reference_T32(gpu):
    z = np.load(os.path.join(uc.GOLDEN, "rmvpe_unet_T32.npz"))
    sd = uc.seeded_weights(uc.golden_keys(), int(z["seed"]))
    _parity(sd, torch.from_numpy(z["mel"]), torch.from_numpy(z["out"]), gpu, "golden T32")


def test_reduced_network_matches_the_real_reference_T24(gpu):
    z = np.load(os.path.join(uc.GOLDEN, "rmvpe_unet_small_T24.npz"))
    keys = uc.key_list(levels=int(z["levels"]), blocks=int(z["blocks"]), inters=int(z["inters"]), base=int(z["base"]))
    _parity(uc.seeded_weights(keys, int(z["seed"])), torch.from_numpy(z["mel"]), torch.from_numpy(z["out"]), gpu, "golden small T24")


@pytest.mark.parametrize("B,T", [(1, 64), (2, 96), (1, 1024)])
def test_full_network_at_other_sizes(B, T, gpu):
    sd = uc.seeded_weights(uc.golden_keys(), 31 + T)
    mel = uc.seeded_mel(B, T, 100 + T)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        ref = uc.forward(sd, mel)
    _parity(sd, mel, ref, gpu, "full B=%d T=%d" % (B, T))


@pytest.mark.parametrize("levels,blocks,inters,base,B,T", [(2, 1, 1, 16, 1, 4), (2, 1, 1, 16, 2, 20), (3, 2, 2, 32, 1, 8), (3, 2, 2, 32, 2, 40),
                                                           (4, 1, 2, 16, 1, 48), (1, 2, 1, 48, 1, 6)])
def test_reduced_networks(levels, blocks, inters, base, B, T, gpu):
    sd = uc.seeded_weights(uc.key_list(levels, blocks, inters, base), 5 * levels + base)
    mel = uc.seeded_mel(B, T, T)
    with torch.no_grad():
        ref = uc.forward(sd, mel)
    _parity(sd, mel, ref, gpu, "reduced %d/%d/%d/%d B=%d T=%d" % (levels, blocks, inters, base, B, T))


def test_two_forwards_are_bit_identical(gpu):
    import rvc_amd

    sd = uc.seeded_weights(uc.golden_keys(), 1)
    hip = rvc_amd.UNetHIP.from_state_dict(sd, gpu)
    for T in (32, 256):
        mel = uc.seeded_mel(1, T, 2)
        a = _hip_out(hip, mel, gpu).clone()
        torch.empty(1 << 22, device=gpu).normal_()  # (other memory behind the next call's workspace)
        b = _hip_out(hip, mel, gpu)
        assert torch.equal(a, b), "T = %d" % T


def test_workspace_sizes_are_those_of_the_planner_before_the_shared_carve(gpu):
    """``rvcmi_unet_workspace_bytes`` is ABI-visible.  The numbers are the full network's (5 levels, 4 units, 4 intermediate layers, base 16)
    worked by hand from the dry run's arithmetic: four full-size fp16 buffers, one skip tensor per level, then the largest split-K
    partial buffer, each part rounded up to 256 bytes.  Sizes depend on the row count only: (2, 64) and the packed [32, 96] agree."""
    import ctypes as C

    import rvc_amd
    from rvc_amd import _lib

    hip = rvc_amd.UNetHIP.from_state_dict(uc.seeded_weights(uc.golden_keys(), 1), gpu)
    L = _lib.lib()
    assert L.rvcmi_unet_workspace_bytes(hip._h, 1, 32) == hip.workspace_bytes(1, 32) == 1368064
    assert L.rvcmi_unet_workspace_bytes(hip._h, 2, 64) == 5472256
    assert L.rvcmi_unet_workspace_bytes_ragged(hip._h, 2, (C.c_int * 3)(0, 32, 128)) == 5472256


# ---------------------------------------------------------------- swap, graph, errors

def _standin(gpu, seed=11, half=False, keys=None, **kw):
    keys = keys or uc.golden_keys()
    m = uc.StandIn(keys, uc.seeded_weights(keys, seed), **kw).eval().to(gpu)
    return m.half() if half else m


@pytest.mark.parametrize("half,real", [(False, False), (True, False), (False, True), (True, True)])
def test_swap_and_restore(half, real, gpu):
    """``real``: the tree's leaves are real ``nn.Conv2d`` / ``BatchNorm2d`` / ``ConvTranspose2d`` modules, as in the reference's network (every
    torch convolution carries ``output_padding``; the recogniser must tell the transposed ones apart)."""
    import rvc_amd

    model = _standin(gpu, half=half, real_modules=real)
    keys = uc.golden_keys()
    sd = uc.seeded_weights(keys, 11)
    mel = uc.seeded_mel(1, 64, 3)
    orig_unet, orig_cnn = model.unet, model.cnn
    # torch's own results bit for bit need torch's deterministic kernels: MIOpen's convolutions differ in the last bits from run to run
    # (tests/test_gpu_gru.py notes the same), the native ones do not
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        ref = uc.forward(sd, mel)
        x = mel.to(gpu).half() if half else mel.to(gpu)
        before = model(x)
        assert torch.equal(before, model(x)), "torch's native kernels are not run-to-run deterministic here: the restore check below could not tell"
        assert rvc_amd.accelerate_rmvpe_unet(model) == 1 and isinstance(model.unet, rvc_amd.UNetHIP) and isinstance(model.cnn, torch.nn.Identity)
        assert rvc_amd.accelerate_rmvpe_unet(model) == 0  # (already swapped)
        assert not any(k.startswith("unet.") or k.startswith("cnn.") for k in model.state_dict())  # (the originals are kept unregistered)
        got = model(x)
        assert got.shape == before.shape and got.dtype == before.dtype and got.is_contiguous()
        halfp = uc.forward(uc.to(sd, gpu, torch.float16), mel.to(gpu).half())
        (r, m), (hr, hm) = _err(got.float().cpu(), ref), _err(halfp.float().cpu(), ref)
        print("swap half=%s: HIP rms %.4e max %.4e | torch .half() rms %.4e max %.4e" % (half, r, m, hr, hm))
        assert r <= 2 * hr and m <= 2 * hm
        assert rvc_amd.restore_rmvpe_unet(model) == 1 and model.unet is orig_unet and model.cnn is orig_cnn
        assert [k for k in model.state_dict()] == [k for k, _ in keys]
        assert torch.equal(model(x), before)
        assert rvc_amd.restore_rmvpe_unet(model) == 0


def test_unsupported_and_cpu_models_are_left_alone(gpu):
    import rvc_amd

    keys = uc.golden_keys()
    cpu = uc.StandIn(keys).eval()
    assert rvc_amd.accelerate_rmvpe_unet(cpu) == 0 and isinstance(cpu.unet, uc._UNet)
    pooled_real = uc.StandIn(uc.key_list(2, 1, 1, 16), pool=(1, 2), real_modules=True).eval().to(gpu)
    assert rvc_amd.accelerate_rmvpe_unet(pooled_real) == 0 and isinstance(pooled_real.unet, uc._UNet)
    pooled = uc.StandIn(uc.key_list(2, 1, 1, 16), pool=(1, 2)).eval().to(gpu)
    assert rvc_amd.accelerate_rmvpe_unet(pooled) == 0 and isinstance(pooled.unet, uc._UNet)
    odd = uc.StandIn(uc.key_list(2, 1, 1, 24)).eval().to(gpu)
    assert rvc_amd.accelerate_rmvpe_unet(odd) == 0 and isinstance(odd.unet, uc._UNet)
    altered = [(k, (s[0], s[1], 1, 3) if k == "unet.encoder.layers.1.conv.0.conv.3.weight" else s) for k, s in uc.key_list(2, 1, 1, 16)]
    alt = uc.StandIn(altered).eval().to(gpu)
    assert rvc_amd.accelerate_rmvpe_unet(alt) == 0 and isinstance(alt.unet, uc._UNet)
    assert rvc_amd.accelerate_rmvpe_unet(torch.nn.Linear(4, 4).to(gpu)) == 0 and rvc_amd.accelerate_rmvpe_unet(object()) == 0


class _E2ELike(uc.StandIn):
    """The stand-in network with the recurrent tail of rvc/f0/e2e.py:31-35 behind it: mel [B, 128, T] -> salience [B, T, 360]."""

    def __init__(self, keys, sd):
        super().__init__(keys, sd, real_modules=True)
        torch.manual_seed(5)
        self.gru = torch.nn.GRU(384, 256, num_layers=1, batch_first=True, bidirectional=True)
        self.out = torch.nn.Linear(512, 360)

    def forward(self, mel):
        return torch.sigmoid(self.out(self.gru(super().forward(mel))[0]))


def _rmvpe_standin(gpu):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    from e2e_proxies import RmvpeProxy

    keys = uc.golden_keys()
    r = RmvpeProxy(gpu, half=True)
    r.model = _E2ELike(keys, uc.seeded_weights(keys, 21)).eval().to(gpu).half()
    return r


def test_switch_swaps_through_the_f0_helper_and_the_env_overrides_install(gpu, monkeypatch):
    import rvc_amd
    import rvc_amd.unet as ru
    from rvc_amd.gru import accelerate_f0_rmvpe

    monkeypatch.delenv("RVCMI_RMVPE_GRU", raising=False)
    monkeypatch.delenv("RVCMI_RMVPE_UNET", raising=False)
    r = _rmvpe_standin(gpu)
    assert accelerate_f0_rmvpe(r) == 1 and not hasattr(r, "_rvcmi_unet") and not isinstance(r.model.unet, rvc_amd.UNetHIP)  # default: off
    monkeypatch.setattr(ru, "RMVPE_UNET", True)      # what install(rmvpe_unet=True) sets
    monkeypatch.setenv("RVCMI_RMVPE_UNET", "0")      # ... and the environment overrides
    assert accelerate_f0_rmvpe(r) == 1 and not hasattr(r, "_rvcmi_unet")
    monkeypatch.delenv("RVCMI_RMVPE_UNET")
    assert accelerate_f0_rmvpe(r) == 1 and r._rvcmi_unet == 1 and isinstance(r.model.unet, rvc_amd.UNetHIP) and isinstance(r.model.gru, rvc_amd.GRUHIP)
    assert accelerate_f0_rmvpe(r) == 1 and r._rvcmi_unet == 1
    monkeypatch.setattr(ru, "RMVPE_UNET", False)
    monkeypatch.setenv("RVCMI_RMVPE_UNET", "1")
    r2 = _rmvpe_standin(gpu)
    accelerate_f0_rmvpe(r2)
    assert r2._rvcmi_unet == 1


def test_realtime_f0_graph_with_the_swap_on(gpu, monkeypatch):
    """``realtime._rmvpe_f0_graphed`` with ``RVCMI_RMVPE_UNET=1``: captured after ``RT_GRAPH_AFTER`` blocks; every replay equals the eager
    chain BIT FOR BIT (no MIOpen convolution is left in the chain), follows its input, and still does after a call of the whole chain
    at a larger T (the U-Net's workspace comes from the caller per call, and the GRU handle keeps the workspace a captured graph points at)."""
    import rvc_amd
    import rvc_amd.pipeline as rp
    from rvc_amd import realtime as rt

    monkeypatch.delenv("RVCMI_RMVPE_GRU", raising=False)
    monkeypatch.delenv("RVCMI_RT_GRAPH", raising=False)
    monkeypatch.setenv("RVCMI_RMVPE_UNET", "1")
    n = rt.f0_extractor_frame(4096, "rmvpe", 160)
    p_len = n // 160
    me = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=_rmvpe_standin(gpu), is_half=True, device=gpu))
    g = torch.Generator().manual_seed(1)
    outs = []
    for i in range(8):
        wav = (0.2 * (i + 1) * torch.randn(n, generator=g)).to(gpu)
        if i == 5:  # a longer input through the SAME chain (U-Net handle and GRU handle) between two replays
            big = (0.2 * torch.randn(16000 * 3, generator=g)).to(gpu)
            assert rp._rmvpe_on_device(me, big, big.shape[0] // 160, 0)[1].shape[-1] == big.shape[0] // 160
        pitch, pitchf = rt._rmvpe_f0_graphed(me, wav, p_len, 0)
        pitch, pitchf = pitch.clone(), pitchf.clone()
        entry = me._rvcmi_f0_graphs[(n, p_len, 0, str(wav.device))]
        assert ("graph" in entry) == (i >= rt.RT_GRAPH_AFTER - 1), (i, list(entry))
        want = rp._rmvpe_on_device(me, wav, p_len, 0)
        assert torch.equal(pitch, want[0]) and torch.equal(pitchf, want[1]), "block %d: the replay differs from the eager chain" % i
        outs.append(me.f0_gen.rmvpe._mel2hidden(me.f0_gen.rmvpe.mel_extractor(wav.unsqueeze(0), center=True)).clone())
    r = me.f0_gen.rmvpe
    assert r._rvcmi_unet == 1 and isinstance(r.model.unet, rvc_amd.UNetHIP) and isinstance(r.model.gru, rvc_amd.GRUHIP)
    assert not torch.equal(outs[-1], outs[-2]), "two different inputs gave the same salience: the network does not follow its input"


def test_errors(gpu):
    import rvc_amd

    hip = rvc_amd.UNetHIP.from_state_dict(uc.seeded_weights(uc.key_list(3, 1, 1, 16), 0), gpu)
    assert hip(torch.zeros(1, 1, 8, 128, device=gpu)).shape == (1, 3, 8, 128)
    with pytest.raises(rvc_amd.RvcmiError):
        hip(torch.zeros(1, 1, 8, 128))                 # CPU input: no fallback
    with pytest.raises(rvc_amd.RvcmiError):
        hip(torch.zeros(1, 1, 8, 100, device=gpu))     # mel width
    with pytest.raises(rvc_amd.RvcmiError):
        hip(torch.zeros(1, 1, 12, 128, device=gpu))    # T not a multiple of 2^levels
    with pytest.raises(rvc_amd.RvcmiError):
        hip(torch.zeros(1, 1, 1 << 23, 1, device=gpu).expand(1, 1, 1 << 23, 128))  # beyond what the handle serves: rejected, nothing launched
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.UNetHIP.from_state_dict(uc.seeded_weights(uc.key_list(2, 1, 1, 24), 0), gpu)   # channels not a multiple of 16
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.UNetHIP.from_state_dict(uc.seeded_weights(uc.key_list(2, 1, 1, 16), 0), "cpu")
    if torch.cuda.device_count() > 1:
        with pytest.raises(rvc_amd.RvcmiError):
            hip(torch.zeros(1, 1, 8, 128, device="cuda:1"))
    else:  # one GPU here: the check itself, against a handle that claims another device
        other = rvc_amd.UNetHIP.from_state_dict(uc.seeded_weights(uc.key_list(3, 1, 1, 16), 0), gpu)
        other._device = torch.device("cuda", 1)
        with pytest.raises(rvc_amd.RvcmiError):
            other(torch.zeros(1, 1, 8, 128, device=gpu))
