"""Shared pieces of the HuBERT feature-extractor tests (tests/test_cpu_hubert.py, tests/test_gpu_hubert.py) and of tools/hubert_fe_parity.py /
tools/make_golden_hubert.py: the seeded cases, an fp64 restatement of the seven layers with the kernel's fp16 rounding points, and the bars
csrc/hubert_fe.hip is held to against it.

The oracle (``extractor``) rounds to fp16 where the kernel does -- the weights, the input when it arrives as fp16, every layer's output --
and nowhere else; with the rounding off it is transformers' ``HubertFeatureEncoder`` in fp64 to ~1e-12 (tests/test_cpu_hubert.py, and the
committed goldens tests/golden/hubert_fe_*.npz written by tools/make_golden_hubert.py from that module).  Weights come from numpy's
``default_rng(seed)`` at torch's default scales (conv: uniform within 1 / sqrt(fan_in)), so every machine rebuilds them.

The bars are derived, not measured on the kernel.  ``floor`` = the oracle evaluated in float32 against its float64 evaluation: fp32 rounding
that now and then flips the fp16 rounding of a stored activation; a flip is one fp16 ulp, and the layers behind it carry it on.  The kernel
differs from that fp32 evaluation in three ways, each of which the oracle can imitate (``perturb=``): erff (perturbed by +-4 ulp at random,
above the 2 ulp CUDA documents for erff and the bound of the device library's polynomial), the normalisation's 1 / sqrt (its scale is
rounded to float once: +-1 ulp), and the summation order of the K loop (the products summed in 64-wide chunks in a permuted order).  With
all three at once, over every case of ``TABLE`` and two seeds, the error against the fp64 oracle moved to at most 1.13x the floor's RMS and
1.12x the floor's max-abs; twice that, rounded up to the next half, is the factor 2.5.  On the all-zero input the floor is exactly 0 (every
frame is the same number and fp32 agrees with fp64 on its rounding), and the perturbed evaluation sits 0.59 ulp16(rms y) RMS and
0.5 ulp16(max |y|) max-abs away (ulp16(v) = the spacing of fp16 at v); twice that is the additive term:

    bar_rms = 2.5 * floor_rms + 1.2 * ulp16(rms y)        bar_max = 2.5 * floor_max + ulp16(max |y|)

Layer 0 alone is held to account too (``bars0``): a wrong GELU or a wrong variance is a fraction of an fp16 ulp per element there, plain to
see against a floor of rare flips, while six more layers of fp16 rounding bury it in the final output.  The factor is the same 2.5 (the
perturbed evaluations moved to at most 1.1x the floor there).  The additive term above is NOT: it measures flips that have cascaded through
six layers, and at layer 0 nothing has cascaded -- the perturbations leave the all-zero input's layer 0 bit-equal.  There it is ONE flip of
one element more than the floor saw: ``bar_rms = 2.5 * floor_rms + ulp16(max |y|) / sqrt(n)``, ``bar_max = 2.5 * floor_max + ulp16(max |y|)``.
``test_cpu_hubert.py::test_perturbations_stay_inside_half_the_bars`` prints the ratios and asserts that the perturbed evaluations stay within
HALF of each bar.
tests/test_cpu_hubert.py asserts that the named wrong variants of the oracle stand clear of these bars, so widening them fails there.
"""
import collections
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHANNELS = 512
KERNELS = (10, 3, 3, 3, 3, 2, 2)
STRIDES = (5, 2, 2, 2, 2, 2, 2)
EPS = 1e-5
M_TILE = 128  # frames per block of k_hfe_gemm (csrc/hubert_fe_kernels.hpp GM)
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# kind: "noise" (white, amplitude 0.5), "zero", "small" (white, amplitude 1e-3), "dc" (0.5 + white 1e-3: the cancellation case)
Case = collections.namedtuple("Case", "B N seed half wgain kind", defaults=(0, True, 1.0, "noise"))

ITEM_GAINS = (1.0, 0.125, 3.0)  # item b of a batch is scaled by ITEM_GAINS[b]: statistics shared across the batch would show


def n_for_frames(L6):
    return 400 + 320 * (L6 - 1)


def n_for_layer1_rows(L1):
    return 5 * (2 * L1 + 1 - 1) + 10


# N = 400 / 719: one frame, 720 / 1040: 2 / 3 frames; the M tile of the GEMM kernel one under, at and one over at the last layer and (through N)
# at layer 1; batches with items of different gain; both input dtypes; weights x 2.5; the zero, small and DC inputs
SHAPES = tuple(Case(1, N, 10 + i) for i, N in enumerate((400, 719, 720, 1040, 16000)))
TILE_EDGES = tuple(Case(1, n_for_frames(L), 20 + i) for i, L in enumerate((M_TILE - 1, M_TILE, M_TILE + 1))) + tuple(
    Case(1, n_for_layer1_rows(L), 30 + i) for i, L in enumerate((M_TILE - 1, M_TILE, M_TILE + 1)))
BATCHES = (Case(2, 1040, 40), Case(3, 5040, 41), Case(2, 5040, 42, False))
SPECIAL = (Case(1, 5040, 50, False), Case(1, 5040, 51, True, 2.5), Case(1, 5040, 52, True, 1.0, "zero"), Case(2, 5040, 53, False, 1.0, "small"),
           Case(1, 5040, 54, True, 1.0, "small"), Case(2, 16000, 55, False, 1.0, "dc"), Case(1, 5040, 56, True, 1.0, "dc"))
TABLE = SHAPES + TILE_EDGES + BATCHES + SPECIAL
# the cases whose layer 0 is also compared on its own (bars0); the all-zero input's layer 0 has a test to itself (it is GELU(beta))
LAYER0 = tuple(c for c in TABLE if c.B == 1 and c.N in (1040, 5040, 16000) and c.kind != "zero")
GOLDEN = {"hubert_fe_n8000": Case(1, 8000, 60, False), "hubert_fe_b2_n1040": Case(2, 1040, 61, False)}


def case_id(c):
    return "B%d-N%d-seed%d-%s%s%s" % (c.B, c.N, c.seed, "f16" if c.half else "f32", "" if c.wgain == 1.0 else "-w%g" % c.wgain,
                                      "" if c.kind == "noise" else "-" + c.kind)


def frames(N):
    return (N - 400) // 320 + 1 if N >= 400 else 0


@functools.lru_cache(maxsize=None)
def weights(seed, wgain=1.0):
    """-> {"conv": 7 float32 arrays in torch's [Cout, Cin, k] layout, "gamma", "beta"}: torch's default conv scale (times ``wgain``), an
    affine GroupNorm away from its (1, 0) default"""
    rng = np.random.default_rng(seed)
    conv = []
    for i, k in enumerate(KERNELS):
        cin = CHANNELS if i else 1
        b = 1.0 / np.sqrt(cin * k)
        conv.append((wgain * rng.uniform(-b, b, (CHANNELS, cin, k))).astype(np.float32))
    w = {"conv": tuple(conv), "gamma": (1.0 + 0.25 * rng.standard_normal(CHANNELS)).astype(np.float32),
         "beta": (0.25 * rng.standard_normal(CHANNELS)).astype(np.float32)}
    for a in conv + [w["gamma"], w["beta"]]:
        a.setflags(write=False)
    return w


def state_dict(w, layout="hf"):
    """The weights under transformers' (``hf``) or fairseq's key layout, as torch tensors."""
    sd = {}
    for i, a in enumerate(w["conv"]):
        sd[("conv_layers.%d.conv.weight" if layout == "hf" else "conv_layers.%d.0.weight") % i] = torch.from_numpy(a.copy())
    for name, a in (("weight", w["gamma"]), ("bias", w["beta"])):
        sd[("conv_layers.0.layer_norm." if layout == "hf" else "conv_layers.0.2.") + name] = torch.from_numpy(a.copy())
    return sd


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> x [B, N] float32 (already on the fp16 grid when ``c.half``, so the fp16 tensor the kernel receives holds the same numbers)"""
    rng = np.random.default_rng(1000 + c.seed)
    noise = rng.uniform(-1.0, 1.0, (c.B, c.N))
    x = {"noise": 0.5 * noise, "zero": 0.0 * noise, "small": 1e-3 * noise, "dc": 0.5 + 1e-3 * noise}[c.kind]
    x = x * np.asarray(ITEM_GAINS[:c.B])[:, None]
    x = x.astype(np.float32)
    if c.half:
        x = x.astype(np.float16).astype(np.float32)
    x.setflags(write=False)
    return x


def r16(a):
    return a.astype(np.float16).astype(a.dtype)


def _erf(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def _ulps(rng, shape, n, dtype):
    """1 + a random whole number of float32 ulps in [-n, n]"""
    return (1.0 + rng.integers(-n, n + 1, shape) * 2.0 ** -23).astype(dtype)


def _matmul(a, w, perturb, rng):
    """a [.., K] @ w [K, C]; with the summation-order perturbation: 64-wide chunks summed one after the other in a permuted order"""
    if not (perturb and perturb.get("reorder")):
        return a @ w
    K = a.shape[-1]
    acc = np.zeros(a.shape[:-1] + (w.shape[1],), dtype=a.dtype)
    for k0 in rng.permutation(np.arange(0, K, 64)):
        acc = acc + a[..., k0:k0 + 64] @ w[k0:k0 + 64]
    return acc


def gelu(v, variant=None, perturb=None, rng=None):
    if variant == "tanh_gelu":
        return 0.5 * v * (1.0 + np.tanh(np.sqrt(2.0 / np.pi).astype(v.dtype) * (v + v.dtype.type(0.044715) * v * v * v)))
    e = _erf(v * v.dtype.type(0.7071067811865476))
    if perturb and perturb.get("erf"):
        e = e * _ulps(rng, e.shape, perturb["erf"], v.dtype)
    return v.dtype.type(0.5) * v * (v.dtype.type(1.0) + e)


def extractor(w, x, half_input=True, arith="f64", variant=None, round_operands=True, perturb=None, layers=7):
    """The seven layers.  ``x`` [B, N]; -> [B, 512, L6] in ``arith``'s dtype (``layers=1``: layer 0 alone, channels-last [B, L0, 512]).  ``round_operands=False``: no fp16 rounding anywhere (the
    function transformers' module computes).  ``variant``: a named WRONG network (tests/test_cpu_hubert.py).  ``perturb``: {"erf": ulps,
    "rsqrt": ulps, "reorder": bool, "seed": int}, the kernel's documented liberties (module docstring)."""
    dt = np.float64 if arith == "f64" else np.float32
    rng = np.random.default_rng((perturb or {}).get("seed", 0))
    rnd = r16 if round_operands else (lambda a: a)
    x = np.asarray(x, dtype=dt)
    if half_input:
        x = rnd(x)
    B, N = x.shape
    # layer 0: one input channel, 10 taps, stride 5; GroupNorm over the time axis per (item, channel); GELU
    n_extra = {"frame_more": 1, "frame_less": -1}.get(variant, 0)
    L = (N - KERNELS[0]) // STRIDES[0] + 1
    w0 = rnd(w["conv"][0][:, 0, :].astype(dt))
    if variant == "taps_reversed":
        w0 = w0[:, ::-1]
    fr = np.lib.stride_tricks.sliding_window_view(x, KERNELS[0], axis=1)[:, ::STRIDES[0]][:, :L]
    y = _matmul(np.ascontiguousarray(fr), np.ascontiguousarray(w0.T), None, rng)  # [B, L, 512]
    src = r16(y) if variant == "stats_from_fp16" else y
    if variant == "stats_across_batch":
        mean, var = src.mean(axis=(0, 1), keepdims=True), src.var(axis=(0, 1), keepdims=True)
    else:
        mean, var = src.mean(axis=1, keepdims=True), src.var(axis=1, keepdims=True, ddof=1 if variant == "unbiased_var" and L > 1 else 0)
    rstd = 1.0 / np.sqrt(var + (0.0 if variant == "no_eps" else dt(EPS)))
    if perturb and perturb.get("rsqrt"):
        rstd = rstd * _ulps(rng, rstd.shape, perturb["rsqrt"], dt)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = (y - mean) * rstd.astype(dt) * w["gamma"].astype(dt) + w["beta"].astype(dt)
    h = rnd(gelu(y.astype(dt), variant, perturb, rng))
    if layers == 1:
        return h
    # layers 1 - 6: channels-last, row t of the operand = the k * 512 values that start at input row 2 t
    for i in range(1, len(KERNELS)):
        k = KERNELS[i]
        wi = rnd(w["conv"][i].astype(dt))
        if variant == "taps_reversed":
            wi = wi[:, :, ::-1]
        L = (h.shape[1] - k) // STRIDES[i] + 1
        if i == len(KERNELS) - 1:
            L += n_extra
        a = np.stack([h[:, 2 * t:2 * t + k].reshape(B, -1) if 2 * t + k <= h.shape[1] else np.zeros((B, k * CHANNELS), dt) for t in range(L)],
                     axis=1) if L > 0 else np.zeros((B, 0, k * CHANNELS), dt)
        y = _matmul(a, np.ascontiguousarray(wi.transpose(2, 1, 0).reshape(k * CHANNELS, CHANNELS)), perturb, rng)
        h = rnd(gelu(y.astype(dt), variant, perturb, rng))
    return np.ascontiguousarray(h.transpose(0, 2, 1))


def ulp16(v):
    """the spacing of fp16 at |v| (normal range)"""
    v = max(abs(float(v)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(v)) - 10)


def err(got, want):
    """-> (RMS, max-abs) of got - want, in float64"""
    e = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    return (float(np.sqrt(np.mean(e * e))), float(np.abs(e).max())) if e.size else (0.0, 0.0)


def bars_of(y32, y64, layer0=False):
    floor_rms, floor_max = err(y32, y64)
    y = np.asarray(y64, dtype=np.float64)
    one = ulp16(np.abs(y).max())
    add_rms = one / np.sqrt(y.size) if layer0 else 1.2 * ulp16(np.sqrt(np.mean(y * y)))
    return {"floor_rms": floor_rms, "floor_max": floor_max, "bar_rms": 2.5 * floor_rms + add_rms, "bar_max": 2.5 * floor_max + one}


@functools.lru_cache(maxsize=None)
def bars(c):
    """The oracle of a case (``y`` [B, 512, L6] float64; computed once, never changed) and the bars against it."""
    w, x = weights(c.seed, c.wgain), inputs(c)
    y64 = extractor(w, x, c.half)
    y32 = extractor(w, x, c.half, arith="f32")
    y64.setflags(write=False)
    return {"y": y64, **bars_of(y32, y64)}


def layer0_kept_rows(N):
    """Rows [first, L0) of layer 0's output are still in the caller's workspace after a forward of ONE item: the buffer is reused by layers 2
    and 4, which overwrite its first L2 rows (include/rvcmi.h, rvcmi_hubert_fe_forward)."""
    L0 = (N - KERNELS[0]) // STRIDES[0] + 1
    L1 = (L0 - 3) // 2 + 1
    return (L1 - 3) // 2 + 1, L0


@functools.lru_cache(maxsize=None)
def bars0(c):
    """As ``bars`` for layer 0 alone, on the rows ``layer0_kept_rows`` names (``y`` [rows, 512]; B = 1): where a wrong GroupNorm or GELU shows
    before six more layers of fp16 rounding bury it."""
    assert c.B == 1
    w, x = weights(c.seed, c.wgain), inputs(c)
    first, _ = layer0_kept_rows(c.N)
    y64 = extractor(w, x, c.half, layers=1)[0, first:]
    y32 = extractor(w, x, c.half, arith="f32", layers=1)[0, first:]
    y64.setflags(write=False)
    return {"y": y64, **bars_of(y32, y64, layer0=True)}


def hf_module(w, dtype=torch.float64):
    """transformers' own feature encoder holding ``w`` (the independent definition of the network)"""
    from transformers import HubertConfig
    from transformers.models.hubert.modeling_hubert import HubertFeatureEncoder

    fe = HubertFeatureEncoder(HubertConfig()).eval()
    fe.load_state_dict(state_dict(w, "hf"))
    return fe.to(dtype)
