"""Shared pieces of the generator's per-layer tests (tests/test_cpu_nsf_layers.py, tests/test_gpu_nsf_layers.py) and of tools/nsf_parity.py: the
seeded cases, which ResBlock path and which stream dtypes each of them runs on, the per-layer fp64 oracle (oracle/nsf_layer_oracle.py, which rounds
where csrc/nsf.hip and its kernel headers round) and the bars the kernels are held to against it.

Layer by layer: the oracle of layer n is applied to the tap the DEVICE produced for layer n - 1, so only layer n's arithmetic is compared, and the
floor stays shallow (an end-to-end rounded oracle is as far from its own fp32 evaluation as the fp16 design is from the reference: flips of fp16
roundings cascade through 72 convolutions; DESIGN.md "Generator parity").

The bars are derived, not measured on the kernel.  ``floor`` = the layer's oracle evaluated in float32 against its float64 evaluation on the same
input: fp32 summation noise, and -- wherever an operand or a stream is rounded inside the layer -- the rare fp16 roundings it flips.  The kernels
differ from that fp32 evaluation in the summation order of the K loop (MFMA k-steps of 16 channels, taps split over waves) and in tanhf.  The
oracle imitates each (``perturb=``: the K loop summed k-step by k-step in a permuted order, tanh moved by +-4 ulp at random, the one contractible
multiply-add of the MFMA layers fused; conv_post's fp32 evaluation already is the kernels' one-rounding fmaf chain); over ``CPU_TABLE`` and two perturbation seeds the perturbed fp32 evaluations moved
to at most ``PERTURB_WORST`` x the floor (tests/test_cpu_nsf_layers.py prints every ratio and asserts that they stay within HALF of each bar);
``FACTOR`` is derived from that where it is defined below -- one for the MFMA layers, one for conv_post, whose liberties differ.  The additive
term covers a floor of (nearly) zero -- a short layer in which the fp32 evaluation happened to flip nothing: ONE flip of one stored element more
than the floor saw, i.e. one fp16 ulp at max |y| for max-abs and that ulp over sqrt(n) for RMS where the layer's output is stored as fp16 (X0
under ``x0_half``, the Y streams under ``y_half``), and the same with an fp32 ulp where it is stored as fp32:

    bar_rms = FACTOR * floor_rms + ulp(max |y|) / sqrt(n)            bar_max = FACTOR * floor_max + ulp(max |y|)

tests/test_cpu_nsf_layers.py asserts that the named wrong variants of the oracle stand clear of these bars, so widening them fails there.

Sizes, from the constants of the headers (rows = B x L, L = T x the product of the upsample rates so far):
  CONV_TILE_SMALL = 32     rows per block of conv_pre and of the SPLIT path at C = 256 for short launches (nsf.hip run_conv nj = 1, conv_ks_nj(256))
  SPLIT_ROWS_128 = 96      rows per block of the SPLIT path at C = 128 (nsf.hip conv_ks_nj(128) x 32)
  UPS_TQ0 = 64             input rows per block of k_ups at C_in = 512 (nsf.hip ups_mfma: nj = 2, four channel waves); 32 at C_in = 256, 64 at 128
  RB_ROWS = 128            k_rb_pair's tile: 128 - (k - 1) valid rows per tile (rb_pair_kernels.hpp RB_ROWS, nsf.hip rb_rows)
  RB_SPLIT_MAX_ROWS = 1024 / RB_SPLIT_MAX_ROWS_128 = 4096: the SPLIT path ends above these rows (nsf.hip plan_stage)
  RBF_SMALL_ROWS = 256     k_rb_full's small tile, 256 - 2 * halo valid rows (halo 60 / 36 / 12 for k = 11 / 7 / 3: 136 / 184 / 232)
  rbf_rows(64) = 512, rbf_rows(32) = rbf_rows(16) = 384: its default tiles, taken from num_cus() / 2 (C = 64) or num_cus() (C = 32) blocks (plan_stage)
  RBF_TALL_ROWS = 768      its tall tile at C = 32, taken from 4 x num_cus() blocks of 768 rows on (option RBF32_TALL: 1 always, 0 never)
  RS_HEAD = 62, R = 32 * NJ = 192 (RS_SMALL = 1) / 256 (RS_SMALL = 0) rows per step of k_rb_stream; the strip planner (rb_stream.hip launch_geo) cuts
                           an utterance into at most L / R strips per resblock: a forced launch at T = 24 (2880 rows) is up to 15 strips of two steps each
                           (one step of rows, one of warm-up), T = 1, 2, 3 are single strips of 120, 240, 360 rows against the 192-row step
Every L is T times a product of upsample rates, so the row counts BRACKET the edges of k_rb_pair's, k_rb_full's and k_rb_stream's tiles (one or two
tiles per kernel size, a sequence that ends inside the first tile, inside the second, behind it); they cannot sit exactly one under, at and one over
118 / 122 / 126, 136 / 184 / 232 or 192 rows, because no shipped config has an L of those sizes.  The tiles that ARE hit exactly: conv_pre's and SPLIT's
32 rows (T = 31, 32, 33), k_ups' 64 input rows (T = 63, 64, 65), the SPLIT thresholds, and k_rb_full's block-count threshold (T = 76 / 77, 54 / 55).

Which kernel ran is REPORTED by the forward whose output is compared: the path, k_rb_full's tile class, the tile / strip counts and the stream dtypes
of every stage come from ``gen.last_plan()`` (include/rvcmi.h rvcmi_nsf_last_plan), and the profiler's kernel names must agree with the reported path.
The rules below (``expected_paths``, ``stream_plan``, ``full_tile_counts``) restate the planner independently and are held against the report in every case.
"""
import collections
import functools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import nsf_layer_oracle as lo  # noqa: E402
from oracle import nsf_oracle, synth  # noqa: E402
from oracle.nsf_oracle import GenConfig  # noqa: E402

CONFIGS = dict(nsf_oracle.CONFIGS)
CONFIGS["nof0_v2_48k"] = GenConfig(**{**vars(nsf_oracle.CONFIGS["v2_48k"]), "use_f0": False})

MI355X_CUS = 256  # what the CPU tests plan with; the GPU test asks the device
RB_SPLIT_MAX_ROWS, RB_SPLIT_MAX_ROWS_128 = 1024, 4096
RBF_SMALL_ROWS, RBF_TALL_ROWS = 256, 768
CONV_TILE_SMALL, UPS_TQ0, RB_ROWS = 32, 64, 128

# 2 x the largest perturbed / floor ratio (RMS or max-abs) seen over CPU_TABLE x 2 perturbation seeds, rounded up to the next half.  Per kind of layer,
# because the liberties differ: the MFMA layers (pre, up<i>, stage<i>) reorder their K loop (and may contract the one multiply-add of their fp32 epilogues,
# see below); conv_post's fp32 evaluation is the kernels' own fmaf chain on a floor of a few fp32 ulps, and tanhf moves it.  Layers whose bar is decided by
# the additive term (FACTOR * floor < the one-flip term: a handful of flips or none) do not count.
# FMA contraction: the MFMA layers' fp32 epilogues are additions of already rounded terms (acc + bias + cond, conv_kernels.hpp: conv_mfma_body, epilogue; + NZ / + bn, ups_kernels.hpp: k_ups, epilogue;
# conv2 + b2 + x), lrelu's product feeds a median, not an add, and div3_exact is the IEEE quotient whatever is fused (exact_fp.hpp).  The ONE product that an add
# follows is the VALU noise conv of the last stage, bias + w * har (ups_kernels.hpp: k_ups, VALU noise loop of the epilogue): ``perturb["fma"]`` rounds it once instead of twice.
PERTURB_WORST = {"mfma": 1.99, "post": 2.29}  # pre of the bf16 case (max-abs): 3.98 -> 4.0; post of v1_32k and v1_48k (RMS): 4.58 -> 5.0
FACTOR = {"mfma": 4.0, "post": 5.0}


def kind_of(name):
    return "post" if name == "post" else "mfma"


# opts: the handle options that pin the path, as a sorted tuple of (key, value).  kind: "synth" (oracle/synth.py's draws), "voiced" (f0 > 0
# everywhere), "unvoiced" (f0 = 0), "zero" (z = 0 and f0 = 0).  wgain: conv_pre and ups weights and biases x wgain (larger activations at every
# stage, coarser fp16 ulp).  layers: None = every layer, else the layers compared (long cases: only the stage under test gets an oracle).
# want: ((stage, path), ...) the path the case is there for, asserted on the device ("FULL256" / "FULL384" / "FULL512" / "FULL768" name k_rb_full's tile class by its rows).
Case = collections.namedtuple("Case", "cfg B T seed opts operand wgain kind layers want", defaults=(0, (), "fp16", 1.0, "synth", None, ()))


def O(**kw):
    return tuple(sorted(kw.items()))


PAIR = O(RB_STREAM=0, NO_RB_SPLIT=1)
STREAM = O(RB_STREAM=1)

# conv_pre's / SPLIT's 32-row tile one under, at, one over (T = 31, 32, 33); T = 1, 2: the sequence ends inside the first tile and inside the convs' halo
DEFAULT = tuple(Case("v2_48k", 1, T, 10 + i, want=((0, "SPLIT"), (1, "SPLIT"), (2, "FULL256"), (3, "FULL256")))
                for i, T in enumerate((1, 2, 24, CONV_TILE_SMALL - 1, CONV_TILE_SMALL, CONV_TILE_SMALL + 1)))
# the SPLIT path's last and first-not sizes: C = 128 rows 4080 / 4200 (T = 34 / 35), C = 256 rows 1020 / 1032 (T = 85 / 86, where k_rb_pair takes over)
SPLIT_EDGE = (Case("v2_48k", 1, RB_SPLIT_MAX_ROWS_128 // 120, 20, layers=("up1", "stage1"), want=((1, "SPLIT"),)),
              Case("v2_48k", 1, RB_SPLIT_MAX_ROWS_128 // 120 + 1, 21, layers=("up1", "stage1")),
              Case("v2_48k", 1, RB_SPLIT_MAX_ROWS // 12, 22, layers=("up0", "stage0"), want=((0, "SPLIT"),)),
              Case("v2_48k", 1, RB_SPLIT_MAX_ROWS // 12 + 1, 23, layers=("up0", "stage0"), want=((0, "PAIR"),)))
# k_ups' 64-row input tile at C_in = 512 one under, at, one over
UPS_EDGE = tuple(Case("v2_48k", 1, T, 25 + i, layers=("pre", "up0")) for i, T in enumerate((UPS_TQ0 - 1, UPS_TQ0, UPS_TQ0 + 1)))
# the other configs: five stages down to C = 16 and u = 4 (v1_32k; T = 1, 2, 3 are 80, 160, 240 rows at C = 64 against the small tile's 136 / 184 / 232
# valid rows), u = 10 / 10 (v1_40k), the polyphase patterns u = 8 (v2_32k) and u = 6 (v1_48k), no f0
CONFIG_CASES = tuple(Case("v1_32k", 1, T, 30 + i) for i, T in enumerate((1, 2, 3, 16))) + (
    Case("v1_40k", 1, 20, 35), Case("v2_32k", 1, 16, 36), Case("v1_48k", 1, 12, 37), Case("nof0_v2_48k", 1, 16, 38))
# k_rb_pair (128 - (k - 1) = 126 / 122 / 118 valid rows per tile): stage 0 of v1_40k has 110 / 120 / 130 rows at T = 11 / 12 / 13 -- one tile for every k,
# two tiles for k = 11 alone, two for every k -- and v2_48k 120 (stage 0) and 1200 (stage 1, C = 128) at T = 10
PAIR_CASES = tuple(Case("v1_40k", 1, T, 40 + i, PAIR, want=((0, "PAIR"), (1, "PAIR"))) for i, T in enumerate((11, 12, 13))) + (
    Case("v2_48k", 1, 10, 43, PAIR, want=((0, "PAIR"), (1, "PAIR"))),)
# k_rb_stream at C = 128, forced: both tile heights x both K loops, T = 1, 2, 3 (120, 240, 360 rows against steps of 192), fp32 X0 and fp32 Y streams
STREAM_CASES = tuple(Case("v2_48k", 1, 24, 50 + 2 * s + k, O(RB_STREAM=1, RS_SMALL=s, RS_KL=k), want=((1, "STREAM"),))
                     for s in (0, 1) for k in (1, 2)) + tuple(
    Case("v2_48k", 1, T, 55 + T, STREAM, layers=("up1", "stage1", "up2"), want=((1, "STREAM"),)) for T in (1, 2, 3)) + (
    Case("v2_48k", 1, 24, 59, O(RB_STREAM=1, X0_F16_NOSTREAM=1), layers=("up1", "stage1", "up2"), want=((1, "STREAM"),)),
    Case("v2_48k", 1, 24, 60, O(RB_STREAM=1, Y_F16=0), want=((1, "STREAM"),)))
# k_rb_full's large tiles need num_cus() / 2 blocks at C = 64 and num_cus() at C = 32: on 256 CUs the first T with 128 blocks of 512 rows at stage 2
# (L = 240 T; valid rows 392 / 440 / 488) is 77, with 256 blocks of 384 rows at stage 3 (L = 480 T; 264 / 312 / 360) it is 55; one frame less is the small
# tile at its largest launch
FULL_CASES = (Case("v2_48k", 1, 76, 61, layers=("stage2",), want=((2, "FULL256"),)), Case("v2_48k", 1, 77, 62, layers=("stage2",), want=((2, "FULL512"),)),
              Case("v2_48k", 1, 54, 63, layers=("stage3",), want=((3, "FULL256"),)), Case("v2_48k", 1, 55, 64, layers=("stage3", "post"), want=((3, "FULL384"),)),
              Case("v2_48k", 1, 80, 65, layers=("up2", "stage2", "up3", "stage3", "post"), want=((2, "FULL512"), (3, "FULL384"))))
# stream options off the default, conv_post's two kernels at C = 32 and C = 16
OPTION_CASES = (Case("v2_48k", 1, 24, 70, O(Y_F16=0)), Case("v2_48k", 1, 24, 71, O(X0_F16=0)), Case("v2_48k", 1, 24, 72, O(POST_DMA=0)),
                Case("v2_48k", 1, 24, 73, O(POST_DMA=1)), Case("v1_32k", 1, 16, 74, O(POST_DMA=0)), Case("v1_32k", 1, 16, 75, O(POST_DMA=1)))
# bf16 operands, one case per path (the streams stay fp16: pack4_h)
BF16_CASES = (Case("v2_48k", 1, 24, 80, (), "bf16"), Case("v2_48k", 1, 10, 81, PAIR, "bf16", want=((0, "PAIR"), (1, "PAIR"))),
              Case("v2_48k", 1, 24, 82, STREAM, "bf16", want=((1, "STREAM"),)),
              Case("v2_48k", 1, 77, 83, (), "bf16", layers=("stage2",), want=((2, "FULL512"),)))
INPUT_CASES = (Case("v2_48k", 1, 24, 90, kind="voiced"), Case("v2_48k", 1, 24, 91, kind="unvoiced"), Case("v2_48k", 1, 24, 92, wgain=2.5),
               Case("v2_48k", 1, 24, 93, kind="zero"))
TABLE = DEFAULT + SPLIT_EDGE + UPS_EDGE + CONFIG_CASES + PAIR_CASES + STREAM_CASES + FULL_CASES + OPTION_CASES + BF16_CASES + INPUT_CASES
# a batch of two different items: each against its own oracle, and bit-equal to its single-item call with the path pinned
# (T = 16: 3840 rows at C = 128, so the batch and its single items all take the SPLIT path by themselves)
BATCH_CASES = (Case("v2_48k", 2, 16, 95), Case("v2_48k", 2, 24, 96, PAIR), Case("v2_48k", 2, 24, 97, STREAM), Case("v1_32k", 2, 3, 98))
# what the CPU tests walk (no GPU: a layer's input is the fp32 evaluation's own previous tap): every config, every dtype plan (fp32 streams on SPLIT and
# PAIR, fp16 X0 and Y on FULL and STREAM, Y_F16 = 0), both operand types, every kind of input, at the smallest T that still has more than one tile somewhere
CPU_TABLE = (DEFAULT[0], DEFAULT[1], DEFAULT[2], Case("v2_48k", 1, 8, 101, STREAM), Case("v2_48k", 1, 8, 102, O(Y_F16=0)), Case("v2_48k", 1, 8, 103, PAIR, "bf16"),
             Case("v1_32k", 1, 3, 104), Case("v1_40k", 1, 8, 105, PAIR), Case("v2_32k", 1, 8, 106), Case("v1_48k", 1, 6, 107), Case("nof0_v2_48k", 1, 8, 108),
             Case("v2_48k", 1, 8, 109, kind="voiced"), Case("v2_48k", 1, 8, 110, wgain=2.5), Case("v2_48k", 1, 8, 111, kind="zero"), Case("v2_48k", 2, 6, 112))


def case_id(c):
    return "%s-B%d-T%d-seed%d%s%s%s%s" % (c.cfg, c.B, c.T, c.seed, "".join("-%s=%s" % kv for kv in c.opts), "" if c.operand == "fp16" else "-" + c.operand,
                                          "" if c.wgain == 1.0 else "-w%g" % c.wgain, "" if c.kind == "synth" else "-" + c.kind)


@functools.lru_cache(maxsize=8)
def weights(cfg_name, seed, wgain=1.0):
    w = synth.make_dec_weights(CONFIGS[cfg_name], seed)
    if wgain != 1.0:
        for k in w:
            if k.startswith(("conv_pre.", "ups.")):
                w[k] = w[k] * wgain
    return w


@functools.lru_cache(maxsize=8)
def inputs(c):
    """-> {"z", "g", "f0", "noise"} (f0 / noise None without f0)"""
    cfg = CONFIGS[c.cfg]
    z, f0, g = synth.make_dec_inputs(cfg, c.B, c.T, c.seed)
    noise = nsf_oracle.reference_noise(c.B, c.T, cfg.upp, c.seed) if cfg.use_f0 else None
    if cfg.use_f0:
        if c.kind == "voiced":
            t = torch.arange(c.T, dtype=torch.float32)
            f0 = (180.0 * torch.pow(2.0, torch.sin(2 * math.pi * t / 50.0))).unsqueeze(0).repeat(c.B, 1).contiguous()
        elif c.kind in ("unvoiced", "zero"):
            f0 = torch.zeros_like(f0)
    if c.kind == "zero":
        z = torch.zeros_like(z)
    return {"z": z, "g": g, "f0": f0, "noise": noise}


def cpu_har(c):
    """The excitation as nsf_oracle computes it in fp32 (the CPU tests' stand-in for the device's "har" tap)"""
    cfg, x = CONFIGS[c.cfg], inputs(c)
    if not cfg.use_f0:
        return None
    with torch.no_grad():
        return nsf_oracle.har_source(weights(c.cfg, c.seed, c.wgain), x["f0"], cfg.upp, cfg.sr, x["noise"])


# ---- plan_stage restated (nsf.hip plan_stage): which ResBlock path a stage takes and what its streams are stored as ------------------------------

def _rbf_halo(k, dils):
    return (k - 1) // 2 * (sum(dils) + len(dils))


def rbf_rows(C):
    return 512 if C == 64 else 384


def stage_rows(cfg, T):
    L, out = T, []
    for u in cfg.upsample_rates:
        L *= u
        out.append(L)
    return out


def expected_paths(cfg, B, T, opts, ncu=MI355X_CUS):
    """-> per stage "SPLIT" / "STREAM" / "FULL<tile rows>" / "PAIR", or None where the streaming planner decides (RB_STREAM unset, C = 128
    beyond the SPLIT rows: it takes the stage from 4 steps per block, else the stage runs pair by pair)"""
    o = dict(opts)
    mode = {None: 2, 0: 0, 1: 1}.get(o.get("RB_STREAM"), 2)
    nk = cfg.num_kernels
    out = []
    for i, L in enumerate(stage_rows(cfg, T)):
        C = cfg.upsample_initial_channel >> (i + 1)
        rows = B * L
        if ((C == 256 and rows <= RB_SPLIT_MAX_ROWS) or (C == 128 and rows <= RB_SPLIT_MAX_ROWS_128)) and nk <= 3 and not o.get("NO_RB_SPLIT") and mode != 1:
            out.append("SPLIT")
        elif mode != 0 and C == 128 and nk == 3 and all(len(d) == 3 for d in cfg.resblock_dilation_sizes):
            out.append("STREAM" if mode == 1 else None)
        elif C <= 64:
            R = rbf_rows(C)
            if C in (64, 32):
                blocks, blocks_tall, fits_tall = 0, 0, True
                for k, d in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes):
                    HL = _rbf_halo(k, d)
                    v = rbf_rows(C) - 2 * HL
                    blocks += (L + v - 1) // v * B
                    if RBF_SMALL_ROWS - 2 * HL < RBF_SMALL_ROWS // 4:
                        blocks = 1 << 30
                    blocks_tall += -(-L // (RBF_TALL_ROWS - 2 * HL)) * B
                    fits_tall = fits_tall and RBF_TALL_ROWS - 2 * HL >= RBF_TALL_ROWS // 4
                small = blocks < ncu // 2 * (1 if C == 64 else 2)
                tall = {None: 2, 0: 0, 1: 1}.get(o.get("RBF32_TALL"), 2) if C == 32 and fits_tall else 0
                if tall == 1 or (tall == 2 and not small and blocks_tall >= 4 * ncu):
                    R = RBF_TALL_ROWS
                elif small:
                    R = RBF_SMALL_ROWS
            out.append("FULL%d" % R)
        else:
            out.append("PAIR")
    return out


def stream_plan(paths, opts):
    """-> (x0_half, y_half) per stage for the paths a forward took (StagePlan.x0_half / stage_half)"""
    o = dict(opts)
    yh = o.get("Y_F16", 1) != 0
    x0h = yh and o.get("X0_F16", 1) != 0
    x0, y = [], []
    for p in paths:
        if p == "STREAM":
            # fp16 input rows only in the lean-K-loop kernel with the coalesced step IO (rb_stream.hip rb_stream_plan: RS_KL = 2 and the 192-row steps)
            x0.append(x0h and not o.get("X0_F16_NOSTREAM") and o.get("RS_KL", 2) == 2 and o.get("RS_SMALL", 1) != 0)
            y.append(yh)
        elif p.startswith("FULL"):
            x0.append(x0h)
            y.append(yh)
        else:
            x0.append(False)
            y.append(False)
    return tuple(x0), tuple(y)


def full_tile_counts(cfg, L, R):
    """{k: tiles} k_rb_full launches per resblock at tile height R: ceil(L / (R - 2 halo)) (nsf.hip rb_full J.ntiles)"""
    return {k: -(-L // (R - 2 * _rbf_halo(k, d))) for k, d in zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)}


def pair_tile_counts(cfg, L):
    """{k: tiles} k_rb_pair launches per resblock and pair level: ceil(L / (RB_ROWS - (k - 1))) (nsf.hip rb_pair J.ntiles)"""
    return {k: -(-L // (RB_ROWS - (k - 1))) for k in cfg.resblock_kernel_sizes}


KERNELS_OF = {"F32_CHAIN": ("rb_c%d",), "SPLIT": ("rb_split_c%d",), "STREAM": ("rb_stream_c%d",), "FULL": ("rb_full_c%d",),
              "PAIR": ("rb_pair_c%d", "rb_stream1_c%d")}  # (rb_stream1: a pair level on the streaming kernel)


def paths_from_plan(cfg, plan, names):
    """-> the path each stage took as the forward reported it (``gen.last_plan()``), k_rb_full's as "FULL<tile rows>", after asserting that the kernel
    names the profiler recorded for the same forward are those of the reported paths"""
    assert len(plan) == len(cfg.upsample_rates), plan
    out = []
    for i, r in enumerate(plan):
        C = cfg.upsample_initial_channel >> (i + 1)
        assert r["C"] == C, (i, r)
        ran = {p for p, nms in KERNELS_OF.items() for nm in nms if nm % C in names}
        assert ran == {r["path"]}, "stage %d (C = %d) reports %s, the profiler saw %s" % (i, C, r["path"], sorted(names))
        if r["path"] == "PAIR":
            levels = max(len(d) for d in cfg.resblock_dilation_sizes)
            assert ("rb_stream1_c%d" % C in names) == (r["pair_streamed"] != 0) and ("rb_pair_c%d" % C in names) == (r["pair_streamed"] != (1 << levels) - 1), (r, sorted(names))
        out.append("FULL%d" % r["tile_rows"] if r["path"] == "FULL" else r["path"])
    return out


def check_plan(c, plan, paths, ncu):
    """The report of case ``c``'s forward against the restated rules: paths, stream dtypes, tile and strip counts"""
    cfg, cid = CONFIGS[c.cfg], case_id(c)
    for i, p in c.want:
        assert paths[i] == p, "%s: stage %d ran on %s, the case is there for %s" % (cid, i, paths[i], p)
    for i, p in enumerate(expected_paths(cfg, c.B, c.T, c.opts, ncu)):
        assert p == paths[i] if p is not None else paths[i] in ("STREAM", "PAIR"), "%s: stage %d ran on %s, plan_stage restated says %s" % (cid, i, paths[i], p)
    x0h, yh = stream_plan(paths, c.opts)
    assert (tuple(r["x0_half"] for r in plan), tuple(r["y_half"] for r in plan)) == (x0h, yh), "%s: stream dtypes %s, restated %s" % (cid, plan, (x0h, yh))
    for r, L in zip(plan, stage_rows(cfg, c.T)):
        assert (r["B"], r["rows"], r["num_cus"]) == (c.B, L, ncu), (cid, r)
        tiles = dict(zip(r["k"], r["tiles"]))
        if r["path"] == "FULL":
            assert tiles == full_tile_counts(cfg, L, r["tile_rows"]), (cid, r)
        elif r["path"] == "PAIR":
            assert r["tile_rows"] == RB_ROWS and tiles == pair_tile_counts(cfg, L), (cid, r)
        elif r["path"] == "STREAM":
            assert sorted(r["k"]) == sorted(cfg.resblock_kernel_sizes) and all(n * s >= L > (n - 1) * s for n, s in zip(r["tiles"], r["strip_len"])), (cid, r)


# ---- errors and bars ---------------------------------------------------------------------------------------------------------------------

def ulp16(v):
    v = max(abs(float(v)), 2.0 ** -14)
    return 2.0 ** (math.floor(math.log2(v)) - 10)


def ulp32(v):
    v = max(abs(float(v)), 2.0 ** -126)
    return 2.0 ** (math.floor(math.log2(v)) - 23)


def err(got, want):
    """-> (RMS, max-abs) of got - want, in float64"""
    e = torch.as_tensor(got).double() - torch.as_tensor(want).double()
    return (float(e.pow(2).mean().sqrt()), float(e.abs().max())) if e.numel() else (0.0, 0.0)


def bars_of(y32, y64, half_out, kind="mfma"):
    factor = FACTOR[kind]
    floor_rms, floor_max = err(y32, y64)
    one = (ulp16 if half_out else ulp32)(float(y64.abs().max()))
    return {"floor_rms": floor_rms, "floor_max": floor_max, "bar_rms": factor * floor_rms + one / math.sqrt(y64.numel()), "bar_max": factor * floor_max + one,
            "add_rms": one / math.sqrt(y64.numel()), "add_max": one}


def half_out(name, x0_half, y_half):
    """Is layer ``name``'s tap stored as fp16?"""
    if name.startswith("up"):
        return x0_half[int(name[-1])]
    if name.startswith("stage"):
        return y_half[int(name[-1])]
    return False


def make_layers(c, paths, arith, perturb=None, operand="case", halves=None):
    """halves: (x0_half, y_half) per stage as a forward reported them; None = the restated rule"""
    x0h, yh = halves or stream_plan(paths, c.opts)
    return lo.Layers(CONFIGS[c.cfg], weights(c.cfg, c.seed, c.wgain), arith, c.operand if operand == "case" else operand, x0h, yh, perturb)


def layer_bars(c, paths, name, taps, halves=None):
    """The fp64 oracle of layer ``name`` applied to ``taps`` (whatever feeds it), its fp32 evaluation on the same input, and the bars."""
    x0h, yh = halves or stream_plan(paths, c.opts)
    with torch.no_grad():
        y64 = lo.apply_layer(make_layers(c, paths, "f64", halves=halves), name, taps)
        y32 = lo.apply_layer(make_layers(c, paths, "f32", halves=halves), name, taps)
    return {"y": y64, "y32": y32, **bars_of(y32, y64, half_out(name, x0h, yh), kind_of(name))}


def layer_list(c):
    names = lo.layer_names(CONFIGS[c.cfg])
    return names if c.layers is None else [n for n in names if n in c.layers]


def feeds(cfg, name):
    """The taps layer ``name`` consumes"""
    n = len(cfg.upsample_rates)
    if name == "pre":
        return ["z", "g"]
    if name == "post":
        return ["stage%d" % (n - 1)]
    i = int(name[-1])
    if name.startswith("up"):
        return (["pre"] if i == 0 else ["stage%d" % (i - 1)]) + (["har"] if cfg.use_f0 else [])
    return ["up%d" % i]


@functools.lru_cache(maxsize=None)
def cpu_chain(c):
    """No GPU: the fp32 evaluation composed end to end stands in for the device (``taps``: its taps; "post" = its waveform), and for every layer the
    bars on that evaluation's own previous tap.  Computed once per case, never changed."""
    cfg, x = CONFIGS[c.cfg], inputs(c)
    paths = [p or "PAIR" for p in expected_paths(cfg, c.B, c.T, c.opts)]
    taps = {"z": x["z"], "g": x["g"], "har": cpu_har(c)}
    with torch.no_grad():
        taps["post"] = make_layers(c, paths, "f32").forward(x["z"], x["g"], taps["har"], taps)
    bars = {name: layer_bars(c, paths, name, taps) for name in layer_list(c)}
    return {"paths": paths, "taps": taps, "bars": bars}


# ---- one case on the device (tests/test_gpu_nsf_layers.py, tools/nsf_parity.py) -----------------------------------------------------------

def device_case(c, device, items=False):
    """Run case ``c`` on ``device``: pin the options, take the waveform of a plain forward (profiled, and its own report of how it ran: ``check_plan``)
    and every tap the case's layers need -- each fetched twice, bit-equal -- and compare every layer's tap with the fp64 oracle of that layer applied to
    the DEVICE's previous tap.  -> (record, wave, handle); record = {"case", "paths", "plan", "kernels", "layers": [{"layer", "item", "rms", "max",
    floor / bar fields}]} holds plain data only; ``items``: per batch item."""
    import rvc_amd

    cfg, x, w = CONFIGS[c.cfg], inputs(c), weights(c.cfg, c.seed, c.wgain)
    cls = rvc_amd.NSFGeneratorHIP if cfg.use_f0 else rvc_amd.GeneratorHIP
    gen = cls(vars(cfg), w, device=device, operand=c.operand, max_B=c.B, max_T=c.T)
    for k, v in c.opts:
        gen.set_option(k, v)
    z, g = x["z"].to(device), x["g"].to(device)
    if cfg.use_f0:
        f0, noise = x["f0"].to(device), x["noise"].to(device)
        run = lambda: gen(z, f0, g, noise=noise)
        tap = lambda what: gen.debug_tap(what, z, f0, g, noise=noise)
    else:
        run = lambda: gen(z, g)
        tap = lambda what: gen.debug_tap(what, z, g)
    gen.profile(True)
    wave = run().cpu()
    names = {s["name"] for s in gen.profile_read()}
    gen.profile(False)
    plan = gen.last_plan()
    paths = paths_from_plan(cfg, plan, names)
    check_plan(c, plan, paths, torch.cuda.get_device_properties(device).multi_processor_count)
    halves = tuple(r["x0_half"] for r in plan), tuple(r["y_half"] for r in plan)
    layers = layer_list(c)
    need = sorted({t for n in layers for t in feeds(cfg, n)} | set(layers) - {"post"} - {"z", "g"})
    taps = {"z": x["z"], "g": x["g"]}
    for what in need:
        if what in ("z", "g"):
            continue
        a, b = tap(what), tap(what)
        assert torch.equal(a, b), "%s: tap %s differs between two calls" % (case_id(c), what)
        assert bool(torch.isfinite(a).all()), what
        taps[what] = a
    # the taps above were cut out of forwards that ended early; the plain forward ran again behind them on the same handle and must not have moved
    wave2 = run().cpu()
    assert torch.equal(wave, wave2), "%s: the waveform differs between two forwards" % case_id(c)
    taps["post"] = wave
    out = []
    for name in layers:
        for b in (range(c.B) if items else (None,)):
            sl = (lambda t: t) if b is None else (lambda t: None if t is None else t[b:b + 1])
            lb = layer_bars(c, paths, name, {k: sl(taps.get(k)) for k in feeds(cfg, name)}, halves)
            got = sl(taps[name])
            assert got.shape == lb["y"].shape, (name, got.shape, lb["y"].shape)
            rms, mx = err(got, lb["y"])
            out.append({"layer": name, "item": b, "rms": rms, "max": mx, **{k: lb[k] for k in ("floor_rms", "floor_max", "bar_rms", "bar_max")},
                        "rms_ratio": rms / lb["floor_rms"] if lb["floor_rms"] else None, "max_ratio": mx / lb["floor_max"] if lb["floor_max"] else None,
                        "within_bars": bool(rms <= lb["bar_rms"] and mx <= lb["bar_max"])})
    rec = {"case": case_id(c), "paths": paths, "plan": plan, "kernels": sorted(n for n in names if n.startswith("rb_") or n == "conv_post"), "layers": out}
    return rec, wave, gen
