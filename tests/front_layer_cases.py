"""The front's kernels (csrc/front.hip, front_kernels.hpp) in their DEFAULT arithmetic (fp16 / bf16 operands), SEGMENT BY SEGMENT against the float64
oracle that rounds where they round (oracle/front_layer_oracle.py).  Shared by tests/test_cpu_front_layers.py, tests/test_gpu_front_layers.py and
tools/front_layer_parity.py: the cases, the bars and the one function that runs a case on a device.

THE BARS (the recipe of 2.1).  For one segment on one input x (on the GPU: the tap the DEVICE produced for the segment in front of it):

    floor = | segment(x) in float32  -  segment(x) in float64 |   same input, same roundings: RMS and max-abs (but see A FLOOR IS A SAMPLE)
    bar   = FACTOR[kind] * floor + one ulp at max |y| of the tap's storage type (fp32), over sqrt(n) for the RMS bar

FACTOR = 2 x the largest ratio to the floor that the kernels' liberties reach on the CPU (``PERTURB_WORST``, measured by
test_cpu_front_layers.py::test_perturbations_stay_inside_half_the_bars over CPU_TABLE x 2 seeds), rounded up to the next half.  The liberties
(``PERTURB``, oracle/front_layer_oracle.py): every K loop summed one MFMA k-step (16 channels) at a time in a permuted order; the split FFN's four
partial sums and the tap-split gate's per-tap partial sums, each added in a permuted order; the online softmax's 32-key tiles dealt to the four
waves in a permuted order; the hardware exp behind softmax / sigmoid / tanh as exp2 of the float32-rounded x * log2(e), moved by +-1 ulp.

    The 1 ulp of v_exp_f32 is an ASSUMPTION: it is the accuracy the AMD GCN / CDNA instruction-set manuals state for V_EXP_F32 as the author recalls
    them; no copy was at hand to cite a page from, and nothing here measures the instruction.  The float32 rounding of x * log2(e) in front of it is
    the larger term anyway (|x| up to ~20 in a softmax: ~12 ulp of p), and both are small against the 2^-11 operand rounding of p that follows.

A FLOOR IS A SAMPLE, and at the sizes the edge cases need it is a sample of almost nothing.  Against float64 the float32 evaluation differs by its
accumulation noise (1e-7 class) and by the operand roundings that fall the other way: rare, discrete, each worth 1e-4 - 1e-3 on one output row.  With fp16
operands 133 of the 115200 q / k / v values of attn0 flip at B = 2, T = 100 (one in 870), with bf16 operands 6 (one in 19000): a few at T <= 11, fewer than
one per projection with bf16 at T = 65.  A case whose float32 evaluation happens to flip nothing has a floor of 1e-7, and ANY correct evaluation that flips
one value misses every multiple of it: measured here before the pooling below, the perturbed evaluations reached 22x their case's own floor at T = 1
(attn0), 287x / 802x with bf16 operands at B = 2, T = 65 (layer4 RMS, attn1 max-abs) -- against <= 3.6x wherever the floor holds a few dozen flips.
So the floor a bar is built on is the case's own or that of its POPULATED SIBLING, whichever is larger: the same segment, config, operand type, weights
and kind of input at T = 128, ragged, B = 2 (fp16) or 8 (bf16), evaluated on the CPU alone (``pool_case`` / ``pool_floor``):

    max-abs:  max(own floor, sibling's floor)                     one flip is worth the same on 2 rows as on 229
    RMS:      max(own floor, sqrt(sibling_rms^2 + r2 / n))        r2 = the sibling's largest squared error norm of ONE row: the expected density of
                                                                  flips plus one whole flipped row, which is what n elements can always hold

The price, plainly: a small case's RMS bar is up to ~8x a populated case's (attn0 at T = 1: 1.1e-3 against 1.4e-4 at T = 100) -- at T = 1 a defect has to be worth one
flipped row to show in RMS; the max-abs bar does not grow.  And PERTURB_WORST / FACTOR below are ratios to this floor, not to the case's own.

At B = 2, T = 100 the floor used is the case's own or within its sampling spread (measured: attn<i> <= 1.15x RMS / 1.5x max-abs, layer<i> <= 2.2x / 4.4x
-- a float32 FFN flips a handful of ReLU outputs, its floor is the noisiest); both floors are in every record.  This is where the recipe departs from
"per segment and per case": without it the bars of the small and the bf16 cases would be set by chance.

NEAR-TIES OF THE HIDDEN ACTIVATION.  The bars are not the place for a rounding that is genuinely open.  A hidden value of the FFN whose exact value lies within
2 float32 ulps of the midpoint between two operand values is rounded either way by a correct float32 K loop, depending on its summation order, and with bf16
operands one such rounding at |h| = 4.7 is worth 1.2e-3 on the tap.  For "layer<i>" the comparison therefore resolves every near-tie the way the tap under test
has it (``tie_resolved``: greedy, only values the oracle itself finds within ``flo.TIE_FP32_ULPS`` of a midpoint, at most a few per layer; the counts are in every
record) and then compares as usual; floor, FACTOR and bars are what they were.  The first GPU run is why: "layer2" of the four bf16 cases with an unsplit conv_2
missed its RMS bar by 5 %, and that error was ONE hidden value (4.7031, 0.7 float32 ulp from the midpoint) -- DESIGN.md 2.2.
test_cpu_front_layers.py::test_a_near_tie_passes_rounded_either_way_and_nothing_else_does restates it.

Measured on the CPU before anything ran on a GPU (RMS ratio / max-abs ratio to the floor used, the larger over CPU_TABLE x seeds 1, 2; a bar the additive
ulp term decides does not count) -- see PERTURB_WORST below.  The floors themselves (fp16 operands, seed 77, B = 2, T = 100, lengths (100, 91)):
emb 3.4e-7 RMS / 2.7e-6 max-abs (fp32 accumulation alone), attn<i> 2.1-3.0e-5 / 2.4-5.0e-4, layer<i> 2.3-5.2e-6 / 4.1-7.9e-5, z_p 2.4e-7 / 2.2e-6,
flow<f> 1.3-1.6e-4 / 1.0-1.2e-3 on outputs of max |y| 4-7.  A floor is the roundings that fall the other way in float32: q, k, v, P and the
attention output in attn<i>; the ReLU output in layer<i>; three gate outputs per coupling and the fp32 WN stream re-staged in front of every in_layer in
flow<f> (why the flow's floor is the largest).  The code under test never sets a bar.
"""
import collections
import functools
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import front_layer_oracle as flo  # noqa: E402
from oracle import synth  # noqa: E402
from oracle.front_oracle import FrontConfig  # noqa: E402

PERTURB = {"reorder": True, "softmax": True, "exp": 1}
KINDS = ("emb", "attn", "ffn", "z_p", "flow", "out")
# largest perturbed / floor ratio (RMS or max-abs) per kind over CPU_TABLE x seeds (1, 2); FACTOR = 2 x that, rounded up to the next half.  "out" moves
# values and multiplies by 0 or 1: its floor is 0, no liberty exists, the bar is the additive ulp and the GPU test asks for bit-equality besides.
# fp16 operands: emb 0.67, attn 2.19 (attn0 of cpu-w15-k7, max-abs), ffn 2.01 (layer1 of cpu-T33, RMS), z_p 0.44, flow 1.19 (cpu-T161);
# bf16 operands: emb 1.34, attn 1.56, ffn 2.57 (layer5 of cpu-bf16-T65, RMS), z_p 0.92, flow 1.18.  One FACTOR per kind: from the larger of the two.
# ffn: as derived before the first GPU run, with the layer<i> comparison not yet tie-aware; tie-aware, the same evaluations reach 1.00 at most, and the FACTOR
# stays.  z_p and flow: re-measured once the permuted order also covered the attention's products and merge (other draws of the same permutations: 0.79 -> 0.92,
# 1.14 -> 1.19; attn unchanged at 2.19); every FACTOR is what it was.
PERTURB_WORST = {"emb": 1.34, "attn": 2.19, "ffn": 2.57, "z_p": 0.92, "flow": 1.19, "out": 0.0}
FACTOR = {"emb": 3.0, "attn": 4.5, "ffn": 5.5, "z_p": 2.0, "flow": 2.5, "out": 1.0}


def kind_of(name):
    for k, kind in (("attn", "attn"), ("layer", "ffn"), ("flow", "flow")):
        if name.startswith(k):
            return kind
    return name


# cfg: FrontConfig overrides as a sorted tuple of (key, value).  opts: the handle options that pin the launch forms.  lengths: None = every item full.
# inputs: "synth" (oracle/synth.py's draws) / "pitch_edges" (the pitch track runs through bins 1 and 255) / "zero_phone".  gain: weights x 2.5 on one
# conv per segment kind.  segments: None = every segment, else prefixes of the segments compared.
Case = collections.namedtuple("Case", "name B T lengths fh opts operand cfg seed inputs gain segments", defaults=(None, 0, (), "fp16", (), 77, "synth", False, None))


def O(**kw):
    return tuple(sorted(kw.items()))


# the launch forms (csrc/front.hip pick_nj, launch_ffn*, launch_wn*): tile height x FFN form x WN form
F_DEFAULT = O(FR_NJ=1, FR_FFN_SPLIT=1, FR_WN_SPLIT=2)                       # what a single clip runs: k_fr_ffn_part<1> + k_fr_ffn_ln, k_fr_gate_ks + res_skip launch
F_FUSED1 = O(FR_NJ=1, FR_FFN_SPLIT=0, FR_WN_SPLIT=0)                        # k_fr_ffn<1>, k_fr_wn<1>
F_FUSED2 = O(FR_NJ=2, FR_FFN_SPLIT=0, FR_WN_SPLIT=0)                        # k_fr_ffn<2>, k_fr_wn<2> (what a large batch runs)
F_SPLIT2 = O(FR_NJ=2, FR_FFN_SPLIT=1, FR_WN_SPLIT=0)                        # k_fr_ffn_part<2>
F_UNFUSED1 = O(FR_NJ=1, FR_NO_FFN_FUSION=1, FR_WN_SPLIT=1)                  # 32-row conv tiles: enc_ffn1 + enc_ffn2_ln; FR_GATE + res_skip, channel split
F_UNFUSED2 = O(FR_NJ=2, FR_NO_FFN_FUSION=1, FR_WN_SPLIT=0)                  # 64-row conv tiles
FORMS = {"default": F_DEFAULT, "fused1": F_FUSED1, "fused2": F_FUSED2, "split2": F_SPLIT2, "unfused1": F_UNFUSED1, "unfused2": F_UNFUSED2}

ENC = ("emb", "attn", "layer")
TIME_CASES = tuple(Case("T%d-default" % T, 1, T, opts=F_DEFAULT) for T in (1, 2, 11, 30, 31, 32, 33, 64, 65)) + tuple(
    # the fused FFN's valid rows per tile: 30 at FR_NJ = 1, 62 at FR_NJ = 2; the 32- / 64-row tiles of everything else
    Case("T%d-fused1" % T, 1, T, opts=F_FUSED1) for T in (30, 31, 33, 65)) + tuple(
    Case("T%d-fused2" % T, 1, T, opts=F_FUSED2) for T in (60, 61, 62, 63, 65)) + tuple(
    Case("T%d-split2" % T, 1, T, opts=F_SPLIT2, segments=ENC) for T in (62, 63)) + tuple(
    Case("T%d-unfused1" % T, 1, T, opts=F_UNFUSED1) for T in (33, 65)) + (
    Case("T64-unfused2", 1, 64, opts=F_UNFUSED2), Case("T65-unfused2", 1, 65, opts=F_UNFUSED2), Case("T64-fused2", 1, 64, opts=F_FUSED2))
ATTN_CASES = (
    Case("attn-T97-plain", 1, 97, opts=F_DEFAULT),                    # key tile 3 of query tile 0 is the first `plain` tile
    Case("attn-T97-len80", 1, 97, lengths=(80,), opts=F_DEFAULT),     # ... and must take the general path
    Case("attn-T129", 1, 129, opts=F_DEFAULT),                        # fifth key tile: wave 0 walks two
    Case("attn-T161", 1, 161, opts=F_DEFAULT),                        # sixth: wave 1 too
    Case("attn-ragged", 2, 70, lengths=(45, 1), opts=F_DEFAULT),                          # a length ending mid-tile, a length of 1
    Case("attn-window4", 1, 40, opts=F_DEFAULT, cfg=O(window_size=4), segments=ENC),
    Case("attn-window15", 1, 40, opts=F_DEFAULT, cfg=O(window_size=15), segments=ENC),    # k_fr_attn<., 96, 31>
)
FLOW = ("z_p", "flow", "out")
FLOW_CASES = (
    Case("flow-head6", 1, 70, fh=6, opts=F_DEFAULT),
    Case("flow-head-last", 2, 33, lengths=(33, 20), fh=32, opts=F_DEFAULT),               # flow_head = T - 1: one row left
) + tuple(Case("flow-k%d-wn%d" % (k, m), 1, 40, opts=O(FR_NJ=1, FR_FFN_SPLIT=1, FR_WN_SPLIT=m), cfg=O(flow_kernel_size=k), segments=FLOW + ("layer5",))
          for k in (3, 7) for m in (0, 2))
BF16_CASES = tuple(Case("bf16-%s" % n, 2, 65, lengths=(65, 40), opts=o, operand="bf16") for n, o in FORMS.items())
INPUT_CASES = (
    Case("v1-in256", 2, 33, lengths=(33, 17), opts=F_DEFAULT, cfg=O(in_channels=256)),
    Case("no-f0", 1, 33, opts=F_DEFAULT, cfg=O(use_f0=False)),
    Case("gain2.5", 1, 40, opts=F_DEFAULT, gain=True),
    Case("pitch-edges", 1, 40, opts=F_DEFAULT, inputs="pitch_edges", segments=("emb", "attn0", "layer0")),
    Case("zero-phone", 1, 40, opts=F_DEFAULT, inputs="zero_phone"),
    # an ODD number of couplings: the folded Flips leave the stream channel-reversed at the end, k_fr_out must hand out the logical order
    Case("flows3", 1, 33, opts=F_DEFAULT, cfg=O(flow_n_flows=3), segments=FLOW),
)
TABLE = TIME_CASES + ATTN_CASES + FLOW_CASES + BF16_CASES + INPUT_CASES
BATCH_CASES = (Case("batch-default", 2, 65, lengths=(65, 50), opts=F_DEFAULT), Case("batch-fused2", 2, 65, lengths=(65, 50), opts=F_FUSED2))

# the CPU cases the FACTORs are measured on: the issue's measuring case, a ragged one past four key tiles, the window-15 / flow-k7 config, bf16, one row
CPU_MAIN = Case("cpu-T100", 2, 100, lengths=(100, 91))
CPU_TABLE = (CPU_MAIN, Case("cpu-T161", 2, 161, lengths=(161, 70), seed=78), Case("cpu-w15-k7", 1, 40, cfg=O(window_size=15, flow_kernel_size=7), seed=79),
             Case("cpu-T1", 1, 1, seed=81), Case("cpu-T11", 1, 11, seed=83), Case("cpu-head6", 1, 70, fh=6, seed=82), Case("cpu-T33", 2, 33, lengths=(33, 20)),
             Case("cpu-bf16-T65", 2, 65, lengths=(65, 40), operand="bf16", seed=80), Case("cpu-bf16-T33", 1, 33, operand="bf16"),
             Case("cpu-bf16-T100", 2, 100, lengths=(100, 91), operand="bf16"))

GAIN_CONVS = ("enc_p.emb_phone.weight", "enc_p.encoder.attn_layers.1.conv_q.weight", "enc_p.encoder.ffn_layers.2.conv_1.weight",
              "enc_p.proj.weight", "flow.flows.2.enc.in_layers.0.weight")


def case_id(c):
    return c.name


def config(c):
    return FrontConfig(**dict(c.cfg))


@functools.lru_cache(maxsize=None)
def weights(c):
    w = synth.make_front_weights(config(c), c.seed)
    if c.gain:
        for k in GAIN_CONVS:
            w[k] = w[k] * 2.5
    return w


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> {"phone", "pitch", "lengths", "g", "noise", "flow_head"}; never changed afterwards."""
    cfg, w = config(c), weights(c)
    phone = synth.make_phone(c.B, c.T, cfg.in_channels, c.seed)
    if c.inputs == "zero_phone":
        phone = torch.zeros_like(phone)
    pitch = synth.make_pitch(synth.make_f0(c.B, c.T)) if cfg.use_f0 else None
    if c.inputs == "pitch_edges":
        pitch = pitch.clone()
        pitch[:, 0::3] = 1
        pitch[:, 1::3] = 255
        assert int(pitch.min()) == 1 and int(pitch.max()) == 255
    lengths = torch.tensor(c.lengths if c.lengths is not None else (c.T,) * c.B)
    sid = (1 + 6 * torch.arange(c.B)) % cfg.spk_embed_dim
    noise = torch.randn(c.B, cfg.inter_channels, c.T - c.fh, generator=torch.Generator().manual_seed(c.seed + 3))
    return {"phone": phone, "pitch": pitch, "lengths": lengths, "g": w["emb_g.weight"][sid].unsqueeze(-1), "sid": sid, "noise": noise, "flow_head": c.fh}


def segment_list(c):
    names = flo.segment_names(config(c))
    return names if c.segments is None else [n for n in names if n.startswith(tuple(c.segments))]


def make_segments(c, arith, perturb=None, variants=None, operand="case"):
    return flo.Segments(config(c), weights(c), arith, c.operand if operand == "case" else operand, perturb, variants)


# ---- errors and bars ---------------------------------------------------------------------------------------------------------------------

def ulp32(v):
    v = max(abs(float(v)), 2.0 ** -126)
    return 2.0 ** (math.floor(math.log2(v)) - 23)


def compared(c, name, t):
    """The elements of tap ``name`` that are compared: encoder taps on the rows below the length (LayerNorm outputs behind it are arbitrary by design);
    "z_p", "flow<f>" and z whole."""
    t = torch.as_tensor(t)
    if kind_of(name) in ("emb", "attn", "ffn"):
        rows = torch.arange(c.T).unsqueeze(0) < inputs(c)["lengths"].unsqueeze(1)
        return t[rows]
    return t


def err(got, want):
    """-> (RMS, max-abs) of got - want, in float64"""
    e = torch.as_tensor(got).double() - torch.as_tensor(want).double()
    return (float(e.pow(2).mean().sqrt()), float(e.abs().max())) if e.numel() else (0.0, 0.0)


def rows_of(t):
    """[rows, channels] view of a compared tap (every tap is channels-last; z is not compared row-wise: its floor is 0)"""
    return t.reshape(-1, t.shape[-1])


def evaluations(c, name, taps):
    """Segment ``name`` applied to ``taps`` (the raw inputs and the tap in front of it) in float64 and in float32, on the compared elements."""
    feed = {**inputs(c), **taps}
    with torch.no_grad():
        y64 = compared(c, name, flo.apply_segment(make_segments(c, "f64"), name, feed))
        y32 = compared(c, name, flo.apply_segment(make_segments(c, "f32"), name, feed))
    return y32, y64


def pool_case(c):
    """The POPULATED sibling of a case: the same config, operand, weights and kind of input at T = 128, ragged, no flow_head; B = 2 for fp16 operands
    and 8 for bf16, whose roundings fall the other way an eighth as often."""
    lengths = (128, 101, 128, 77, 115, 128, 90, 128)
    B = 2 if c.operand == "fp16" else 8
    return c._replace(name="pool", B=B, T=128, lengths=lengths[:B], fh=0, opts=(), segments=None)


@functools.lru_cache(maxsize=None)
def pool_floor(p):
    """{segment: floor of the sibling ``p`` = pool_case(c)}: RMS, max-abs, and ``row2``: the largest squared error norm of ONE row.  CPU only, once per sibling."""
    x, taps, out = inputs(p), {}, {}
    with torch.no_grad():
        make_segments(p, "f32").forward(x["phone"], x["pitch"], x["lengths"], x["g"], x["noise"], p.fh, taps)
    for name in flo.segment_names(config(p)):
        y32, y64 = evaluations(p, name, taps)
        e = rows_of(y32.double() - y64)
        out[name] = {"rms": float(e.pow(2).mean().sqrt()), "max": float(e.abs().max()), "row2": float(e.pow(2).sum(dim=1).max())}
    return out


def bars_of(y32, y64, kind, pool):
    """``floor_*``: this input's own floor, as measured.  ``eff_*``: the floor the bar is built on -- see the module docstring, "a floor is a SAMPLE"."""
    factor = FACTOR[kind]
    floor_rms, floor_max = err(y32, y64)
    one = ulp32(float(y64.abs().max())) if y64.numel() else 0.0
    n = max(1, y64.numel())
    eff_max = max(floor_max, pool["max"])
    eff_rms = max(floor_rms, math.sqrt(pool["rms"] ** 2 + pool["row2"] / n))
    return {"floor_rms": floor_rms, "floor_max": floor_max, "eff_rms": eff_rms, "eff_max": eff_max,
            "bar_rms": factor * eff_rms + one / math.sqrt(n), "bar_max": factor * eff_max + one, "add_rms": one / math.sqrt(n), "add_max": one}


def tie_resolved(c, name, taps, got):
    """The float64 oracle of "layer<i>" on the compared elements, with every NEAR-TIE of the hidden activation rounded the way ``got`` (the whole tap under
    test) has it -> (y, number of near-ties, number rounded away from nearest).  A hidden value whose exact pre-rounding value lies within
    flo.TIE_FP32_ULPS float32 ulps of the midpoint between two operand values is rounded either way by a correct float32 K loop, depending on its summation
    order; the oracle cannot know which, so both are right.  Greedy, one near-tie after the other: the other rounding is kept where it brings the oracle closer
    to ``got`` in the squared error.  Nothing else is adjusted: a value that is not a near-tie keeps its nearest rounding, and the bars stay what they are."""
    i = int(name[5:])
    sg = make_segments(c, "f64")
    with torch.no_grad():
        head = sg.ffn_head(i, taps[flo.feed_of(config(c), name)], inputs(c)["lengths"])
        g = compared(c, name, got).double()
        y = compared(c, name, sg.ffn_tail(i, head))
        best, flipped = float((g - y).pow(2).sum()), []
        for idx in head["ties"]:
            y2 = compared(c, name, sg.ffn_tail(i, head, flipped + [idx]))
            e2 = float((g - y2).pow(2).sum())
            if e2 < best:
                best, flipped, y = e2, flipped + [idx], y2
    return y, len(head["ties"]), len(flipped)


def segment_bars(c, name, taps, got=None):
    """The float64 oracle of segment ``name`` applied to ``taps``, its float32 evaluation on the same input, and the bars -- all on the compared elements.
    ``got``: the tap under test; for "layer<i>" the reference ``y`` is then the tie-resolved one (``tie_resolved``; the floor and the bars are not touched)."""
    y32, y64 = evaluations(c, name, taps)
    b = {"y": y64, "y32": y32, "ties": 0, "ties_flipped": 0, **bars_of(y32, y64, kind_of(name), pool_floor(pool_case(c))[name])}
    if got is not None and kind_of(name) == "ffn" and c.operand is not None:
        b["y"], b["ties"], b["ties_flipped"] = tie_resolved(c, name, taps, got)
    return b


@functools.lru_cache(maxsize=None)
def cpu_chain(c):
    """No GPU: the rounded float32 evaluation composed end to end stands in for the device (``taps``), and for every segment the bars on that evaluation's
    own previous tap.  Computed once per case, never changed."""
    x = inputs(c)
    taps = {}
    with torch.no_grad():
        make_segments(c, "f32").forward(x["phone"], x["pitch"], x["lengths"], x["g"], x["noise"], c.fh, taps)
    return {"taps": taps, "bars": {name: segment_bars(c, name, taps) for name in flo.segment_names(config(c))}}


def compare(c, name, got, b):
    """One record: tap ``got`` of segment ``name`` against the bars ``b``."""
    g = compared(c, name, got)
    assert g.shape == b["y"].shape, (name, g.shape, b["y"].shape)
    rms, mx = err(g, b["y"])
    return {"segment": name, "rms": rms, "max": mx, **{k: b[k] for k in ("floor_rms", "floor_max", "eff_rms", "eff_max", "bar_rms", "bar_max", "ties", "ties_flipped")},
            "rms_ratio": rms / b["eff_rms"] if b["eff_rms"] else None, "max_ratio": mx / b["eff_max"] if b["eff_max"] else None,
            "within_bars": bool(rms <= b["bar_rms"] and mx <= b["bar_max"])}


# ---- which launch forms run ------------------------------------------------------------------------------------------------------------------

def expected_forms(cfg, B, T, fh, opts):
    """csrc/front.hip restated: pick_nj (:83-89), the FFN's choice (:368-382), launch_wn_op / launch_wn_split (:172,219-224)."""
    o = dict(opts)
    nj = int(o["FR_NJ"]) if o.get("FR_NJ") in (1, 2) else (2 if B * ((T + 63) // 64) >= 192 else 1)
    if cfg.kernel_size > 5 or o.get("FR_NO_FFN_FUSION"):
        ffn = "unfused"
    else:
        tiles = ((T + 32 * nj - 3) // (32 * nj - 2)) * B
        split = cfg.kernel_size == 3 and cfg.filter_channels == 768 and B * T <= 8192 and o.get("FR_FFN_SPLIT", 1 if tiles <= 96 else 0) != 0
        ffn = "split" if split else "fused"
    T2 = T - fh
    nj2 = int(o["FR_NJ"]) if o.get("FR_NJ") in (1, 2) else (2 if B * ((T2 + 63) // 64) >= 192 else 1)
    tiles = ((T2 + 32 * nj2 - 1) // (32 * nj2)) * B
    if nj2 == 1 and o.get("FR_WN_SPLIT", 1 if tiles <= 96 else 0) != 0:
        wn = "split_taps" if o.get("FR_WN_SPLIT", 2) == 2 and 2 <= cfg.flow_kernel_size <= 8 else "split_channels"
    else:
        wn = "one_launch"
    return {"nj": nj, "nj_flow": nj2, "ffn": ffn, "wn": wn}


FFN_NAMES = {"fused": {"enc_ffn_ln"}, "split": {"enc_ffn_part", "enc_ffn_ln"}, "unfused": {"enc_ffn1", "enc_ffn2_ln"}}
WN_NAMES = {"one_launch": {"flow_wn", "flow_wn_last"}, "split_taps": {"flow_wn_gate", "flow_wn_rs"}, "split_channels": {"flow_wn_gate", "flow_wn_rs"}}


def observed_forms(names):
    """What the profiler's kernel names tell: the FFN's form, and whether a WN layer was one launch or two.  One name covers both tile heights, and
    "flow_wn_gate" both split modes: those stay as computed."""
    ffn = [k for k, v in FFN_NAMES.items() if v == {n for n in names if n.startswith("enc_ffn")}]
    wn = "one_launch" if "flow_wn" in names else ("two_launches" if "flow_wn_gate" in names else None)
    return {"ffn": ffn[0] if ffn else None, "wn": wn}


# ---- one case on the device ------------------------------------------------------------------------------------------------------------------

def device_case(c, device):
    """Run case ``c`` on ``device``: pin the options, take z of a plain forward (profiled: which kernels ran) and every tap the case's segments need -- each
    fetched twice, bit-equal -- and compare every segment's tap with the float64 oracle of that segment applied to the DEVICE's previous tap.
    -> (record, z, handle); the record holds plain data only."""
    import rvc_amd

    cfg, x = config(c), inputs(c)
    fr = rvc_amd.FrontHIP(vars(cfg), weights(c), device=device, operand=c.operand, max_B=c.B, max_T=c.T)
    for k, v in c.opts:
        fr.set_option(k, v)
    dv = lambda t: None if t is None else t.to(device)
    args = (dv(x["phone"]), dv(x["pitch"]), dv(x["lengths"]), dv(x["g"]))
    nz = dv(x["noise"])
    run = lambda: fr(*args, c.fh, noise=nz).cpu()
    fr.profile(True)
    z = run()
    names = {s["name"] for s in fr.profile_read()}
    fr.profile(False)
    want, seen = expected_forms(cfg, c.B, c.T, c.fh, c.opts), observed_forms(names)
    assert seen["ffn"] == want["ffn"], "%s: the FFN ran as %s (kernels %s), the case pins %s" % (c.name, seen["ffn"], sorted(names), want["ffn"])
    assert WN_NAMES[want["wn"]] <= names and (want["wn"] == "one_launch") == (seen["wn"] == "one_launch"), \
        "%s: a WN layer ran as %s (kernels %s), the case pins %s" % (c.name, seen["wn"], sorted(names), want["wn"])
    segs = segment_list(c)
    need = sorted({flo.feed_of(cfg, n) for n in segs if n != "emb"} | set(segs) - {"out"})
    taps = {}
    for what in need:
        a, b = fr.debug_tap(what, *args, c.fh, noise=nz), fr.debug_tap(what, *args, c.fh, noise=nz)
        assert torch.equal(a, b), "%s: tap %s differs between two calls" % (c.name, what)
        assert bool(torch.isfinite(a).all()), what
        taps[what] = a
    z2 = run()
    assert torch.equal(z, z2), "%s: z differs between two forwards" % c.name
    taps["out"] = z
    T2 = c.T - c.fh
    beyond = (torch.arange(T2).unsqueeze(0) + c.fh) >= x["lengths"].unsqueeze(1)  # [B, T2]
    for what in need:
        if kind_of(what) in ("z_p", "flow"):
            assert float(taps[what][beyond].abs().max() if beyond.any() else 0.0) == 0.0, "%s: %s is not 0 at or beyond the length" % (c.name, what)
    assert float(z.transpose(1, 2)[beyond].abs().max() if beyond.any() else 0.0) == 0.0, "%s: z is not 0 at or beyond the length" % c.name
    if "flow0" in taps:  # the taps ARE the real run: the last flow tap, transposed and masked, is the forward's z bit for bit
        zt = taps["flow0"].masked_fill(beyond.unsqueeze(-1), 0.0).transpose(1, 2)
        if cfg.flow_n_flows % 2 == 1:  # (the tap is in the device's channel order: reversed after an odd number of flips)
            zt = torch.flip(zt, [1])
        assert torch.equal(zt, z), "%s: the flow0 tap is not the forward's z" % c.name
    out = [compare(c, name, taps[name], segment_bars(c, name, taps, got=taps[name])) for name in segs]
    rec = {"case": c.name, "operand": c.operand, "B": c.B, "T": c.T, "forms": want, "forms_observed": seen,
           "forms_computed_only": ["nj", "nj_flow"] + (["wn: split_taps / split_channels share their kernel names"] if want["wn"] != "one_launch" else []),
           "kernels": sorted(names), "segments": out}
    return rec, z, fr
