"""Shared pieces of the HuBERT encoder-layer tests (tests/test_cpu_hubert_enc.py, tests/test_gpu_hubert_enc.py) and of
tools/hubert_enc_parity.py: the seeded cases, an fp64 restatement of one post-norm layer with the kernels' fp16 rounding points, the
fairseq-shaped stand-in model, and the bars csrc/hubert_enc.hip is held to.

The oracle (``layer``) rounds to fp16 where the kernels do -- the weights; the input when it arrives as fp16; the input as the QKV GEMM's
operand (the same numbers then; when the input is fp32 the residual keeps the unrounded value); q / k / v; the probabilities; the attention
output fed to the out-projection; the stream as FFN-1's operand (the residual keeps fp32); the GELU output; the layer output when the dtype is
fp16 -- and nowhere else.  The probabilities are rounded as the kernel rounds them: keys come in tiles of KT with a running maximum, so a
probability is exp(score - the maximum of the keys SO FAR), rounded, and rescaled later; the row sum takes them unrounded.  With the rounding
off all of this is the plain softmax, and the oracle is transformers' ``HubertEncoderLayer`` in fp64 to ~1e-12 (tests/test_cpu_hubert_enc.py),
key mask included.  Weights come from numpy's ``default_rng(seed)`` at torch's default scales (Linear: uniform within 1 / sqrt(fan_in), weight
and bias), LayerNorm affine away from (1, 0).

The bars are derived on the CPU, not measured on the kernel.  ``floor`` = the oracle evaluated in float32 against its float64 evaluation:
fp32 rounding that now and then flips the fp16 rounding of a stored operand.  The kernel differs from that fp32 evaluation in four nameable
ways, each of which the oracle imitates (``perturb=``): the K-loop summation order (64-wide chunks summed in a permuted order), erff (+-4 ulp
at random), expf (+-2 ulp at random on every probability and every rescaling factor of the online softmax), and the LayerNorm's 1 / sqrt
(+-1 ulp).  With all four at once, over every case of ``TABLE`` and two perturbation seeds (tests/test_cpu_hubert_enc.py prints them), the error
against the fp64 oracle moved to at most 1.72x the floor's RMS and 2.00x the floor's max-abs (one fp16 ulp of the output became two); twice
the worse is 4.0, already a multiple of one half: the factor.  One case has a floor of exactly 0, the all-zero fp16 input; there the perturbed
evaluation sits 0.11 ulp16(max |y|) / sqrt(n) RMS and 0.03 ulp16(max |y|) max-abs away (ulp16(v) = the spacing of fp16 at v; n elements):
a few flips of small elements.  A flip can strike the largest element as well as a small one, so the additive term is not twice those figures
but ONE whole flip of one element more than the floor saw:

    bar_rms = 4.0 * floor_rms + ulp16(max |y|) / sqrt(n)        bar_max = 4.0 * floor_max + ulp16(max |y|)

The GELU output alone is held to account too (``bars_ffn1``, same formula, on ``STAGE_CASES``; the kernels leave it in the caller's workspace):
the tanh approximation differs from the exact GELU by a fraction of an fp16 ulp per element, plain to see against a floor of rare flips there
(1.6x the bar), while FFN-2, the LayerNorm and the output's own rounding bury it in the layer's output.  The perturbed evaluations moved to at
most 1.03x the floor there.  tests/test_cpu_hubert_enc.py asserts that the perturbed evaluations stay within HALF of each bar and that the
named wrong variants (q scaled before the bias, tanh-GELU, pre-norm order, key mask ignored, softmax without max subtraction, unbiased
variance) stand clear of the bars (beyond 1.25x one of them), so widening a bar fails there.
"""
import collections
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KT = 64        # keys per tile of k_he_attn (csrc/hubert_enc_kernels.hpp KT; also its queries per block)
MT = 32        # rows per block of k_he_gemm_ln (MT)
MT_PLAIN = 64  # rows per block of k_he_gemm (GM)
HEAD = 64
EPS = 1e-5
FACTOR = 4.0
# "odd": d = 64 x an odd number, where k_he_gemm_ln runs on 4 waves (8 at d = 128, 16 at d = 768)
CONFIGS = {"small": dict(d=128, heads=2, ffn=256), "base": dict(d=768, heads=12, ffn=3072), "odd": dict(d=192, heads=3, ffn=320)}
ITEM_GAINS = (1.0, 0.125, 3.0)  # item b of a batch is scaled by ITEM_GAINS[b]

# lens: the unmasked keys of every item (None: no mask); kind: "noise" or "zero"
Case = collections.namedtuple("Case", "cfg B T seed half wgain kind lens", defaults=(True, 1.0, "noise", None))

_TS = (1, 2, 3, MT - 1, MT, MT + 1, KT - 1, KT, KT + 1, 3 * KT + 5, 137)
SHAPES = tuple(Case("small", 1, T, 10 + i, bool(i % 2)) for i, T in enumerate(_TS))
BASE = (Case("base", 1, 137, 30), Case("base", 1, KT + 1, 31, False), Case("base", 1, 3 * KT + 5, 32))
# a mask that leaves ONE key (item 1 of the first), a mask ending exactly on a key-tile edge (item 1 of the second)
BATCHES = (Case("small", 2, 70, 40, True, 1.0, "noise", (70, 1)), Case("small", 3, 130, 41, False, 1.0, "noise", (130, KT, 37)),
           Case("base", 2, 70, 42, True, 1.0, "noise", (70, 33)), Case("small", 3, 33, 43, True), Case("odd", 2, 37, 44, True, 1.0, "noise", (37, 20)),
           Case("odd", 1, 70, 45, False))
SPECIAL = (Case("small", 1, 137, 50, True, 4.0), Case("small", 1, 137, 51, False, 4.0), Case("base", 1, 70, 52, True, 4.0),
           Case("small", 1, 33, 53, True, 1.0, "zero"), Case("small", 2, 33, 54, False, 1.0, "zero"))
TABLE = SHAPES + BASE + BATCHES + SPECIAL
LARGE_SCORES = SPECIAL[0]


def case_id(c):
    return "%s-B%d-T%d-seed%d-%s%s%s%s" % (c.cfg, c.B, c.T, c.seed, "f16" if c.half else "f32", "" if c.wgain == 1.0 else "-w%g" % c.wgain,
                                           "" if c.kind == "noise" else "-" + c.kind, "" if c.lens is None else "-mask" + "_".join(map(str, c.lens)))


_LINEAR = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "fc1", "fc2")
_NORMS = ("self_attn_layer_norm", "final_layer_norm")


@functools.lru_cache(maxsize=None)
def weights(cfg, seed, wgain=1.0, n_layers=1):
    """-> a tuple of ``n_layers`` dicts {fairseq's tensor name: float32 array}: torch's default Linear scale (the weights times ``wgain``), an
    affine LayerNorm away from its (1, 0) default"""
    g = CONFIGS[cfg]
    d, ffn = g["d"], g["ffn"]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_layers):
        w = {}
        for name in _LINEAR:
            fo, fi = {"fc1": (ffn, d), "fc2": (d, ffn)}.get(name, (d, d))
            b = 1.0 / np.sqrt(fi)
            w[name + ".weight"] = (wgain * rng.uniform(-b, b, (fo, fi))).astype(np.float32)
            w[name + ".bias"] = rng.uniform(-b, b, fo).astype(np.float32)
        for name in _NORMS:
            w[name + ".weight"] = (1.0 + 0.25 * rng.standard_normal(d)).astype(np.float32)
            w[name + ".bias"] = (0.25 * rng.standard_normal(d)).astype(np.float32)
        for a in w.values():
            a.setflags(write=False)
        out.append(w)
    return tuple(out)


def state_dict(w):
    """One layer's weights under fairseq's names as torch tensors (``HubertEncoderHIP.from_state_dicts``)."""
    return {k: torch.from_numpy(a.copy()) for k, a in w.items()}


def hf_state_dict(w):
    """One layer's weights under the names of transformers' ``HubertEncoderLayer``."""
    ren = {"self_attn.": "attention.", "self_attn_layer_norm.": "layer_norm.", "fc1.": "feed_forward.intermediate_dense.",
           "fc2.": "feed_forward.output_dense."}
    out = {}
    for k, a in w.items():
        for old in sorted(ren, key=len, reverse=True):
            if k.startswith(old):
                k = ren[old] + k[len(old):]
                break
        out[k] = torch.from_numpy(a.copy())
    return out


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> x [B, T, d] float32 (already on the fp16 grid when ``c.half``)"""
    rng = np.random.default_rng(1000 + c.seed)
    x = rng.standard_normal((c.B, c.T, CONFIGS[c.cfg]["d"]))
    if c.kind == "zero":
        x = 0.0 * x
    x = (x * np.asarray(ITEM_GAINS[:c.B])[:, None, None]).astype(np.float32)
    if c.half:
        x = x.astype(np.float16).astype(np.float32)
    x.setflags(write=False)
    return x


def key_mask(c):
    """-> bool [B, T], True = a padded key; None without a mask"""
    if c.lens is None:
        return None
    return np.arange(c.T)[None, :] >= np.asarray(c.lens)[:, None]


def r16(a):
    return a.astype(np.float16).astype(a.dtype)


def _erf(a):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def _ulps(rng, shape, n, dtype):
    """1 + a random whole number of float32 ulps in [-n, n]"""
    return (1.0 + rng.integers(-n, n + 1, shape) * 2.0 ** -23).astype(dtype)


def _linear(a, w, b, perturb, rng):
    """a [.., K] @ w[N, K]' + b; with the summation-order perturbation: 64-wide chunks summed one after the other in a permuted order"""
    wt = np.ascontiguousarray(w.T)
    if not (perturb and perturb.get("reorder")):
        return a @ wt + b
    acc = np.zeros(a.shape[:-1] + (wt.shape[1],), dtype=a.dtype)
    for k0 in rng.permutation(np.arange(0, a.shape[-1], 64)):
        acc = acc + a[..., k0:k0 + 64] @ wt[k0:k0 + 64]
    return acc + b


def gelu(v, variant=None, perturb=None, rng=None):
    if variant == "tanh_gelu":
        return 0.5 * v * (1.0 + np.tanh(v.dtype.type(np.sqrt(2.0 / np.pi)) * (v + v.dtype.type(0.044715) * v * v * v)))
    e = _erf(v * v.dtype.type(0.7071067811865476))
    if perturb and perturb.get("erf"):
        e = e * _ulps(rng, e.shape, perturb["erf"], v.dtype)
    return v.dtype.type(0.5) * v * (v.dtype.type(1.0) + e)


def _layer_norm(y, g, b, variant, perturb, rng):
    dt = y.dtype.type
    mean = y.mean(axis=-1, keepdims=True)
    var = y.var(axis=-1, keepdims=True, ddof=1 if variant == "unbiased_var" else 0)
    rstd = 1.0 / np.sqrt(var + dt(EPS))
    if perturb and perturb.get("rsqrt"):
        rstd = rstd * _ulps(rng, rstd.shape, perturb["rsqrt"], y.dtype)
    return (y - mean) * rstd.astype(y.dtype) * g + b


def _softmax_pv(s, v, rnd, variant, perturb, rng):
    """s [B, H, T, T] (masked keys -inf), v [B, H, T, 64] -> sum_k rnd(p) v / sum_k p in the kernel's order: keys in tiles of KT, a running
    maximum, sum and output rescaled from tile to tile -- so a probability is rounded to fp16 relative to the maximum of the keys SO FAR, as
    the kernel rounds it.  Without rounding this is the plain softmax.  ``perturb["expf"]``: every exponential +- that many ulps."""
    dt = s.dtype
    ul = (lambda shape: _ulps(rng, shape, perturb["expf"], dt)) if perturb and perturb.get("expf") else (lambda shape: dt.type(1.0))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if variant == "no_max":
            p = np.exp(s).astype(dt)
            return (rnd(p) @ v) / p.sum(axis=-1, keepdims=True)
        T = s.shape[-1]
        m = np.full(s.shape[:-1] + (1,), -np.inf, dtype=dt)
        l = np.zeros_like(m)
        o = np.zeros(s.shape[:-1] + (v.shape[-1],), dtype=dt)
        for k0 in range(0, T, KT):
            st = s[..., k0:k0 + KT]
            m_new = np.maximum(m, st.max(axis=-1, keepdims=True))
            ref = np.where(np.isfinite(m_new), m_new, 0.0).astype(dt)
            alpha = (np.exp(m - ref) * ul(m.shape)).astype(dt)
            p = (np.exp(st - ref) * ul(st.shape)).astype(dt)
            l = l * alpha + p.sum(axis=-1, keepdims=True)
            o = o * alpha + rnd(p) @ v[..., k0:k0 + KT, :]
            m = m_new
        return o / l


def layer(w, x, mask=None, half=True, arith="f64", variant=None, round_operands=True, perturb=None, stage=None):
    """One post-norm layer.  ``x`` [B, T, d], ``mask`` bool [B, T] (True = a padded key) or None; -> [B, T, d] in ``arith``'s dtype.
    ``round_operands=False``: no fp16 rounding anywhere (the function transformers' module computes).  ``variant``: a named WRONG layer.
    ``perturb``: {"reorder": bool, "erf": ulps, "expf": ulps, "rsqrt": ulps, "seed": int}, the kernels' liberties (module docstring).
    ``stage="ffn1"``: -> the GELU output [B, T, ffn] as FFN-2 reads it, instead of the layer's."""
    dt = np.float64 if arith == "f64" else np.float32
    rng = np.random.default_rng((perturb or {}).get("seed", 0))
    rnd = r16 if round_operands else (lambda a: a)
    W = lambda n: rnd(w[n + ".weight"].astype(dt))
    b_ = lambda n: w[n + ".bias"].astype(dt)
    x = np.asarray(x, dtype=dt)
    if half:
        x = rnd(x)
    B, T, d = x.shape
    H = d // HEAD
    scale = dt(HEAD ** -0.5)

    kept = {}

    def attn(a):
        a = rnd(a)
        if variant == "scale_before_bias":
            q = _linear(a, W("self_attn.q_proj"), 0.0, perturb, rng) * scale + b_("self_attn.q_proj")
        else:
            q = _linear(a, W("self_attn.q_proj"), b_("self_attn.q_proj"), perturb, rng) * scale
        k = _linear(a, W("self_attn.k_proj"), b_("self_attn.k_proj"), perturb, rng)
        v = _linear(a, W("self_attn.v_proj"), b_("self_attn.v_proj"), perturb, rng)
        q, k, v = [rnd(t.astype(dt)).reshape(B, T, H, HEAD).transpose(0, 2, 1, 3) for t in (q, k, v)]
        s = (q @ k.transpose(0, 1, 3, 2)).astype(dt)
        if mask is not None and variant != "mask_ignored":
            s = np.where(np.asarray(mask)[:, None, None, :], dt(-np.inf), s)
        o = _softmax_pv(s, v, rnd, variant, perturb, rng).astype(dt)
        o = rnd(o.transpose(0, 2, 1, 3).reshape(B, T, d))
        return _linear(o, W("self_attn.out_proj"), b_("self_attn.out_proj"), perturb, rng).astype(dt)

    def ffn(a):
        h = rnd(gelu(_linear(rnd(a), W("fc1"), b_("fc1"), perturb, rng).astype(dt), variant, perturb, rng).astype(dt))
        kept["ffn1"] = h
        return _linear(h, W("fc2"), b_("fc2"), perturb, rng).astype(dt)

    ln1 = lambda y: _layer_norm(y, w["self_attn_layer_norm.weight"].astype(dt), w["self_attn_layer_norm.bias"].astype(dt), variant, perturb, rng).astype(dt)
    ln2 = lambda y: _layer_norm(y, w["final_layer_norm.weight"].astype(dt), w["final_layer_norm.bias"].astype(dt), variant, perturb, rng).astype(dt)
    with np.errstate(over="ignore", invalid="ignore"):
        if variant == "pre_norm":
            x1 = x + attn(ln1(x))
            y = x1 + ffn(ln2(x1))
        else:
            x1 = ln1(x + attn(x))
            y = ln2(x1 + ffn(x1))
    if stage is not None:
        return kept[stage]
    return rnd(y) if half else y


def chain(ws, x, mask=None, half=True, arith="f64", **kw):
    """Several layers, each rounded at its boundary like a single-layer call."""
    for w in ws:
        x = layer(w, x, mask, half, arith, **kw)
    return x


def ulp16(v):
    """the spacing of fp16 at |v| (normal range)"""
    v = max(abs(float(v)), 2.0 ** -14)
    return 2.0 ** (np.floor(np.log2(v)) - 10)


def err(got, want):
    """-> (RMS, max-abs) of got - want, in float64; a non-finite difference is infinitely far"""
    e = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    if not e.size:
        return 0.0, 0.0
    if not np.isfinite(e).all():
        return float("inf"), float("inf")
    return float(np.sqrt(np.mean(e * e))), float(np.abs(e).max())


def bars_of(y32, y64):
    floor_rms, floor_max = err(y32, y64)
    y = np.asarray(y64, dtype=np.float64)
    one = ulp16(np.abs(y).max())
    return {"floor_rms": floor_rms, "floor_max": floor_max, "bar_rms": FACTOR * floor_rms + one / np.sqrt(y.size), "bar_max": FACTOR * floor_max + one}


def valid_rows(c):
    """bool [B, T]: the rows a test compares -- every row (a padded QUERY row is computed like any other, and the oracle computes it too)."""
    return np.ones((c.B, c.T), dtype=bool)


@functools.lru_cache(maxsize=None)
def bars(c, n_layers=1):
    """The oracle of a case (``y`` [B, T, d] float64; computed once, never changed) and the bars against it."""
    ws, x, m = weights(c.cfg, c.seed, c.wgain, n_layers), inputs(c), key_mask(c)
    y64 = chain(ws, x, m, c.half)
    y32 = chain(ws, x, m, c.half, arith="f32")
    y64.setflags(write=False)
    return {"y": y64, **bars_of(y32, y64)}


STAGE_CASES = (SHAPES[10], BASE[0])  # the cases whose GELU output (FFN-2's operand, left in the caller's workspace) is compared on its own


@functools.lru_cache(maxsize=None)
def bars_ffn1(c):
    """As ``bars`` for the GELU output alone (``y`` [B, T, ffn]): where a wrong GELU shows before FFN-2, the LayerNorm and the output's own
    rounding bury it."""
    w, x, m = weights(c.cfg, c.seed, c.wgain)[0], inputs(c), key_mask(c)
    y64 = layer(w, x, m, c.half, stage="ffn1")
    y32 = layer(w, x, m, c.half, arith="f32", stage="ffn1")
    y64.setflags(write=False)
    return {"y": y64, **bars_of(y32, y64)}


def ffn1_offset(c):
    """Byte offset of the GELU output, fp16 [B T, ffn], in the caller's workspace after a forward (include/rvcmi.h, rvcmi_hubert_enc_forward)."""
    g = CONFIGS[c.cfg]
    a = lambda n: (n + 255) & ~255
    M, d = c.B * c.T, g["d"]
    return a(3 * M * d * 2) + a(M * d * 2) + a(M * d * 4) + a(M * d * 2)


PERTURB = {"reorder": True, "erf": 4, "expf": 2, "rsqrt": 1}


def hf_layer(w, cfg, dtype=torch.float64):
    """transformers' own encoder layer holding ``w`` (the independent definition of the layer)"""
    from transformers import HubertConfig
    from transformers.models.hubert.modeling_hubert import HubertEncoderLayer

    m = HubertEncoderLayer(hf_config(cfg, 1)).eval()
    m.load_state_dict(hf_state_dict(w))
    return m.to(dtype)


def hf_config(cfg, n_layers):
    from transformers import HubertConfig

    g = CONFIGS[cfg]
    return HubertConfig(hidden_size=g["d"], num_attention_heads=g["heads"], intermediate_size=g["ffn"], num_hidden_layers=n_layers, hidden_act="gelu",
                        hidden_dropout=0.0, attention_dropout=0.0, activation_dropout=0.0, layerdrop=0.0, layer_norm_eps=EPS, do_stable_layer_norm=False,
                        attn_implementation="eager")


# ---- a fairseq-shaped stand-in: the attribute names, the T x B x C convention and the encoder loop of the reference's HuBERT ----
class FsAttention(torch.nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        self.num_heads, self.head_dim, self.scaling = heads, d // heads, (d // heads) ** -0.5
        self.q_proj, self.k_proj, self.v_proj, self.out_proj = (torch.nn.Linear(d, d) for _ in range(4))

    def forward(self, query, key, value, key_padding_mask=None, need_weights=False, attn_mask=None):
        T, B, C = query.shape
        sp = lambda t: t.contiguous().view(T, B * self.num_heads, self.head_dim).transpose(0, 1)
        q, k, v = sp(self.q_proj(query) * self.scaling), sp(self.k_proj(key)), sp(self.v_proj(value))
        s = torch.bmm(q, k.transpose(1, 2))
        if attn_mask is not None:
            s = s + attn_mask
        if key_padding_mask is not None:
            s = s.view(B, self.num_heads, T, T).masked_fill(key_padding_mask[:, None, None, :].to(torch.bool), float("-inf")).view(B * self.num_heads, T, T)
        p = torch.softmax(s, dim=-1, dtype=torch.float32 if s.dtype == torch.float16 else None).to(s.dtype)  # (fairseq: softmax in fp32)
        o = torch.bmm(p, v).transpose(0, 1).contiguous().view(T, B, C)
        return self.out_proj(o), (p.view(B, self.num_heads, T, T).mean(1) if need_weights else None)


class FsLayer(torch.nn.Module):
    """fairseq's TransformerSentenceEncoderLayer by its attribute names and call convention."""

    def __init__(self, d, heads, ffn, layer_norm_first=False, activation=torch.nn.functional.gelu):
        super().__init__()
        self.layer_norm_first, self.activation_fn = layer_norm_first, activation
        self.self_attn = FsAttention(d, heads)
        self.dropout1, self.dropout2, self.dropout3 = (torch.nn.Dropout(0.1) for _ in range(3))
        self.self_attn_layer_norm, self.final_layer_norm = torch.nn.LayerNorm(d, eps=EPS), torch.nn.LayerNorm(d, eps=EPS)
        self.fc1, self.fc2 = torch.nn.Linear(d, ffn), torch.nn.Linear(ffn, d)

    def forward(self, x, self_attn_mask=None, self_attn_padding_mask=None, need_weights=False, att_args=None):
        residual = x
        if self.layer_norm_first:
            x = self.self_attn_layer_norm(x)
            x, attn = self.self_attn(x, x, x, key_padding_mask=self_attn_padding_mask, attn_mask=self_attn_mask, need_weights=need_weights)
            x = residual + self.dropout1(x)
            residual = x
            x = self.fc2(self.dropout2(self.activation_fn(self.fc1(self.final_layer_norm(x)))))
            x = residual + self.dropout3(x)
        else:
            x, attn = self.self_attn(x, x, x, key_padding_mask=self_attn_padding_mask, attn_mask=self_attn_mask, need_weights=need_weights)
            x = self.self_attn_layer_norm(residual + self.dropout1(x))
            residual = x
            x = self.fc2(self.dropout2(self.activation_fn(self.fc1(x))))
            x = self.final_layer_norm(residual + self.dropout3(x))
        return x, (attn, None)


class FsEncoder(torch.nn.Module):
    def __init__(self, d, heads, ffn, n_layers):
        super().__init__()
        self.layers = torch.nn.ModuleList([FsLayer(d, heads, ffn) for _ in range(n_layers)])

    def forward(self, x, padding_mask=None):
        x = x.transpose(0, 1)  # B x T x C -> T x B x C
        for layer_ in self.layers:
            x, _ = layer_(x, self_attn_padding_mask=padding_mask, need_weights=False)
        return x.transpose(0, 1)


class FsModel(torch.nn.Module):
    """``model.encoder.layers`` where the reference's HuBERT has it; the layers are the whole model here."""

    def __init__(self, cfg, n_layers):
        super().__init__()
        g = CONFIGS[cfg]
        self.encoder = FsEncoder(g["d"], g["heads"], g["ffn"], n_layers)

    def forward(self, x, padding_mask=None):
        return self.encoder(x, padding_mask)


def fs_model(ws, cfg):
    m = FsModel(cfg, len(ws)).eval()
    for lyr, w in zip(m.encoder.layers, ws):
        lyr.load_state_dict(state_dict(w))
    return m
