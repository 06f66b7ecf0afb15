"""TEST INFRASTRUCTURE ONLY -- the generator restated LAYER BY LAYER, with the operand rounding of the HIP kernels.

``nsf_oracle.generator_forward`` is the reference's function; this module cuts it at the taps the library can hand out
(``har``, ``pre``, ``up<i>``, ``stage<i>``; csrc/nsf.hip:1361-1390) so that ONE layer's arithmetic can be compared at a time:

    pre(z, g)                -> the "pre" tap          conv_pre + cond, fp32                                   nsf.py:164-166
    up(i, prev_tap, har)     -> the "up<i>" tap        x / num_kernels, lrelu 0.1, ups[i], + noise_convs[i]    nsf.py:171-174,186
    stage(i, x0)             -> the "stage<i>" tap     (y0 + y1) + y2, the UN-divided sum of the resblocks      nsf.py:175-185
    post(last_stage_tap)     -> the waveform           x / num_kernels, lrelu 0.01, conv_post, tanh            nsf.py:186-189

Tensors are channel-first [B, C, L] as ``debug_tap`` returns them.  ``arith`` = "f64" / "f32" is the dtype everything is evaluated in;
``operand`` = "fp16" / "bf16" / None rounds (to nearest even) where the kernels round and NOWHERE else; None is the reference's function.

Where the kernels round (file:line of csrc/, OpT = the operand type, to_op = mfma_conv.hpp: to_op: RNE, fp16 saturates at 65504):

  weights      every conv that runs on the MFMA path has its weights packed as OpT once, at handle creation: conv_pre, ups, resblock convs
               (conv_pack.hpp build_conv, called from nsf.hip:128,190,227), the noise conv where it runs as an MFMA conv (nsf.hip:151, "mfma"
               route) or as one extra k-step of k_ups (nsf.hip:163, "k1" route).  Biases, cond, conv_post and the noise conv of the "valu"
               route (the last stage's 1-tap conv, or a stride the two MFMA forms do not take; nsf.hip:144-145) stay fp32.
  conv_pre     z is rounded while it is staged, to_op(z) (conv_kernels.hpp: stage_tile, IN_F32_CF); fp32 accumulation, + bias + cond in fp32
               (conv_kernels.hpp: conv_mfma_body, epilogue).  The "pre" tap is that fp32 sum (OUT_F32); a real forward stores to_op(lrelu(sum, 0.1)) instead
               (OUT_ACT, nsf.hip:950-959, conv_kernels.hpp: conv_mfma_body, OUT_ACT store) -- the very value k_ups computes from the fp32 sum (next line), so ``up(0, pre)`` is
               what the real run computes.
  ups input    to_op(lrelu(div3_exact((a + b) + c), 0.1)) (ups_kernels.hpp: k_ups, convert_store): the three streams are summed in fp32 in that order (as the
               stage tap sums them, post_kernels.hpp: k_sum3h, k_sum3), div3_exact is the IEEE quotient bit for bit (exact_fp.hpp:31-42).
  noise conv   "mfma" route (stride % 8 == 0, stride <= 64): to_op(har) (conv_kernels.hpp: stage_tile, IN_HAR) x OpT weights, fp32 sum + fp32 bias -> NZ, added in
               k_ups' epilogue in fp32 (ups_kernels.hpp: k_ups, addend in the epilogue).  "k1" route (2..16 taps, even stride): to_op(har) (ups_kernels.hpp: k_ups, har16 staging) x
               OpT weights, one extra MFMA k-step on the transposed conv's accumulator (ups_kernels.hpp: k_ups, nz_k1 k-step).  "valu" route: fp32 har x fp32
               weights (ups_kernels.hpp: k_ups, VALU noise loop of the epilogue).  (k_noise_add, conv_kernels.hpp, belongs to the fp32 path alone: nothing is rounded.)
  X0           written as fp32, or -- ``StagePlan.x0_half`` (nsf.hip:845-897) -- as FP16 whatever OpT is (mfma_conv.hpp: pack4_h; ups_kernels.hpp: k_ups, X0 stores):
               k_rb_full's stages under Y_F16 and X0_F16, the streaming kernel's unless X0_F16_NOSTREAM / RS_KL != 2 / RS_SMALL = 0
               (rb_stream.hip:258-261).  The SPLIT and PAIR paths keep fp32.  The "up<i>" tap is X0 as stored (widened).
  resblock     conv1's input to_op(lrelu(x, 0.1)) (SPLIT conv_kernels.hpp: stage_tile, row-major batch; PAIR rb_pair_kernels.hpp: k_rb_pair, step 1; FULL / STREAM mfma_conv.hpp: pack4_lrelu), the H tile
               between conv1 and conv2 to_op(lrelu(conv1 + b1, 0.1)) (SPLIT conv_kernels.hpp: conv_mfma_body / conv_ks_body, OUT_ACT store; fused kernels mfma_conv.hpp: publish_operand), and
               x <- conv2 + b2 + x with x the fp32 residual stream (it starts as X0 as stored and is never rounded inside a resblock).
  Y streams    a resblock's output is written fp32, or -- ``StagePlan.stage_half`` = option Y_F16 on the FULL and STREAM paths -- as FP16 whatever
               OpT is (pack4_h: rb_full_kernels.hpp: k_rb_full, fp16 stores; rb_stream_kernels.hpp:499,555).  SPLIT and PAIR write fp32.
  conv_post    nothing is rounded: (a + b) + c, div3_exact, lrelu 0.01, an fp32 fmaf chain over (tap, channel), tanhf
               (post_kernels.hpp: k_post, staging and tap loop; k_post_dma, convert pass and tap loop).

``variant=`` names a WRONG layer (tests/test_cpu_nsf_layers.py: the bars must reject each); ``perturb=`` a liberty the kernels may take
against the fp32 evaluation (``reorder``: summation order of the K loop; ``tanh``: tanhf by a few ulp; ``fma``: the one multiply-add of the MFMA layers'
fp32 epilogues that a compiler may contract, the last stage's VALU noise conv -- every other epilogue step is an addition of rounded terms;
tests/nsf_cases.py derives the bars' factors from them).  conv_post's fp32 evaluation IS the kernels' fmaf chain, in their order: nothing is left
to perturb there but tanhf.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from .nsf_oracle import GenConfig, get_padding, har_source  # noqa: F401  (har_source: the "har" layer is nsf_oracle's)

TILE_ROW_PERIOD = 128  # variant "tile_row": one output row in every 128 (the SPLIT / PAIR kernels' conv tile, rb_pair_kernels.hpp RB_ROWS)


def dtype_of(arith: str):
    return {"f64": torch.float64, "f32": torch.float32}[arith]


def round_h(x: torch.Tensor) -> torch.Tensor:
    """fp16 RNE with saturation (to_op<_Float16> / sat_h).  float64 goes through numpy: its double -> half conversion rounds once."""
    x = x.clamp(-65504.0, 65504.0)
    if x.dtype == torch.float64:
        return torch.from_numpy(x.numpy().astype(np.float16).astype(np.float64))
    return x.to(torch.float16).to(x.dtype)


def round_bf(x: torch.Tensor) -> torch.Tensor:
    """bf16 RNE (to_op<__bf16>).  float64 is rounded once, on its own mantissa (8 significant bits; activations are far from bf16's range limits)."""
    if x.dtype == torch.float64:
        m, e = torch.frexp(x)
        return torch.ldexp(torch.round(m * 256.0) / 256.0, e)  # torch.round: halves to even
    return x.to(torch.bfloat16).to(x.dtype)


def rounder(operand: Optional[str]):
    if operand is None:
        return lambda x: x
    return {"fp16": round_h, "bf16": round_bf}[operand]


def lrelu(x: torch.Tensor, slope: float) -> torch.Tensor:
    """v > 0 ? v : v * slope, the slope being the float32 constant the kernels multiply by (mfma_conv.hpp: lrelu, lrelu_op)"""
    return torch.where(x > 0, x, x * float(np.float32(slope)))


def noise_route(cfg: GenConfig, i: int) -> Optional[str]:
    """How noise_convs[i] runs on the MFMA path (build_stage, nsf.hip:132-170): "mfma", "k1", "valu"; None for a no-f0 generator"""
    if not cfg.use_f0:
        return None
    if i + 1 == len(cfg.upsample_rates):
        return "valu"
    s = math.prod(cfg.upsample_rates[i + 1:])
    if s % 8 == 0 and s <= 64:
        return "mfma"
    if 2 <= 2 * s <= 16 and s % 2 == 0:
        return "k1"
    return "valu"


def _ulps(rng, shape, n, dt):
    return torch.from_numpy(1.0 + rng.integers(-n, n + 1, tuple(shape)) * 2.0 ** -23).to(dt)


def conv1d(x, w, b, dilation=1, padding=0, stride=1, perturb=None, rng=None):
    """F.conv1d; with ``perturb["reorder"]`` the K loop is summed tap by tap and 16 channels at a time (one MFMA k-step) in a permuted order"""
    if not (perturb and perturb.get("reorder")):
        return F.conv1d(x, w, b, stride=stride, dilation=dilation, padding=padding)
    B, C, L = x.shape
    k = w.shape[2]
    xp = F.pad(x, (padding, padding))
    Lo = (L + 2 * padding - dilation * (k - 1) - 1) // stride + 1
    acc = torch.zeros(B, w.shape[0], Lo, dtype=x.dtype)
    steps = [(t, c0) for t in range(k) for c0 in range(0, C, 16)]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # thousands of 16-deep products: a thread pool only gets in their way (and in another OpenMP runtime's, once one is loaded)
    try:
        for idx in rng.permutation(len(steps)):
            t, c0 = steps[idx]
            xs = xp[:, c0:c0 + 16, t * dilation: t * dilation + (Lo - 1) * stride + 1: stride]
            acc = acc + torch.matmul(w[:, c0:c0 + 16, t], xs)
    finally:
        torch.set_num_threads(threads)
    if b is not None:
        acc = acc + b[None, :, None]
    return acc


def conv_transpose1d(x, w, b, stride, padding, perturb=None, rng=None):
    if not (perturb and perturb.get("reorder")):
        return F.conv_transpose1d(x, w, b, stride=stride, padding=padding)
    B, C, L = x.shape
    k = w.shape[2]
    xu = torch.zeros(B, C, (L - 1) * stride + 1, dtype=x.dtype)  # the same sum as a plain conv over the zero-stuffed input
    xu[:, :, ::stride] = x
    return conv1d(xu, w.flip(2).transpose(0, 1).contiguous(), b, padding=k - 1 - padding, perturb=perturb, rng=rng)


class Layers:
    """The layers of one generator (``cfg``, fp32 weights ``w``) in one arithmetic.

    ``x0_half[i]`` / ``y_half[i]``: stage i's X0 / Y streams are stored as fp16 (module docstring; ignored when ``operand`` is None)."""

    def __init__(self, cfg: GenConfig, w: Dict[str, torch.Tensor], arith: str = "f64", operand: Optional[str] = "fp16",
                 x0_half=None, y_half=None, perturb: Optional[dict] = None):
        self.cfg, self.arith, self.operand = cfg, arith, operand
        self.dt = dtype_of(arith)
        self.rnd = rounder(operand)
        n = len(cfg.upsample_rates)
        self.x0_half = tuple(x0_half) if x0_half is not None else (False,) * n
        self.y_half = tuple(y_half) if y_half is not None else (False,) * n
        self.perturb = perturb or None
        self.rng = np.random.default_rng((perturb or {}).get("seed", 0))
        self.w = {k: v.detach().to(self.dt) for k, v in w.items()}
        self._wr: Dict[str, torch.Tensor] = {}

    def W(self, name):  # a conv's weights as the MFMA path holds them
        if name not in self._wr:
            self._wr[name] = self.rnd(self.w[name])
        return self._wr[name]

    def _t(self, x):
        return torch.as_tensor(x).detach().to(self.dt)

    # -- conv_pre + cond --------------------------------------------------------------------------
    def pre(self, z, g=None, variant=None):
        w = self.w
        y = conv1d(self.rnd(self._t(z)), self.W("conv_pre.weight"), None if variant == "no_bias" else w["conv_pre.bias"], padding=3,
                   perturb=self.perturb, rng=self.rng)
        if g is not None and self.cfg.gin_channels and variant != "no_cond":
            y = y + F.conv1d(self._t(g).reshape(y.shape[0], -1, 1), w["cond.weight"], w["cond.bias"])
        return y

    # -- x / nk, lrelu, ups[i], + noise_convs[i](har) ---------------------------------------------
    def up(self, i, prev, har=None, variant=None):
        cfg, w = self.cfg, self.w
        u, k = cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i]
        x = self._t(prev)
        if i > 0:
            if variant != "div_skipped":
                x = x / cfg.num_kernels
            if variant == "div_twice":
                x = x / cfg.num_kernels
        a = self.rnd(lrelu(x, 0.01 if variant == "slope001" else 0.1))
        pad = (k - u) // 2
        L = x.shape[-1] * u
        if variant == "tpad_off1":  # padding (k - u) // 2 - 1: every output one sample late
            y = conv_transpose1d(a, self.W(f"ups.{i}.weight"), w[f"ups.{i}.bias"], u, pad - 1, self.perturb, self.rng)[..., :L]
        else:
            y = conv_transpose1d(a, self.W(f"ups.{i}.weight"), None if variant == "no_bias" else w[f"ups.{i}.bias"], u, pad, self.perturb, self.rng)
        route = noise_route(cfg, i)
        if route is not None:
            h = self._t(har)
            wn, bn = w[f"noise_convs.{i}.weight"], w[f"noise_convs.{i}.bias"]
            if route != "valu":
                h, wn = self.rnd(h), self.W(f"noise_convs.{i}.weight")
            if i + 1 < len(cfg.upsample_rates):
                s = math.prod(cfg.upsample_rates[i + 1:])
                if variant == "npad_off1":
                    y = y + F.conv1d(h, wn, bn, stride=s, padding=s // 2 + 1)[..., :L]
                else:
                    y = y + F.conv1d(h, wn, bn, stride=s, padding=s // 2)
            elif (self.perturb or {}).get("fma") and self.arith == "f32":
                # bias + w * har with ONE rounding (the VALU route's product and the add behind it contracted; products of float32 are exact in float64)
                y = y + (wn.double().reshape(1, -1, 1) * h.double() + bn.double().reshape(1, -1, 1)).float()
            else:
                y = y + F.conv1d(h, wn, bn)
        if self.operand is not None and (self.x0_half[i] or variant == "x0_rounded"):
            y = round_h(y)
        return y

    # -- the resblocks of stage i: X0 -> (y0 + y1) + y2 -------------------------------------------
    def resblock(self, i, j, x0, variant=None):
        cfg, w = self.cfg, self.w
        n = i * cfg.num_kernels + j
        k, dils = cfg.resblock_kernel_sizes[j], cfg.resblock_dilation_sizes[j]
        x = self._t(x0)
        for m, d in enumerate(dils):
            w1, b1 = self.W(f"resblocks.{n}.convs1.{m}.weight"), w[f"resblocks.{n}.convs1.{m}.bias"]
            w2, b2 = self.W(f"resblocks.{n}.convs2.{m}.weight"), w[f"resblocks.{n}.convs2.{m}.bias"]
            # where the one-conv variants sit: the second dilation level of the first resblock (k = 3), "tap097" of the last (k = 11: 3 % of ONE OF ELEVEN taps)
            here = variant is not None and j == (cfg.num_kernels - 1 if variant == "tap097" else 0) and m == min(1, len(dils) - 1)
            if here and variant == "tap097":
                w1 = w1.clone()
                w1[:, :, -1] *= 0.97
            xt = self.rnd(lrelu(x, 0.1))
            p = get_padding(k, d)
            if here and variant == "pad_off1":  # the dilated conv reads one row too far left
                xt = conv1d(F.pad(xt, (1, 0))[..., :-1], w1, b1, dilation=d, padding=p, perturb=self.perturb, rng=self.rng)
            else:
                xt = conv1d(xt, w1, None if (here and variant == "no_bias") else b1, dilation=d, padding=p, perturb=self.perturb, rng=self.rng)
            if here and variant == "tile_row":
                xt = xt.clone()
                xt[:, :, TILE_ROW_PERIOD - 1::TILE_ROW_PERIOD] *= 1.1
            xt = self.rnd(lrelu(xt, 0.01 if (here and variant == "slope001") else 0.1))
            xt = conv1d(xt, w2, b2, padding=get_padding(k, 1), perturb=self.perturb, rng=self.rng)
            x = xt + (self.rnd(x) if (here and variant == "res_from_operand") else x)
        if self.operand is not None and self.y_half[i]:
            x = round_h(x)
        return x

    def stage(self, i, x0, variant=None):
        xs = None
        for j in range(self.cfg.num_kernels):
            r = self.resblock(i, j, x0, variant)
            xs = r if xs is None else xs + r
        return xs

    # -- x / nk, lrelu 0.01, conv_post, tanh ------------------------------------------------------
    def post(self, s, variant=None):
        cfg = self.cfg
        x = self._t(s)
        if variant != "div_skipped":
            x = x / cfg.num_kernels
        x = lrelu(x, 0.1 if variant == "slope01" else 0.01)
        wp = self.w["conv_post.weight"]
        p = self.perturb or {}
        if self.operand is not None and self.arith == "f32":
            # both kernels' arithmetic, step for step: ONE fmaf chain per output, taps outer, channels inner (post_kernels.hpp: k_post / k_post_dma, tap loop).  The products
            # are exact in float64, so rounding the float64 sum to float32 is the fused multiply-add's single rounding.
            xp = F.pad(x, (3, 3)).double()
            L = x.shape[-1]
            acc = torch.zeros(x.shape[0], L, dtype=torch.float32)
            for j in range(7):
                for c in range(x.shape[1]):
                    acc = (acc.double() + xp[:, c, j:j + L] * float(wp[0, c, j])).float()
            y = acc.unsqueeze(1)
        else:
            y = conv1d(x, wp, None, padding=3)
        y = torch.tanh(y)
        if p.get("tanh"):
            y = y * _ulps(self.rng, y.shape, int(p["tanh"]), self.dt)
        return y

    # -- the layers composed ----------------------------------------------------------------------
    def forward(self, z, g=None, har=None, taps: Optional[dict] = None, variants: Optional[dict] = None):
        """The whole generator from ``z`` and the excitation ``har`` ([B, 1, T * upp] or None): each layer fed the previous layer's output.
        ``variants`` = {layer name: variant}."""
        variants = variants or {}
        x = self.pre(z, g, variants.get("pre"))
        if taps is not None:
            taps["pre"] = x
        for i in range(len(self.cfg.upsample_rates)):
            x = self.up(i, x, har, variants.get(f"up{i}"))
            if taps is not None:
                taps[f"up{i}"] = x
            x = self.stage(i, x, variants.get(f"stage{i}"))
            if taps is not None:
                taps[f"stage{i}"] = x
        return self.post(x, variants.get("post"))


def layer_names(cfg: GenConfig):
    n = len(cfg.upsample_rates)
    return ["pre"] + [nm for i in range(n) for nm in (f"up{i}", f"stage{i}")] + ["post"]


def apply_layer(ly: Layers, name: str, inputs: dict, variant=None):
    """Layer ``name`` of ``ly`` applied to the taps in ``inputs`` ({"z", "g", "har", "pre", "up<i>", "stage<i>"}: whatever it consumes)."""
    if name == "pre":
        return ly.pre(inputs["z"], inputs.get("g"), variant)
    if name == "post":
        return ly.post(inputs["stage%d" % (len(ly.cfg.upsample_rates) - 1)], variant)
    i = int(name[-1])
    if name.startswith("up"):
        return ly.up(i, inputs["pre"] if i == 0 else inputs[f"stage{i - 1}"], inputs.get("har"), variant)
    return ly.stage(i, inputs[f"up{i}"], variant)
