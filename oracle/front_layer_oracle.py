"""TEST INFRASTRUCTURE ONLY -- the synthesizer front restated SEGMENT BY SEGMENT, with the operand rounding of the HIP kernels.

``front_oracle.infer_front`` is the reference's function; this module cuts it at the taps the library hands out (``emb``, ``attn<i>``, ``layer<i>``,
``z_p``, ``flow<f>``; csrc/front.hip:317,364-367,405-407,417,458-460) so that ONE segment's arithmetic can be compared at a time:

    emb(phone, pitch, lengths)             -> "emb"        emb_phone + emb_pitch, * sqrt(H), lrelu 0.1, mask            encoders.py:142-148
    attn(i, x, lengths)                    -> "attn<i>"    q / k / v, rel-pos attention, conv_o, + x, LayerNorm 1        attentions.py:74-146
    ffn(i, x, lengths)                     -> "layer<i>"   FFN, + x, LayerNorm 2                                          attentions.py:262-272
    z_p(x, lengths, noise, flow_head)      -> "z_p"        proj + the prior sample, rows [flow_head, T)                   synthesizers.py:182-183
    flow(f, zp, lengths, g, flow_head)     -> "flow<f>"    pre, the WN layers with cond_layer(g), post, coupling update   residuals.py:214-238
    out(zp, lengths, flow_head)            -> z            transpose + mask, logical channel order (k_fr_out)             synthesizers.py:192

Tensors are CHANNELS-LAST [B, T', 192] as ``FrontHIP.debug_tap`` returns them; ``out`` is channel-first [B, 192, T'] as ``forward`` returns it.
``arith`` = "f64" / "f32" is the dtype everything is evaluated in; ``operand`` = "fp16" / "bf16" / None rounds (to nearest even, dtype PRESERVED --
float64 is rounded once, not through float32) where the kernels round and NOWHERE else; None is the reference's function.

The flow taps are in the DEVICE's channel order.  The Flip in front of every coupling is folded into the packed weights (front.hip:606-639), so the
stream buffer never moves: coupling f runs after n_flows - f flips, and when that count is odd the buffer holds the logical tensor with its channel
axis reversed.  ``flow`` takes and returns that physical order (n_flows = 4: "flow3" and "flow1" are reversed, "z_p", "flow2" and "flow0" are not).

Where the kernels round (file:line of csrc/; OpT = the operand type; to_op = mfma_conv.hpp: to_op: RNE, fp16 saturates at +-65504):

  weights      every conv's weights are packed as OpT once, at handle creation (conv_pack.hpp build_conv, called from front.hip:532,546,551,585-593,
               603,615,623,628,637) -- emb_phone, conv_q/k/v/o, the FFN convs, proj, the flow's pre / in_layers / res_skip_layers / post.
  rel. keys    emb_rel_k is packed as OpT (front.hip:554-573).  emb_rel_v stays fp32 (front.hip:574).
  conv inputs  an fp32 input is rounded while it is staged, to_op(x) (fr_stage front_kernels.hpp:128; fr_stage_dyn :156): phone, the residual stream
               in front of q/k/v and of the FFN's conv_1, the last layer's x in front of proj, the flow stream in front of pre, the WN stream in
               front of every in_layer, the skip sum in front of post.  An OpT input (in_op = 1) is copied.
  q, k, v      FR_QKV: q = to_op((acc + b) / sqrtf(dk)), k = to_op(acc + b), v = to_op(acc + b)  (front_kernels.hpp:465,477,493).
  P            p = __expf(S - m_new) is cast to OpT BEFORE normalisation (front_kernels.hpp:882-884) while the row sum l accumulates the UNROUNDED p
               (:883,894).  m_new is the running max of ONE wave: wave w of four walks the 32-key tiles w, w + 4, ... (:905-923), rescales its
               (l, O) by __expf(m_run - m_new) in fp32 (:886-893); the four partial (m, l, O) are merged in fp32 (:938-948,966-970).
  rel. values  recomputed in fp32 at the end from the stored band scores: exp(Sb - M) / L times fp32 E_v (front_kernels.hpp:958,972).  Not rounded.
  attn output  to_op(acc) into the OpT buffer conv_o reads (front_kernels.hpp:975).
  FFN hidden   to_op(relu(acc + b1) * mask): FR_RELU_OP (front_kernels.hpp:506), the H tile of k_fr_ffn (:1091) and of k_fr_ffn_part (:1222).
  WN gate      to_op(tanh(a_t + b_t + gc_t) * sigmoid(a_s + b_s + gc_s)): k_fr_wn (front_kernels.hpp:699), FR_GATE (:370), k_fr_gate_ks (:596);
               b + gc is summed first, in fp32 (:350-353,550-553,670).

fp32 on the device, so never rounded here: biases, the pitch embedding (front.hip:533), LayerNorm (front_kernels.hpp:263-311,1109-1160,1257-1292; eps 1e-5
inside sqrtf), masks, the residual added in front of every LayerNorm (the UNMASKED fp32 stream), the flow / WN / skip streams, k_cond (nsf_source_kernels.hpp: k_cond),
the prior sample (expf, the constant 0.66666f; front_kernels.hpp:334-336), the coupling update (:512-513) and k_fr_out (:1295-1314).

Masks, as the kernels apply them: "emb" is masked; the q/k/v conv and conv_o are not (padding keys score -1e4, :869); the FFN's input and hidden rows
are (:1058,1088), conv_2's result is before the residual add (:1115-1121); LayerNorm outputs are NOT, so rows at or beyond the length of "attn<i>" /
"layer<i>" are arbitrary but finite and feed nothing below the length.  proj reads x * mask (front.hip:412); "z_p" and "flow<f>" are exactly 0 there.

``variants`` = {segment name: variant} names a WRONG segment (tests/test_cpu_front_layers.py: the bars must tell each apart, or say that they cannot);
``perturb`` = the liberties the kernels take against the plain evaluation (tests/front_layer_cases.py derives the bars' factors from them):
  ``reorder``   every K loop -- the convs', and the attention's q.k, q.E_k and P.V products -- summed 16 deep (one MFMA k-step) at a time in a permuted order, the
                four waves' partial results merged in a permuted order; the FFN's conv_2 as four partial sums over the quarters
                of the hidden channels (k_fr_ffn_part + k_fr_ffn_ln) and the WN in_layer as per-tap partial sums (k_fr_gate_ks), each added in a
                permuted order;
  ``softmax``   the 32-key tiles dealt to the four waves in a permuted order (another running max at every rounding of p, another merge);
  ``exp``       = n: every exp of the float32 evaluation as the hardware computes it, exp2 of the float32-rounded x * log2(e), moved by up to n ulp.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from .front_oracle import FrontConfig
from .nsf_layer_oracle import dtype_of, rounder

LOG2E32 = float(np.float32(1.4426950408889634))
# A hidden activation whose exact value lies this close (in float32 ulps of the value) to the midpoint of two operand values is rounded either way by a correct
# float32 K loop, depending on its summation order: the comparison accepts both (Segments.ffn_head / ffn_tail; tests/front_layer_cases.tie_resolved).
TIE_FP32_ULPS = 2


def f32c(v: float) -> float:
    """The float32 constant a kernel holds for ``v`` (sqrtf(192), 0.66666f, 1e-5f ...), as a Python float."""
    return float(np.float32(v))


class Segments:
    """The segments of one front (``cfg``, fp32 weights ``w``) in one arithmetic."""

    def __init__(self, cfg: FrontConfig, w: Dict[str, torch.Tensor], arith: str = "f64", operand: Optional[str] = "fp16",
                 perturb: Optional[dict] = None, variants: Optional[dict] = None):
        self.cfg, self.arith, self.operand = cfg, arith, operand
        self.dt = dtype_of(arith)
        self.rnd = rounder(operand)
        self.perturb = perturb or {}
        self.variants = variants or {}
        self.rng = np.random.default_rng(self.perturb.get("seed", 0))
        self.w = {k: (v.detach().to(self.dt) if v.is_floating_point() else v) for k, v in w.items()}
        self._wr: Dict[str, torch.Tensor] = {}

    # ---- pieces ---------------------------------------------------------------------------------------------------------------------------
    def W(self, name):  # a conv's weights (or the relative-key table) as the MFMA path holds them
        if name not in self._wr:
            self._wr[name] = self.rnd(self.w[name])
        return self._wr[name]

    def _t(self, x):
        return torch.as_tensor(x).detach().to(self.dt)

    def _mask(self, lengths, T, t_off=0):
        if lengths is None:
            return torch.ones(1, T, 1, dtype=self.dt)
        return ((torch.arange(T) + t_off).unsqueeze(0) < torch.as_tensor(lengths).reshape(-1, 1)).to(self.dt).unsqueeze(-1)  # [B, T, 1]

    def exp(self, x):
        n = self.perturb.get("exp")
        if not n or self.arith != "f32":
            return torch.exp(x)
        y = torch.exp2(x * LOG2E32)  # float32 product, rounded once: the argument v_exp_f32 sees
        return y * torch.from_numpy(1.0 + self.rng.integers(-n, n + 1, tuple(y.shape)) * 2.0 ** -23).to(self.dt)

    def sigmoid(self, v):  # fast_sigmoid / fast_tanh, front_kernels.hpp:80-81
        return 1.0 / (1.0 + self.exp(-v))

    def tanh(self, v):
        return 2.0 * self.sigmoid(2.0 * v) - 1.0

    def mm(self, a, b):
        """a @ b; under perturb["reorder"] summed 16 deep (one MFMA k-step) at a time in a permuted order: the attention's q.k, q.E_k and P.V products"""
        if not self.perturb.get("reorder"):
            return a @ b
        y = None
        for k0 in self.rng.permutation(range(0, a.shape[-1], 16)):
            t = a[..., k0:k0 + 16] @ b[k0:k0 + 16]
            y = t if y is None else y + t
        return y

    def conv(self, x, weight, bias=None, groups: Optional[str] = None):
        """Channels-last conv1d with "same" zero padding (odd kernels): x [B, T, Cin], weight [Cout, Cin, k] -> [B, T, Cout]; + bias in the end, as the
        epilogues do.  ``groups`` = "taps" / "quarters": under perturb["reorder"] the partial sums a split kernel form keeps apart."""
        k = weight.shape[2]
        pad = (k - 1) // 2
        if not self.perturb.get("reorder"):
            y = F.conv1d(x.transpose(1, 2), weight, None, padding=pad).transpose(1, 2)
        else:
            B, T, C = x.shape
            xp = F.pad(x, (0, 0, pad, pad))
            steps = [(t, c0) for t in range(k) for c0 in range(0, C, 16)]
            key = (lambda s: 0) if groups is None else (lambda s: s[0]) if groups == "taps" else (lambda s: s[1] // (C // 4))
            parts = {}
            for idx in self.rng.permutation(len(steps)):
                t, c0 = steps[idx]
                term = torch.matmul(xp[:, t:t + T, c0:c0 + 16], weight[:, c0:c0 + 16, t].t())
                g = key(steps[idx])
                parts[g] = term if g not in parts else parts[g] + term
            order = list(parts)
            y = None
            for i in self.rng.permutation(len(order)):
                y = parts[order[i]] if y is None else y + parts[order[i]]
        return y if bias is None else y + bias

    def layer_norm(self, v, gamma, beta, eps=1e-5):
        # two passes, as the kernels: mean, then the centred second moment (front_kernels.hpp:285-301)
        mu = v.mean(dim=-1, keepdim=True)
        d = v - mu
        var = (d * d).mean(dim=-1, keepdim=True)
        return d * (1.0 / torch.sqrt(var + f32c(eps))) * gamma + beta

    # ---- emb ------------------------------------------------------------------------------------------------------------------------------
    def emb(self, phone, pitch, lengths):
        cfg, w = self.cfg, self.w
        v = self.variants.get("emb")
        x = self.conv(self.rnd(self._t(phone)), self.W("enc_p.emb_phone.weight").unsqueeze(-1), w["enc_p.emb_phone.bias"])
        if cfg.use_f0:
            x = x + w["enc_p.emb_pitch.weight"][pitch]
        x = x * f32c(math.sqrt(cfg.hidden_channels))
        x = torch.where(x > 0, x, x * f32c(0.01 if v == "slope001" else 0.1))
        return x * self._mask(lengths, x.shape[1])

    # ---- attention + LayerNorm 1 ------------------------------------------------------------------------------------------------------------
    def _attention(self, i, x, lengths):
        cfg, w = self.cfg, self.w
        v_ = self.variants.get("attn%d" % i)
        pre = "enc_p.encoder.attn_layers.%d." % i
        B, T, C = x.shape
        H, dk, ws = cfg.n_heads, C // cfg.n_heads, cfg.window_size
        nb = 2 * ws + 1
        xr = self.rnd(x)
        q = self.rnd(self.conv(xr, self.W(pre + "conv_q.weight"), w[pre + "conv_q.bias"]) / f32c(math.sqrt(dk)))
        k = self.rnd(self.conv(xr, self.W(pre + "conv_k.weight"), w[pre + "conv_k.bias"]))
        v = self.rnd(self.conv(xr, self.W(pre + "conv_v.weight"), w[pre + "conv_v.bias"]))
        Ek, Ev = self.W(pre + "emb_rel_k")[0], w[pre + "emb_rel_v"][0]  # [2ws+1, dk]; heads share them
        if v_ == "relk_edge":
            Ek = Ek.clone()
            Ek[nb - 1] = 0
        if v_ == "relv_edge":
            Ev = Ev.clone()
            Ev[0] = 0
        lens = torch.full((B,), T) if lengths is None else torch.as_tensor(lengths).clamp(max=T)
        nkt = (T + 31) // 32
        Tk = nkt * 32
        ii, jj = torch.arange(T).unsqueeze(1), torch.arange(Tk).unsqueeze(0)
        r = jj - ii + ws
        band = (r >= 0) & (r <= 2 * ws) & (jj < T)
        rc = r.clamp(0, 2 * ws)
        ninf = torch.tensor(-math.inf, dtype=self.dt)
        out = torch.zeros(B, T, C, dtype=self.dt)
        for b in range(B):
            L = int(lens[b])
            ok = (ii < L) & (jj < L)
            for h in range(H):
                sl = slice(h * dk, (h + 1) * dk)
                qh, kh, vh = q[b, :, sl], k[b, :, sl], v[b, :, sl]
                S = F.pad(self.mm(qh, kh.t()), (0, Tk - T))
                R = self.mm(qh, Ek.t())  # [T, 2ws+1]
                S = S + torch.where(band, torch.gather(R, 1, rc), torch.zeros((), dtype=self.dt))
                S = torch.where(ok, S, torch.tensor(-1e4, dtype=self.dt))
                S = torch.where(jj < T, S, ninf)  # tile padding: not a key at all
                vp = F.pad(vh, (0, 0, 0, Tk - T))
                # the four waves' online softmax
                tiles = list(range(nkt))
                if self.perturb.get("softmax"):
                    tiles = [int(t) for t in self.rng.permutation(nkt)]
                Ms, Ls, Os = [], [], []
                for wv in range(4):
                    m = torch.full((T, 1), -math.inf, dtype=self.dt)
                    l = torch.zeros(T, 1, dtype=self.dt)
                    O = torch.zeros(T, dk, dtype=self.dt)
                    for kt in tiles[wv::4]:
                        St = S[:, kt * 32:kt * 32 + 32]
                        m_new = torch.maximum(m, St.max(dim=1, keepdim=True).values)
                        p = self.exp(St - m_new)
                        sc = self.exp(m - m_new)  # 0 on a wave's first tile
                        l = l * sc + p.sum(dim=1, keepdim=True)
                        O = O * sc + self.mm(self.rnd(p), vp[kt * 32:kt * 32 + 32])
                        m = m_new
                    Ms.append(m), Ls.append(l), Os.append(O)
                M = torch.stack(Ms).max(dim=0).values
                e = [self.exp(m - M) for m in Ms]
                Lt, o = torch.zeros(T, 1, dtype=self.dt), torch.zeros(T, dk, dtype=self.dt)
                waves = [int(t) for t in self.rng.permutation(4)] if self.perturb.get("reorder") else range(4)
                for wv in waves:
                    Lt = Lt + Ls[wv] * e[wv]
                for wv in waves:
                    o = o + Os[wv] * (e[wv] / Lt)
                # relative values from the band scores: out_i += sum_r p[i, i + r - ws] E_v[r]
                Sb = torch.where(band, S, ninf)
                idx = (ii + torch.arange(nb).unsqueeze(0) - ws)  # key of band slot r
                inside = (idx >= 0) & (idx < T)
                Sband = torch.where(inside, torch.gather(Sb, 1, idx.clamp(0, Tk - 1)), ninf)  # [T, 2ws+1]
                pb = self.exp(Sband - M) * (1.0 / Lt)
                out[b, :, sl] = o + pb @ Ev
        y = self.conv(self.rnd(out), self.W(pre + "conv_o.weight"), w[pre + "conv_o.bias"])
        return y

    def attn(self, i, x, lengths):
        w = self.w
        x = self._t(x)
        y = self._attention(i, x, lengths)
        eps = 1e-3 if self.variants.get("attn%d" % i) == "eps" else 1e-5
        return self.layer_norm(x + y, w["enc_p.encoder.norm_layers_1.%d.gamma" % i], w["enc_p.encoder.norm_layers_1.%d.beta" % i], eps)

    # ---- FFN + LayerNorm 2 ----------------------------------------------------------------------------------------------------------------
    def ffn_head(self, i, x, lengths):
        """conv_1 + ReLU + mask -> {"x", "m", "hid" (before the operand rounding), "hr" (rounded), "other" (the operand value on the far side of ``hid``; ``hr``
        itself where hid is one), "ties": [(b, t, channel)] of the hidden values below the length whose rounding float32 accumulation leaves open: those
        within TIE_FP32_ULPS float32 ulps (of the value) of the midpoint between ``hr`` and ``other``}"""
        w = self.w
        v = self.variants.get("ffn%d" % i)
        pre = "enc_p.encoder.ffn_layers.%d." % i
        x = self._t(x)
        m = self._mask(lengths, x.shape[1])
        w1 = self.W(pre + "conv_1.weight")
        if isinstance(v, tuple) and v[0] == "tap":  # ("tap", gain): the last tap of conv_1 x gain
            w1 = w1.clone()
            w1[:, :, -1] *= v[1]
        hid = torch.relu(self.conv(self.rnd(x * m), w1, w[pre + "conv_1.bias"]))
        hid = hid if v == "hidden_unmasked" else hid * m
        hr = self.rnd(hid)
        head = {"x": x, "m": m, "hid": hid, "hr": hr, "other": hr, "ties": []}
        if self.operand is not None:
            mant, ex = torch.frexp(hr)  # hr = mant * 2^ex, mant in [0.5, 1)
            ulp = torch.ldexp(torch.ones_like(hr), ex - {"fp16": 11, "bf16": 8}[self.operand])
            if self.operand == "fp16":
                ulp = ulp.clamp(min=2.0 ** -24)  # subnormals
            step = torch.where((hid > hr) | (mant.abs() != 0.5), ulp, ulp / 2)  # below a power of two the spacing halves
            other = hr + torch.sign(hid - hr) * step
            u32 = torch.ldexp(torch.ones_like(hid), torch.frexp(hid)[1] - 24)
            near = (other != hr) & (((hr + other) / 2 - hid).abs() <= TIE_FP32_ULPS * u32) & (m > 0)
            head.update(other=other, ties=[tuple(int(k) for k in idx) for idx in near.nonzero()])
        return head

    def ffn_tail(self, i, head, flipped=()):
        """conv_2, mask, + x, LayerNorm 2 on the rounded hidden activation, the values at ``flipped`` rounded to the other neighbour"""
        w = self.w
        pre = "enc_p.encoder.ffn_layers.%d." % i
        hr = head["hr"]
        if flipped:
            hr = hr.clone()
            for idx in flipped:
                hr[idx] = head["other"][idx]
        y = self.conv(hr, self.W(pre + "conv_2.weight"), w[pre + "conv_2.bias"], groups="quarters") * head["m"]
        eps = 1e-3 if self.variants.get("ffn%d" % i) == "eps" else 1e-5
        return self.layer_norm(head["x"] + y, w["enc_p.encoder.norm_layers_2.%d.gamma" % i], w["enc_p.encoder.norm_layers_2.%d.beta" % i], eps)

    def ffn(self, i, x, lengths):
        return self.ffn_tail(i, self.ffn_head(i, x, lengths))

    # ---- proj + prior sample --------------------------------------------------------------------------------------------------------------
    def z_p(self, x, lengths, noise, flow_head=0):
        cfg, w = self.cfg, self.w
        fh = int(flow_head or 0)
        x = self._t(x)[:, fh:]
        m = self._mask(lengths, x.shape[1], fh)
        stats = self.conv(self.rnd(x * m), self.W("enc_p.proj.weight"), w["enc_p.proj.bias"]) * m
        mean, logs = stats[..., :cfg.inter_channels], stats[..., cfg.inter_channels:]
        c = 2.0 / 3.0 if self.variants.get("z_p") == "two_thirds" else f32c(0.66666)
        # expf, not the hardware exp (front_kernels.hpp:336); the products left to right
        return (mean + torch.exp(logs) * self._t(noise).transpose(1, 2) * c) * m

    # ---- one coupling layer of the reversed flow ---------------------------------------------------------------------------------------------
    def cond(self, f, g):
        """cond_layer(g) of coupling f: [B, 2H * n_layers], fp32 on the device (k_cond)"""
        w, pre = self.w, "flow.flows.%d.enc." % (2 * f)
        return self._t(g).reshape(-1, self.cfg.gin_channels) @ w[pre + "cond_layer.weight"][:, :, 0].t() + w[pre + "cond_layer.bias"]

    def flow(self, f, zp, lengths, g, flow_head=0, skip0=None, want_skip=False):
        cfg, w = self.cfg, self.w
        v = self.variants.get("flow%d" % f)
        Hc, half, nl = cfg.hidden_channels, cfg.inter_channels // 2, cfg.flow_n_layers
        pre = "flow.flows.%d." % (2 * f)
        odd = (cfg.flow_n_flows - f) % 2 == 1
        phys = self._t(zp)
        x = torch.flip(phys, [2]) if odd else phys  # the logical tensor
        m = self._mask(lengths, x.shape[1], int(flow_head or 0))
        x0, x1 = x[..., :half], x[..., half:]
        h = self.conv(self.rnd(x0), self.W(pre + "pre.weight"), w[pre + "pre.bias"]) * m
        gc = self.cond(f, g) if cfg.gin_channels else None
        skip = None
        for l in range(nl):
            wi = self.W(pre + "enc.in_layers.%d.weight" % l)
            if isinstance(v, tuple) and v[0] == "tap" and l == 1:  # ("tap", gain): the last tap of in_layers.1 x gain
                wi = wi.clone()
                wi[:, :, -1] *= v[1]
            bg = w[pre + "enc.in_layers.%d.bias" % l]
            if gc is not None:
                ls = (l + 1) % nl if v == "gc_wrong_layer" else l
                bg = bg + gc[:, ls * 2 * Hc:(ls + 1) * 2 * Hc].unsqueeze(1)
            a = self.conv(self.rnd(h), wi, None, groups="taps") + bg
            acts = self.rnd(self.tanh(a[..., :Hc]) * self.sigmoid(a[..., Hc:]))
            rs = self.conv(acts, self.W(pre + "enc.res_skip_layers.%d.weight" % l), w[pre + "enc.res_skip_layers.%d.bias" % l])
            if l < nl - 1:
                h = (h + rs[..., :Hc]) * m
                s = rs[..., Hc:]
            else:
                s = rs
            if l == 0:
                skip = s if skip0 is None else s + self._t(skip0)  # skip0: variant "the skip sum is not reset at first"
            else:
                skip = skip + s
        if want_skip:
            return skip
        mean = self.conv(self.rnd(skip * m), self.W(pre + "post.weight"), w[pre + "post.bias"])
        x1 = (x1 - mean * m) * m
        y = torch.cat([x0, x1], dim=2)
        return torch.flip(y, [2]) if odd else y

    # ---- transpose + mask -------------------------------------------------------------------------------------------------------------------
    def out(self, zp, lengths, flow_head=0):
        zp = self._t(zp)
        if self.cfg.flow_n_flows % 2 == 1 and self.variants.get("out") != "physical_order":
            zp = torch.flip(zp, [2])  # an odd number of flips in all: the buffer holds z with its channel axis reversed (k_fr_out's ``rev``)
        return (zp * self._mask(lengths, zp.shape[1], int(flow_head or 0))).transpose(1, 2).contiguous()

    # ---- the segments composed --------------------------------------------------------------------------------------------------------------
    def forward(self, phone, pitch, lengths, g, noise, flow_head=0, taps: Optional[dict] = None):
        """The whole front, each segment fed the previous segment's output -> z [B, 192, T - flow_head]; ``taps`` receives every segment's output."""
        inp = {"phone": phone, "pitch": pitch, "lengths": lengths, "g": g, "noise": noise, "flow_head": flow_head}
        t = taps if taps is not None else {}
        for name in segment_names(self.cfg):
            t[name] = apply_segment(self, name, {**inp, **t})
        return t["out"]


def segment_names(cfg: FrontConfig):
    return (["emb"] + [nm for i in range(cfg.n_layers) for nm in ("attn%d" % i, "layer%d" % i)] + ["z_p"]
            + ["flow%d" % f for f in reversed(range(cfg.flow_n_flows))] + ["out"])


def feed_of(cfg: FrontConfig, name: str) -> Optional[str]:
    """The tap segment ``name`` consumes (None: the raw inputs alone)"""
    names = segment_names(cfg)
    return None if name == "emb" else names[names.index(name) - 1]


def variant_key(name: str) -> str:
    """Segment "layer<i>" looks its variant up as "ffn<i>" (the segment is the FFN half of encoder layer i)"""
    return "ffn" + name[5:] if name.startswith("layer") else name


def apply_segment(sg: Segments, name: str, inputs: dict):
    """Segment ``name`` of ``sg`` applied to ``inputs``: the raw inputs (phone, pitch, lengths, g, noise, flow_head) and the tap it consumes."""
    cfg, ln, fh = sg.cfg, inputs.get("lengths"), inputs.get("flow_head") or 0
    if name == "emb":
        return sg.emb(inputs["phone"], inputs.get("pitch"), ln)
    x = inputs[feed_of(cfg, name)]
    if name.startswith("attn"):
        return sg.attn(int(name[4:]), x, ln)
    if name.startswith("layer"):
        return sg.ffn(int(name[5:]), x, ln)
    if name == "z_p":
        return sg.z_p(x, ln, inputs["noise"], fh)
    if name.startswith("flow"):
        return sg.flow(int(name[4:]), x, ln, inputs.get("g"), fh, inputs.get("skip0"))
    assert name == "out", name
    return sg.out(x, ln, fh)
