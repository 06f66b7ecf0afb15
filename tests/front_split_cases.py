"""The front's ``"fp16x2"`` operand mode restated on the CPU oracle (shared by test_cpu_front_split.py, test_gpu_front_split.py and
tools/front_split_parity.py), with the EXACT arithmetic of csrc/front_split_kernels.hpp:

* every MFMA operand x is the pair  hi = fp16(x),  lo' = fp16((x - hi) * 2^11)  (csrc/split_f16.hpp), both saturating at +-65504;
* a product is  A_hi.B_hi + 2^-11 * (A_hi.B_lo' + A_lo'.B_hi)  with fp32 accumulation -- the lo.lo term is dropped, the bracket has an
  accumulator of its own;
* the operands are the conv / linear inputs and weights (so also the FFN's ReLU output and the WN gate output, which are conv inputs),
  q / sqrt(dk), k, v, the relative KEY embeddings and the softmax probabilities;
* fp32, as on the device in every mode: biases, the pitch embedding, LayerNorm, softmax, tanh / sigmoid, masks, the residual and flow
  streams, the relative VALUE term, and cond_layer(g) (csrc k_cond is an fp32 kernel).

``mode``: "fp32" (the oracle as it is), "fp16" (operands rounded to fp16: today's default arithmetic) or "fp16x2".  ``emulate`` swaps
``front_oracle.F`` and ``front_oracle.attention`` and always restores them.  What the emulator does not reproduce: the order of the fp32
accumulation, the hardware exp of softmax / sigmoid / tanh, and the online (unnormalised) softmax whose probabilities the kernel splits.
"""
import contextlib
import math

import torch
import torch.nn.functional as TF

from oracle import front_oracle as fo

SCALE = 2048.0  # 2^11
INV = 1.0 / 2048.0
F16_MAX = 65504.0
MODES = ("fp32", "fp16", "fp16x2")


def split(t):
    """fp32 tensor -> (hi, lo') as fp32 tensors that hold fp16 values."""
    hi = t.clamp(-F16_MAX, F16_MAX).half().float()
    lo = ((t - hi) * SCALE).clamp(-F16_MAX, F16_MAX).half().float()
    return hi, lo


def join(hi, lo):
    return hi + lo * INV


def _product(mode, fn, a, b):
    """fn(a, b) -- bilinear -- on operands of the given mode."""
    if mode == "fp32":
        return fn(a, b)
    if mode == "fp16":
        return fn(a.clamp(-F16_MAX, F16_MAX).half().float(), b.clamp(-F16_MAX, F16_MAX).half().float())
    ah, al = split(a)
    bh, bl = split(b)
    return fn(ah, bh) + (fn(ah, bl) + fn(al, bh)) * INV


class _F:
    """Stands in for ``torch.nn.functional`` inside front_oracle: conv1d / linear on operands of the mode."""

    def __init__(self, mode, plain_weights=()):
        self.mode = mode
        self.plain = {id(t) for t in plain_weights}  # convs that are fp32 kernels on the device in every mode

    def __getattr__(self, name):
        return getattr(TF, name)

    def conv1d(self, x, weight, bias=None, **kw):
        mode = "fp32" if id(weight) in self.plain else self.mode
        y = _product(mode, lambda a, b: TF.conv1d(a, b, None, **kw), x, weight)
        return y if bias is None else y + bias.view(1, -1, 1)

    def linear(self, x, weight, bias=None):
        y = _product(self.mode, TF.linear, x, weight)
        return y if bias is None else y + bias


def _attention(mode, cfg, w, pre, x, mask):
    """front_oracle.attention with its four products on operands of the mode (the conv_q/k/v/o go through front_oracle.F)."""
    F = fo.F
    B, C, T = x.shape
    H, dk, ws = cfg.n_heads, C // cfg.n_heads, cfg.window_size
    q = F.conv1d(x, w[pre + "conv_q.weight"], w[pre + "conv_q.bias"])
    k = F.conv1d(x, w[pre + "conv_k.weight"], w[pre + "conv_k.bias"])
    v = F.conv1d(x, w[pre + "conv_v.weight"], w[pre + "conv_v.bias"])
    q = q.view(B, H, dk, T).transpose(2, 3) / math.sqrt(dk)
    k = k.view(B, H, dk, T).transpose(2, 3)
    v = v.view(B, H, dk, T).transpose(2, 3)
    mm = lambda a, b: _product(mode, torch.matmul, a, b)
    scores = mm(q, k.transpose(-2, -1))
    Ek, Ev = w[pre + "emb_rel_k"][0], w[pre + "emb_rel_v"][0]
    rel = mm(q, Ek.t())
    ii = torch.arange(T).unsqueeze(1)
    jj = torch.arange(T).unsqueeze(0)
    r = jj - ii + ws
    band = (r >= 0) & (r <= 2 * ws)
    rc = r.clamp(0, 2 * ws)
    scores = scores + torch.where(band, torch.gather(rel, -1, rc.expand(B, H, T, T)), torch.zeros(()))
    am = mask.unsqueeze(1).unsqueeze(-1) * mask.unsqueeze(1).unsqueeze(2)
    scores = scores.masked_fill(am == 0, -1e4)
    p = torch.softmax(scores, dim=-1)
    out = mm(p, v)
    pb = torch.where(band, p, torch.zeros(()))
    for rr in range(2 * ws + 1):  # relative values: fp32 on the device too
        d = rr - ws
        diag = torch.diagonal(pb, offset=d, dim1=-2, dim2=-1)
        lo = max(0, -d)
        out[:, :, lo:lo + diag.shape[-1], :] += diag.unsqueeze(-1) * Ev[rr]
    out = out.transpose(2, 3).contiguous().view(B, C, T)
    return F.conv1d(out, w[pre + "conv_o.weight"], w[pre + "conv_o.bias"])


@contextlib.contextmanager
def emulate(mode, w):
    """front_oracle computes in ``mode`` inside the block; its ``F`` and ``attention`` are restored afterwards, whatever happens."""
    assert mode in MODES, mode
    saved = (fo.F, fo.attention)
    try:
        if mode != "fp32":
            fo.F = _F(mode, [t for name, t in w.items() if name.endswith("cond_layer.weight")])
            fo.attention = lambda *a: _attention(mode, *a)
        yield
    finally:
        fo.F, fo.attention = saved


def run_front(mode, cfg, w, phone, pitch, lengths, sid, noise, flow_head=None, taps=None, dtype=None):
    """``z * x_mask`` [B, inter, T'] of the oracle front in ``mode``; ``dtype=torch.float64`` (mode "fp32"): the fp64 run, weights and
    inputs cast.  ``taps``: a dict that receives emb / attn0 / layer<i> / z_p CHANNELS-LAST [B, T', 192], as ``FrontHIP.debug_tap``
    returns them."""
    if dtype is not None:
        assert mode == "fp32"
        w = {k: v.to(dtype) if v.is_floating_point() else v for k, v in w.items()}
        phone, noise = phone.to(dtype), noise.to(dtype)
    raw = {} if taps is not None else None
    with torch.no_grad(), emulate(mode, w):
        z, m1, _ = fo.infer_front(cfg, w, phone, pitch, lengths, sid, noise, flow_head if flow_head else None, raw)
        z = z * m1
    if taps is not None:
        for k, v in raw.items():
            if k not in ("m", "logs"):
                taps[k] = v.transpose(1, 2).contiguous()
    return z


def rms(a, b):
    a = torch.as_tensor(a, dtype=torch.float64)
    b = torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).pow(2).mean().sqrt())
