"""Plain numpy restatement of the bidirectional GRU of csrc/gru.hip (torch.nn.GRU(I, 256, num_layers=1, batch_first=True, bidirectional=True),
h_0 = 0), written from the torch.nn.GRU documentation and the comment at the top of gru.hip.  Checker only: nothing in the product imports it.

PyTorch's cell (gate order r, z, n in the stacked weights; b_hn inside the r * (...) term):

    r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
    n = tanh(W_in x + b_in + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h

``round_operands`` applies the kernel's documented design: x, W_ih, W_hh and the copy of h that enters W_hh . h are rounded to fp16
(round-to-nearest-even); the biases, the projection GX = x . W_ih^T + b, the gates and the carried state are not.

``arith="f64"`` is the oracle.  ``arith="f32"`` is the same recurrence with every intermediate held in float32 and the gates written in the
two forms the kernel's comment documents, 1 / (1 + exp(-v)) and 2 / (1 + exp(-2v)) - 1: the noise floor of an fp32 evaluation (fp32 rounding
flipping the fp16 rounding of h), NOT a model of the device.

``variant`` names a deliberately WRONG recurrence (tests/test_cpu_gru.py: every one must stand clear of the bar the kernel is held to):

    state_fp16    the state fed back through its fp16 copy (z * h uses the rounded h)
    gx_fp16       the projection GX stored as fp16
    h_trunc       the fp16 copy of h truncated towards zero instead of rounded to nearest
    gh_fp16       W_hh . h rounded to fp16
    bhn_outside   b_hn added outside r * (...)
    no_bhh_rz     b_hh left out of the r and z gates
    tail_gx       the last step reads the GX of the step before it
"""
import numpy as np

H = 256
VARIANTS = ("state_fp16", "gx_fp16", "h_trunc", "gh_fp16", "bhn_outside", "no_bhh_rz", "tail_gx")


def _f16(a):
    """Round to fp16 (nearest even), keep the dtype."""
    return a.astype(np.float16).astype(a.dtype)


def _f16_trunc(a):
    """To fp16 towards zero, keep the dtype."""
    r = a.astype(np.float16)
    over = np.abs(r.astype(a.dtype)) > np.abs(a)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(a.dtype)


def bigru(w_ih, w_hh, b_ih, b_hh, x, arith="f64", variant=None, round_operands=True):
    """w_ih [2, 768, I], w_hh [2, 768, 256], b_ih / b_hh [2, 768] (forward, reverse: as ``GRUHIP.__init__`` stacks them), x [B, T, I]
    -> (y [B, T, 512], hn [2, B, 256]) in float64 (``arith="f32"``: float32)."""
    if arith not in ("f64", "f32"):
        raise ValueError("arith: %r" % (arith,))
    if variant is not None and variant not in VARIANTS:
        raise ValueError("variant: %r" % (variant,))
    dt = np.float64 if arith == "f64" else np.float32
    w_ih, w_hh, b_ih, b_hh, x = (np.asarray(a, dtype=np.float64) for a in (w_ih, w_hh, b_ih, b_hh, x))
    if round_operands:
        w_ih, w_hh, x = _f16(w_ih), _f16(w_hh), _f16(x)
    w_ih, w_hh, b_ih, b_hh, x = (a.astype(dt) for a in (w_ih, w_hh, b_ih, b_hh, x))
    B, T, _ = x.shape
    copy_of_h = (_f16_trunc if variant == "h_trunc" else _f16) if round_operands else (lambda a: a)
    y = np.zeros((B, T, 2 * H), dt)
    hn = np.zeros((2, B, H), dt)
    with np.errstate(over="ignore"):  # (exp past the format's range: inf, and 1 / inf = 0 is the gate's limit)
        for d in range(2):
            b_rz = b_ih[d].copy()  # what adds in front of the sigmoid: b_ih + b_hh for r and z; b_hn stays with W_hn h
            if variant != "no_bhh_rz":
                b_rz[:2 * H] += b_hh[d, :2 * H]
            b_hn = b_hh[d, 2 * H:]
            gx = x @ w_ih[d].T + b_rz  # [B, T, 768]
            if variant == "gx_fp16":
                gx = _f16(gx)
            whh_t = np.ascontiguousarray(w_hh[d].T)
            h = np.zeros((B, H), dt)
            for s in range(T):
                t = T - 1 - s if d else s
                g = gx[:, t]
                if variant == "tail_gx" and s == T - 1 and T > 1:
                    g = gx[:, t + 1 if d else t - 1]
                gh = copy_of_h(h) @ whh_t
                if variant == "gh_fp16":
                    gh = _f16(gh)
                r = 1 / (1 + np.exp(-(g[:, :H] + gh[:, :H])))
                z = 1 / (1 + np.exp(-(g[:, H:2 * H] + gh[:, H:2 * H])))
                if variant == "bhn_outside":
                    v = g[:, 2 * H:] + r * gh[:, 2 * H:] + b_hn
                else:
                    v = g[:, 2 * H:] + r * (gh[:, 2 * H:] + b_hn)
                n = np.tanh(v) if arith == "f64" else 2 / (1 + np.exp(-2 * v)) - 1
                h = (1 - z) * n + z * (_f16(h) if variant == "state_fp16" else h)
                y[:, t, d * H:(d + 1) * H] = h
            hn[d] = h
    return y, hn


def ragged(w_ih, w_hh, b_ih, b_hh, x_rows, offsets, arith="f64", variant=None, round_operands=True):
    """The same per sequence over packed rows: x_rows [M, I], sequence i = rows [offsets[i], offsets[i + 1]) -> (y [M, 512], hn [2, n, 256])."""
    ys, hs = [], []
    for i in range(len(offsets) - 1):
        y, hn = bigru(w_ih, w_hh, b_ih, b_hh, np.asarray(x_rows)[None, offsets[i]:offsets[i + 1]], arith, variant, round_operands)
        ys.append(y[0])
        hs.append(hn[:, 0])
    return np.concatenate(ys), np.stack(hs, axis=1)
