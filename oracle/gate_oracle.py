"""The realtime GUI's spectral gate (``TorchGate.forward``, infer/modules/gui/torchgate.py:210-280, utils.py:5-41) in plain numpy fp64,
stage by stage, for the arguments of ``glue.spectral_gate``; with every stage the forward-error bound ("bar") that a device which sums
in fp64 must stay inside, computed from the case's own data, and for the stationary mask the margin of every decision.

    r = gate(x, xn, n_fft, hop, window, filt, nonstationary=..., prop_decrease=...)
    r["X"], r["XN"]         [B, F, K] / [B, Fn, K] complex    zero padding by n_fft / 2, F = 1 + L // hop
    r["xmax"], r["thresh"]  [B, K]                            amp_to_db's 40 dB clamp from each signal's own maximum, unbiased std
    r["m"], r["mraw"]       [B, F, K] fp32                    the decision / the fp32-rounded sigmoid; prop * (m - 1) + 1 in fp32 arithmetic
    r["msk"], r["Y"]        smooth(mraw) (fp64 sum), X * msk
    r["z"]                  [B, F, n_fft]                     window * irfft(Y)
    r["y"]                  [B, hop * (L // hop)]             overlap-add / summed squared window, centre trim
    r["bar_<stage>"]        the bound of that stage;  r["margin"], r["margin_bound"]  [B, F, K] in dB (stationary)

The mask rounds to fp32 where the reference does (``sig_mask.float()``) and the filter is the fp32 data it is; the smoothing sum and
everything else are fp64 (``smooth_fp32=True`` sums in fp32 instead, as the reference's conv2d on its fp32 mask).  "same" padding is
torch's: left pad (k - 1) // 2, cross-correlation.  ``variant`` names one deliberate mistake (VARIANTS); the tests use them to show
that the bars are tight enough to catch it.

The bars (worst case, first order):
  X       n-term fp64 sum of products with a 1-ulp twiddle: |dX_k| <= (n_fft + 2) 2^-53 sum_m |win[m] x[m]| per frame
  dB      that bound through 20 log10(|X| + eps) exactly (log1p), so a bin near zero widens only its own entry
  xmax    the largest dB bound among the frames that can be the maximum
  thresh  the clamped dB bounds through the mean (their mean) and the unbiased std (their 2-norm / sqrt(Fn - 1): the std is the norm
          of the centred vector), plus Fn 2^-53 magnitude for the sums
  mraw    stationary: none (bit-equal; the margins make that well defined).  Non-stationary: one fp32 ulp at the value plus the
          sigmoid's slope (1/4 per unit of its argument) times the argument's propagated bound
  msk     nf nt 2^-24 sum|filt| for the fp32 smoothing chain (mask <= 1), plus the smoothed mraw bound
  Y, z, y the above through the product, the inverse sum and the overlap-add; the overlap-add is divided by the case's own summed
          squared window at each sample; y adds half an fp32 ulp at the value
"""
import numpy as np

U = 2.0 ** -53
EPS = float(np.finfo(np.float64).eps)
DB = 20.0 / np.log(10.0)  # d(20 log10 a) / d(ln a)
VARIANTS = ("biased_std", "clamp_from_x", "no_clamp", "reflect_pad", "movemean_other_side", "smooth_flipped", "smooth_other_side",
            "ola_no_division", "keep_last_partial_hop")
WINDOW_VARIANTS = ("symmetric_hann", "window_not_centred")


def hann_window(n_fft, win_length=None, variant=None):
    """torch.stft's window: torch.hann_window(win_length) (periodic), zero-padded to n_fft at the centre, fp64."""
    wl = n_fft if win_length is None else win_length
    den = wl - 1 if variant == "symmetric_hann" else wl
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(wl) / den) if wl > 1 else np.ones(1)
    out = np.zeros(n_fft)
    left = 0 if variant == "window_not_centred" else (n_fft - wl) // 2
    out[left: left + wl] = w
    return out


def ola_envelope(window, n_fft, hop, L):
    """The summed squared window over the samples torch.istft keeps: [hop * (L // hop)]."""
    F, h = 1 + L // hop, n_fft // 2
    env = np.zeros(n_fft + hop * (F - 1))
    for f in range(F):
        env[f * hop: f * hop + n_fft] += window ** 2
    return env[h: h + hop * (L // hop)]


def _frames(x, n_fft, hop, reflect):
    B, L = x.shape
    F, h = 1 + L // hop, n_fft // 2
    xp = np.pad(x, ((0, 0), (h, h)), mode="reflect" if reflect else "constant")
    return xp[:, np.arange(F)[:, None] * hop + np.arange(n_fft)[None]]


def _stft(x, n_fft, hop, window, reflect=False):
    fr = _frames(np.asarray(x, np.float64), n_fft, hop, reflect) * window
    return np.fft.rfft(fr, axis=-1), (n_fft + 2) * U * np.abs(fr).sum(-1, keepdims=True)


def _db(X, barX):
    """20 log10(|X| + eps), and how far up / down |dX| <= barX can move it (plus the roundings of sqrt, log10 and the product)."""
    a = np.abs(X) + EPS
    db = 20.0 * np.log10(a)
    r = barX / a
    rnd = 8 * U * (np.abs(db) + DB)
    with np.errstate(divide="ignore", invalid="ignore"):
        up = DB * np.log1p(r) + rnd
        dn = np.where(r < 1.0, -DB * np.log1p(-np.minimum(r, 1.0)), np.inf) + rnd
    return db, up, dn


def _clamped(db, up, dn, floor_from=None):
    """amp_to_db's max over frames (axis 1) and the clamp at max - 40, with bounds.  floor_from: (max, bound) of another signal."""
    mx = db.max(1)
    lo = (db - dn).max(1, keepdims=True)
    e = np.maximum(up, dn)
    e_mx = np.where(db + up >= lo, e, 0.0).max(1)
    fmx, e_f = (mx, e_mx) if floor_from is None else floor_from
    floor = (fmx - 40.0)[:, None]
    c = np.maximum(db, floor)
    sure_below = db + up < floor - e_f[:, None]
    e_c = np.where(sure_below, e_f[:, None], np.maximum(e, e_f[:, None]))
    return mx, e_mx, c, e_c


def _same_pad_left(k, other_side):
    return k - 1 - (k - 1) // 2 if other_side else (k - 1) // 2


def _moving_sum(a, k, left):
    """out[f] = sum_j a[f - left + j], j < k, zeros outside; a [B, F, K]."""
    F = a.shape[1]
    ap = np.pad(a, ((0, 0), (left, max(k - 1 - left, 0) + k), (0, 0)))
    out = np.zeros_like(a)
    for j in range(k):
        out += ap[:, j: j + F]
    return out


def smooth(m, filt, left_f, left_t, fp32=False):
    """conv2d(m [B, F, K] viewed as (bin, frame), filt [nf, nt], padding='same'): a cross-correlation, bins outer, frames inner."""
    nf, nt = filt.shape
    B, F, K = m.shape
    dt = np.float32 if fp32 else np.float64
    mp = np.pad(m.astype(dt), ((0, 0), (left_t, nt), (left_f, nf)))
    out = np.zeros((B, F, K), dt)
    for i in range(nf):
        for j in range(nt):
            out = out + dt(filt[i, j]) * mp[:, j: j + F, i: i + K]
    return out


def _ola(z, n_fft, hop):
    B, F, _ = z.shape
    acc = np.zeros((B, n_fft + hop * (F - 1)))
    for f in range(F):
        acc[:, f * hop: f * hop + n_fft] += z[:, f]
    return acc


def gate(x, xn, n_fft, hop, window, filt=None, nonstationary=False, n_std_thresh=1.5, n_thresh_ns=1.3, temp_coeff=0.1, n_movemean=20,
         prop_decrease=1.0, variant=None, smooth_fp32=False):
    assert variant is None or variant in VARIANTS, variant
    x = np.asarray(x, np.float64)
    window = np.asarray(window, np.float64)
    B, L = x.shape
    F, K, h = 1 + L // hop, n_fft // 2 + 1, n_fft // 2
    r = {}
    reflect = variant == "reflect_pad"
    X, barX = _stft(x, n_fft, hop, window, reflect)
    r["X"], r["bar_X"] = X, np.broadcast_to(barX, X.shape)
    db, up, dn = _db(X, barX)
    xmax, e_xmax, cx, e_cx = _clamped(db, up, dn)
    r["xmax"], r["bar_xmax"] = xmax, e_xmax
    prop = np.float32(prop_decrease)
    if not nonstationary:
        if xn is not None:
            XN, barXN = _stft(xn, n_fft, hop, window, reflect)
            r["XN"], r["bar_XN"] = XN, np.broadcast_to(barXN, XN.shape)
            ndb, nup, ndn = _db(XN, barXN)
            _, _, cn, e_cn = _clamped(ndb, nup, ndn, (xmax, e_xmax) if variant == "clamp_from_x" else None)
        else:
            ndb, nup, ndn, cn, e_cn = db, up, dn, cx, e_cx
        if variant == "no_clamp":
            cn, e_cn, cx, e_cx = ndb, np.maximum(nup, ndn), db, np.maximum(up, dn)
        Fn = cn.shape[1]
        mean = cn.mean(1)
        with np.errstate(divide="ignore", invalid="ignore"):
            std = np.sqrt(((cn - mean[:, None]) ** 2).sum(1) / (Fn if variant == "biased_std" else Fn - 1))
            big = np.abs(cn).max(1)
            e_mean = e_cn.mean(1) + Fn * U * big
            e_std = (np.sqrt((e_cn ** 2).sum(1)) + np.sqrt(Fn) * Fn * U * big) / np.sqrt(Fn - 1) + (Fn + 4) * U * std
        thresh = mean + std * n_std_thresh
        r["thresh"], r["bar_thresh"] = thresh, e_mean + abs(n_std_thresh) * e_std + 2 * U * np.abs(thresh)
        with np.errstate(invalid="ignore"):
            m = (cx > thresh[:, None]).astype(np.float32)
            r["margin"], r["margin_bound"] = np.abs(cx - thresh[:, None]), e_cx + r["bar_thresh"][:, None]
        bar_m = np.zeros(m.shape)
    else:
        a = np.abs(X)
        bar_a = barX + 2 * U * a
        left = _same_pad_left(n_movemean, variant == "movemean_other_side")
        s = _moving_sum(a, n_movemean, left) / n_movemean
        bar_s = _moving_sum(np.broadcast_to(bar_a, a.shape).copy(), n_movemean, left) / n_movemean + (n_movemean + 1) * U * s
        den = s + 1e-6
        ratio = (a - s) / den
        e_ratio = (bar_a + bar_s) / den + np.abs(a - s) * bar_s / den ** 2 + 3 * U * np.abs(ratio)
        arg = (ratio - n_thresh_ns) / temp_coeff
        e_arg = e_ratio / abs(temp_coeff) + 3 * U * (np.abs(arg) + abs(n_thresh_ns / temp_coeff))
        with np.errstate(over="ignore"):
            m = (1.0 / (1.0 + np.exp(-arg))).astype(np.float32)
        bar_m = float(prop) * (0.25 * e_arg + 4 * U)
    mraw = prop * (m - np.float32(1.0)) + np.float32(1.0)
    assert mraw.dtype == np.float32
    r["m"], r["mraw"] = m, mraw
    r["bar_mraw"] = bar_m + (np.spacing(np.abs(mraw)).astype(np.float64) if nonstationary else 0.0)
    if filt is not None:
        filt = np.asarray(filt, np.float32)
        nf, nt = filt.shape
        fl = filt[::-1, ::-1] if variant == "smooth_flipped" else filt
        lf, lt = _same_pad_left(nf, variant == "smooth_other_side"), _same_pad_left(nt, variant == "smooth_other_side")
        msk = smooth(mraw, fl, lf, lt, smooth_fp32).astype(np.float64)
        bar_msk = nf * nt * 2.0 ** -24 * float(np.abs(filt.astype(np.float64)).sum()) + smooth(r["bar_mraw"], np.abs(fl), lf, lt)
    else:
        msk, bar_msk = mraw.astype(np.float64), r["bar_mraw"] + np.zeros(mraw.shape)
    r["msk"], r["bar_msk"] = msk, bar_msk
    Y = X * msk
    r["Y"], r["bar_Y"] = Y, barX * np.abs(msk) + np.abs(X) * bar_msk + 2 * U * np.abs(Y)
    wk = np.full(K, 2.0)
    wk[0] = wk[-1] = 1.0
    z = np.fft.irfft(Y, n=n_fft, axis=-1) * window
    r["z"] = z
    r["bar_z"] = np.abs(window) * (((r["bar_Y"] + (K + 3) * U * np.abs(Y)) * wk).sum(-1, keepdims=True) / n_fft)
    Lout = L if variant == "keep_last_partial_hop" else hop * (L // hop)
    env = _ola(np.broadcast_to(window ** 2, (1, F, n_fft)), n_fft, hop)[:, h: h + Lout]
    acc = _ola(z, n_fft, hop)[:, h: h + Lout]
    with np.errstate(divide="ignore", invalid="ignore"):
        y = acc if variant == "ola_no_division" else acc / env
        bar64 = (_ola(r["bar_z"], n_fft, hop)[:, h: h + Lout] + (2 * F + 4) * U * _ola(np.abs(z), n_fft, hop)[:, h: h + Lout]) / env
    r["y"], r["env"], r["bar_y64"] = y, env[0], bar64
    with np.errstate(invalid="ignore", over="ignore"):
        r["bar_y"] = bar64 + 0.5 * np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
    return r
