"""The spectral gate's edge cases, shared by tests/test_cpu_gate_oracle.py, tests/test_gpu_gate_edges.py and tools/gate_parity.py: the
case table, the seeded inputs, the windows and filters, the scratch layout of rvcmi_glue_spectral_gate restated, and the oracle run
(oracle/gate_oracle.py) of each case, computed once.

The kernels' edges the table walks (csrc/gate_kernels.hpp): blocks of 64 bins (K = n_fft / 2 + 1), 64 samples and 8 frames; LDS rounds of
512 samples (forward) and 256 bins (inverse), split over four waves; 16 waves over the frames of the statistics and the division by
Fn - 1; 256 bins per mask / smoothing block and "same" padding, asymmetric for an even kernel; n_fft = 4096, the largest."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from oracle import gate_oracle

SR = 8000


@dataclass(frozen=True)
class Case:
    name: str
    n_fft: int
    hop: int
    L: int
    Ln: int = 0                      # 0: xn = None
    gains: Tuple[float, ...] = (1.0,)
    win_length: Optional[int] = None
    window: str = "hann"             # "hamming": through the raw call only
    filt: object = None              # None | ("tg", freq_mask_smooth_hz, time_mask_smooth_ms) | a RAW_FILTERS key
    nonstat: bool = False
    nmm: int = 20
    temp: float = 0.1
    prop: float = 0.9
    xn_gain: float = 0.3             # xn's level against x's: a noise clip, quieter than the signal
    lead: float = 0.05               # the gain of xn's first third
    seed: int = 0

    @property
    def B(self):
        return len(self.gains)

    @property
    def F(self):
        return 1 + self.L // self.hop

    @property
    def K(self):
        return self.n_fft // 2 + 1

    @property
    def Lout(self):
        return self.hop * (self.L // self.hop)

    @property
    def is_class(self):
        """Can TorchGate's constructor express it (its own window, hop and filter)?"""
        return self.window == "hann" and (self.filt is None or isinstance(self.filt, tuple))


def _big_filter():
    f = np.random.default_rng(77).random((7, 9)) + 0.05
    return (f / f.sum()).astype(np.float32)


RAW_FILTERS = {
    "1x1": np.array([[1.0]], np.float32),
    "1x5": np.array([[0.05, 0.15, 0.5, 0.2, 0.1]], np.float32),
    "4x1": np.array([[0.1], [0.2], [0.3], [0.4]], np.float32),
    "2x3": np.array([[0.05, 0.1, 0.15], [0.3, 0.25, 0.15]], np.float32),
    "3x4": np.array([[0.02, 0.05, 0.1, 0.03], [0.1, 0.25, 0.15, 0.05], [0.05, 0.1, 0.07, 0.03]], np.float32),   # an even side over frames
    "7x9": _big_filter(),            # larger than K = 3 and F = 5 of its case
}


def _tg_small(n_fft, hop):
    """(freq_mask_smooth_hz, time_mask_smooth_ms) that give TorchGate a 5 x 3 filter at any size (2.5 bins, 1.5 hops)."""
    return ("tg", 2.5 * SR / (n_fft / 2), 1.5 * hop / SR * 1000)


def _cases():
    out, seed = [], [100]

    def add(name, n_fft, hop, L, **kw):
        seed[0] += 1
        kw.setdefault("seed", seed[0])
        out.append(Case(name, n_fft, hop, L, **kw))

    sweep = []
    for n in (2, 4, 62, 64, 66, 126, 128, 254, 256, 510, 512, 514, 1022, 1024, 1026, 4094, 4096):
        hop = 1 if n <= 4 else n // 4
        for frames in (9, 17):
            name = "nfft%d_f%d" % (n, frames)
            add(name, n, hop, (frames - 1) * hop + hop // 3, Ln=(frames + 4) * hop, filt=_tg_small(n, hop))
            sweep.append(name)
    frames = []
    for F in (1, 2, 7, 8, 9, 15, 16, 17, 33):
        add("F%d" % F, 128, 32, (F - 1) * 32 + 7, Ln=20 * 32, filt=_tg_small(128, 32))
        frames.append("F%d" % F)
    for Fn in (1, 2, 15, 16, 17, 40):
        add("Fn%d" % Fn, 128, 32, 8 * 32 + 5, Ln=(Fn - 1) * 32 + 3, filt=_tg_small(128, 32))
        frames.append("Fn%d" % Fn)
    add("xn_none", 128, 32, 8 * 32 + 5, filt=_tg_small(128, 32))
    add("L_multiple", 128, 32, 8 * 32, Ln=20 * 32, filt=_tg_small(128, 32))
    add("deep_lead", 128, 32, 300, Ln=900, lead=1e-3, filt=_tg_small(128, 32))     # xn's lead-in sits on the 40 dB clamp
    add("quiet_xn", 128, 32, 300, Ln=900, xn_gain=1e-2, filt=_tg_small(128, 32))   # x's maximum is 40 dB above xn's
    frames += ["xn_none", "L_multiple", "deep_lead", "quiet_xn"]
    hopwin = []
    for hop in (1, 32, 33, 50, 64, 96):
        add("hop%d" % hop, 128, hop, 40 if hop == 1 else 300, Ln=60 if hop == 1 else 500, filt=_tg_small(128, hop))
        hopwin.append("hop%d" % hop)
    for wl in (128, 97, 64):
        add("win%d" % wl, 128, wl // 4, 300, Ln=500, win_length=wl, filt=_tg_small(128, wl // 4))
        hopwin.append("win%d" % wl)
    add("hop128_hamming", 128, 128, 700, Ln=900, window="hamming", filt="2x3")
    hopwin.append("hop128_hamming")
    nonstat = []
    for nmm in (1, 2, 19, 20, 21, 50):
        add("nmm%d" % nmm, 128, 32, 16 * 32 + 5, nonstat=True, nmm=nmm, filt=_tg_small(128, 32))
        nonstat.append("nmm%d" % nmm)
    add("temp0.01", 128, 32, 16 * 32 + 5, nonstat=True, temp=0.01, filt=_tg_small(128, 32))
    add("nonstat_silent_row", 128, 32, 16 * 32 + 5, nonstat=True, gains=(1.0, 0.0), filt=_tg_small(128, 32))
    nonstat += ["temp0.01", "nonstat_silent_row"]
    smoothing = []
    add("filt_none", 128, 32, 300, Ln=500)
    add("filt_tg_default", 128, 32, 300, Ln=500, filt=("tg", 500, 50))   # 9 x 25 at 8 kHz: wider than the 10 frames
    smoothing += ["filt_none", "filt_tg_default"]
    for key in ("1x1", "1x5", "4x1", "2x3"):
        add("filt_" + key, 128, 32, 300, Ln=500, filt=key)
        smoothing.append("filt_" + key)
    add("filt_7x9", 4, 1, 4, Ln=9, filt="7x9")
    smoothing.append("filt_7x9")
    props = []
    for n, hop, L in ((128, 32, 300), (4096, 1024, 5000), (2, 1, 9)):
        add("prop0_nfft%d" % n, n, hop, L, Ln=2 * L, prop=0.0)
        props.append("prop0_nfft%d" % n)
    add("prop1", 128, 32, 300, Ln=500, prop=1.0, filt=_tg_small(128, 32))
    props.append("prop1")
    batch = []
    add("b3_gains", 128, 32, 300, Ln=500, gains=(1.0, 1e-3, 3.0), filt=_tg_small(128, 32))
    add("b3_zero_row", 128, 32, 300, Ln=500, gains=(1.0, 0.0, 3.0), filt=_tg_small(128, 32))
    add("b3_nonstat", 128, 32, 300, gains=(1.0, 1e-3, 3.0), nonstat=True, filt=_tg_small(128, 32))
    batch += ["b3_gains", "b3_zero_row", "b3_nonstat"]
    add("filt_3x4", 128, 32, 300, Ln=500, filt="3x4")   # (added last: the seeds above are the fixture's)
    smoothing.append("filt_3x4")
    groups = dict(sweep=sweep, frames=frames, hopwin=hopwin, nonstat=nonstat, smoothing=smoothing, prop=props, batch=batch)
    return out, groups


_ALL, GROUPS = _cases()
CASES = {c.name: c for c in _ALL}
assert len(CASES) == len(_ALL)
NAMES = tuple(CASES)
STATIONARY = tuple(n for n in NAMES if not CASES[n].nonstat)
CLASS_CASES = tuple(n for n in NAMES if CASES[n].is_class)
# the reference fixture (tests/golden/gui_torchgate_edges.npz) holds every case the class can express but the 17-frame runs of the
# sweep at n_fft >= 1022, whose 9-frame twins it has: their fp64 outputs alone would be 350 KB
FIXTURE_CASES = tuple(n for n in CLASS_CASES if not (n.endswith("_f17") and CASES[n].n_fft >= 1022))


def _voice(n, sr, rng, f0, noise):
    """tools/make_golden_gui.py's test signal (as tests/test_gpu_torchgate.py restates it)."""
    t = np.arange(n) / sr
    ph = 2 * np.pi * f0 * (t + 0.002 * np.sin(2 * np.pi * 3.0 * t))
    x = sum((0.3 / h) * np.sin(h * ph + 0.7 * h) for h in range(1, 9))
    return (x + noise * rng.standard_normal(n)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x [B, L] fp32, xn [B, Ln] fp32 or None): harmonics plus noise, each row at its gain; xn with a quieter lead-in."""
    c = CASES[name]
    rng = np.random.default_rng(c.seed)
    xs, xns = [], []
    for r, g in enumerate(c.gains):
        xs.append(np.float32(g) * _voice(c.L, SR, rng, 140.0 + 37.0 * r, 0.02))
        if c.Ln:
            xn = _voice(c.Ln, SR, rng, 140.0 + 37.0 * r, 0.02)
            xn[: c.Ln // 3] *= np.float32(c.lead)
            xns.append(np.float32((g if g else 1.0) * c.xn_gain) * xn)
    x, xn = np.stack(xs), (np.stack(xns) if c.Ln else None)
    x.setflags(write=False)
    if xn is not None:
        xn.setflags(write=False)
    return x, xn


def window(c, variant=None):
    if c.window == "hamming":   # no zero anywhere: hop = n_fft overlap-adds it with nothing
        return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(c.n_fft) / c.n_fft)
    if variant is not None:
        return gate_oracle.hann_window(c.n_fft, c.win_length, variant)
    import torch

    wl = c.n_fft if c.win_length is None else c.win_length   # torch's own samples: what TorchGateHIP hands to the device
    w, left = np.zeros(c.n_fft), (c.n_fft - wl) // 2
    w[left: left + wl] = torch.hann_window(wl, dtype=torch.float64).numpy()
    assert np.abs(w - gate_oracle.hann_window(c.n_fft, c.win_length)).max() <= 1e-15
    return w


def class_kwargs(c):
    """TorchGate's / TorchGateHIP's constructor arguments of a case the class can express."""
    assert c.is_class
    hz, ms = (c.filt[1], c.filt[2]) if c.filt is not None else (None, None)
    return dict(sr=SR, nonstationary=c.nonstat, n_std_thresh_stationary=1.5, n_thresh_nonstationary=1.3, temp_coeff_nonstationary=c.temp,
                n_movemean_nonstationary=c.nmm, prop_decrease=c.prop, n_fft=c.n_fft, win_length=c.win_length, hop_length=c.hop,
                freq_mask_smooth_hz=hz, time_mask_smooth_ms=ms)


@functools.lru_cache(maxsize=None)
def filt(name):
    """The case's smoothing filter [nf, nt] fp32 or None; TorchGate's own through TorchGateHIP's host-side constructor."""
    c = CASES[name]
    if c.filt is None:
        return None
    if isinstance(c.filt, str):
        return RAW_FILTERS[c.filt]
    import rvc_amd

    f = rvc_amd.TorchGateHIP(**class_kwargs(c)).smoothing_filter
    return None if f is None else f[0, 0].numpy().astype(np.float32)


def options(c):
    return dict(nonstationary=c.nonstat, n_std_thresh=1.5, n_thresh_ns=1.3, temp_coeff=c.temp, n_movemean=c.nmm, prop_decrease=c.prop)


def run(name, variant=None, smooth_fp32=False, **over):
    c = CASES[name]
    x, xn = inputs(name)
    wv = variant if variant in gate_oracle.WINDOW_VARIANTS else None
    f = over.pop("filt") if "filt" in over else filt(name)
    kw = dict(options(c), **over)
    return gate_oracle.gate(x, xn, c.n_fft, c.hop, window(c, wv), f, variant=None if wv else variant, smooth_fp32=smooth_fp32, **kw)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The oracle's stages and bars of a case, computed once and shared (read-only)."""
    r = run(name)
    for v in r.values():
        if isinstance(v, np.ndarray) and v.flags.owndata:
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def oracle_x(name):
    """The same case with prop_decrease = 0 and no filter, where Y == X: how the spectrum before masking is checked on the device."""
    return run(name, prop_decrease=0.0, filt=None)


def zero_rows(name):
    return tuple(r for r, g in enumerate(CASES[name].gains) if g == 0.0)


def _a256(v):
    return (v + 255) // 256 * 256


def layout(B, L, Ln, n_fft, hop):
    """csrc/glue.hip's scratch of rvcmi_glue_spectral_gate restated: byte offsets of X, XN, xmax, thresh, mask, frames, and the total.
    Ln = 0 when there is no noise signal, or when the mask is non-stationary (it looks at x alone)."""
    F, Fn, K = 1 + L // hop, (1 + Ln // hop if Ln > 0 else 0), n_fft // 2 + 1
    off, o = {}, 0
    for key, nbytes in (("X", B * F * K * 16), ("XN", B * Fn * K * 16), ("xmax", B * K * 8), ("thresh", B * K * 8), ("mask", B * F * K * 4),
                        ("frames", B * F * n_fft * 8)):
        off[key] = o
        o += _a256(nbytes)
    off["total"] = o
    return off


def ratio(got, want, bar):
    """max |got - want| / bar over the entries (0 / 0 counts as 0; a NaN or inf must sit where the oracle's does)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    if not np.array_equal(np.isfinite(got), fin) or not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf")
    if not fin.any():
        return 0.0
    e = np.abs(got[fin] - want[fin])
    b = np.broadcast_to(bar, want.shape)[fin]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(e == 0, 0.0, e / b)
    return float(q.max())
