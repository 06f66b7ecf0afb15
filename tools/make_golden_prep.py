"""Fixtures of the device input preparation (``glue.filtfilt``: scipy.signal.filtfilt with the pipeline's 48 Hz high-pass,
infer/modules/vc/pipeline.py:23,221) -> tests/golden/prep_filtfilt.npz.

What is stored per case: the EXACT result of the forward-backward recurrence at a fixed set of positions -- the same direct form II
transposed recurrence, the same fp64 coefficients and ``lfilter_zi`` values, the same odd extension, evaluated in ``np.longdouble``
(asserted to carry a 64-bit mantissa: x87 extended precision, 2048 times finer than fp64) and rounded to fp64 once at the end --
plus the sha256 of the input.  The inputs are RECIPES (``make_input``): ``default_rng(seed).integers`` and exact fp64 operations
only (an integer parabola for the tone, integer noise, powers of two), so a test regenerates them bit for bit on any numpy and
checks the hash first.  scipy's own result is NOT stored: the tests compute it and compare its deviation from the exact values with
the device's.

The script also evaluates a CPU model of the device scheme (``lane_model``: independent lanes of ``FILT_LANE`` outputs, each warmed up
over ``filt_warmup`` samples from ``zi * in[start]``, every lane scipy's own ``lfilter``) and prints, per case, the ratio
max|model - exact| / max|scipy - exact| and, for the long cases, whether the quiet-point search finds the same cuts on the model's
signal as on scipy's.  Nothing of the model is stored.

    python tools/make_golden_prep.py
"""
import hashlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SR = 16000
STRIDE, EDGE = 61, 2000  # compared positions: the first and last EDGE samples and every STRIDE-th in between

# name: (seed, samples, dtype, kind)   kinds: plain | zeros (a stretch of exact zeros) | int16 (quantised to the int16 grid) |
# envelope (loud and quiet quarter-seconds, so that the quiet-point search has something to find)
CASES = {
    "tone_noise_dc_5s": (11, 5 * SR + 123, "float64", "plain"),
    "zeros_stretch_7s": (12, 7 * SR + 1, "float32", "zeros"),
    "int16_quantised_4s": (13, 4 * SR + 77, "float32", "int16"),
    "envelope_80s": (14, 80 * SR, "float32", "envelope"),
    "int16_envelope_72s": (15, 72 * SR + 5, "float64", "int16_envelope"),
}
CUT_GEOMETRY = (160, 38 * SR, 6 * SR, 41 * SR)  # window, t_center, t_query, t_max: configs/config.py x_center 38, x_query 6, x_max 41


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def make_input(name: str) -> np.ndarray:
    """Tone + noise + DC offset from integers alone: a 220 Hz parabolic 'sine' (16-bit phase, increment 901; peak 0.25), uniform
    integer noise (peak 0.125) and the offset 1/16, all on the 2^-30 grid, so every step is exact in fp64.  The variants zero a
    stretch, apply a power-of-two envelope per quarter second, round to the int16 grid, and finally cast to the case's dtype."""
    seed, n, dtype, kind = CASES[name]
    rng = np.random.default_rng(seed)
    k = np.arange(n, dtype=np.int64)
    p = (k * 901) & 0xFFFF
    h = 32768
    tone = np.where(p < h, p * (h - p), -(p - h) * (2 * h - p))               # |.| <= 2^28
    noise = rng.integers(-(1 << 15), 1 << 15, size=n, dtype=np.int64) << 12   # |.| <  2^27
    v = (tone + noise).astype(np.float64)
    if "envelope" in kind:
        nb = (n + 3999) // 4000
        shift = rng.integers(0, 8, size=nb)
        shift[rng.integers(0, 4, size=nb) == 0] = 12                          # a quiet block: 2^-12 of full scale
        v = np.ldexp(v, -np.repeat(shift, 4000)[:n])
    x = np.ldexp(v, -30) + 0.0625
    if kind == "zeros":
        x[n // 3: n // 3 + 9000] = 0.0
    if "int16" in kind:
        x = np.rint(x * 32768.0) / 32768.0
    return np.ascontiguousarray(x.astype(dtype))


def positions(n: int) -> np.ndarray:
    return np.concatenate([np.arange(0, EDGE), np.arange(EDGE, n - EDGE, STRIDE), np.arange(n - EDGE, n)]).astype(np.int64)


def coefficients():
    from scipy import signal

    return signal.butter(N=5, Wn=48, btype="high", fs=16000)  # pipeline.py:23


def odd_ext(x: np.ndarray, padlen: int) -> np.ndarray:
    """scipy's odd extension, in the dtype of ``x`` as scipy evaluates it."""
    return np.concatenate((2 * x[0] - x[padlen:0:-1], x, 2 * x[-1] - x[-2:-(padlen + 2):-1]))


def exact_lfilter(b, a, zi, x):
    """Direct form II transposed in np.longdouble, state ``zi * x[0]``."""
    ld = np.longdouble
    nb = len(b)
    b = [ld(v) for v in b]
    a = [ld(v) for v in a]
    z = [ld(v) * ld(x[0]) for v in zi]
    y = np.empty(len(x), dtype=ld)
    xs = x.astype(ld)
    for i in range(len(xs)):
        xv = xs[i]
        yv = b[0] * xv + z[0]
        for k in range(nb - 2):
            z[k] = (b[k + 1] * xv + z[k + 1]) - a[k + 1] * yv
        z[nb - 2] = b[nb - 1] * xv - a[nb - 1] * yv
        y[i] = yv
    return y


def exact_filtfilt(b, a, x):
    from scipy import signal

    assert np.finfo(np.longdouble).nmant == 63, "np.longdouble is not the 80-bit extended type here: the fixture needs a 64-bit mantissa"
    assert a[0] == 1.0
    padlen = 3 * max(len(a), len(b))
    zi = signal.lfilter_zi(b, a)
    ext = odd_ext(x, padlen)
    y1 = exact_lfilter(b, a, zi, ext)
    y2 = exact_lfilter(b, a, zi, y1[::-1])
    return y2[::-1][padlen:-padlen].astype(np.float64)


def lane_model(b, a, x, warm, lane):
    """The device scheme on the CPU: per pass, lane j gives outputs [j lane, (j + 1) lane) from a run that starts ``warm`` samples
    earlier (or at sample 0) in the state ``zi * in[start]``; every run is scipy's lfilter, i.e. the kernel's arithmetic."""
    from scipy import signal

    padlen = 3 * max(len(a), len(b))
    zi = signal.lfilter_zi(b, a)

    def one_pass(v):
        out = np.empty(len(v), dtype=np.float64)
        for p0 in range(0, len(v), lane):
            s = max(0, p0 - warm)
            p1 = min(p0 + lane, len(v))
            out[p0:p1] = signal.lfilter(b, a, v[s:p1], zi=zi * v[s])[0][p0 - s:]
        return out

    y1 = one_pass(odd_ext(x, padlen))
    return one_pass(y1[::-1])[::-1][padlen:-padlen]


def host_cuts(audio, geometry=CUT_GEOMETRY):
    sys.path.insert(0, ROOT)
    import rvc_amd.pipeline as rp

    w, tc, tq, tm = geometry
    state = types.SimpleNamespace(window=w, t_center=tc, t_query=tq, t_max=tm)
    return rp._cut_points(state, audio, np.pad(audio, (w // 2, w // 2), mode="reflect"))


def main():
    from scipy import signal

    sys.path.insert(0, ROOT)
    from rvc_amd import glue

    b, a = coefficients()
    warm = glue.filt_warmup(a)
    out = {"names": np.array(list(CASES)), "b": b, "a": a}
    for name, (seed, n, dtype, kind) in CASES.items():
        x = make_input(name)
        assert x.shape == (n,) and str(x.dtype) == dtype
        exact = exact_filtfilt(b, a, x)
        idx = positions(n)
        out[name + "_exact"] = exact[idx]
        out[name + "_input_sha256"] = sha(x)
        sp = signal.filtfilt(b, a, x)
        model = lane_model(b, a, x, warm, glue.FILT_LANE)
        e_sp, e_model = np.abs(sp - exact)[idx].max(), np.abs(model - exact)[idx].max()
        line = "%-20s n %8d %s  peak %.3f  scipy-exact %.3e  model-exact %.3e  ratio %.2f" % (name, n, dtype, np.abs(x).max(), e_sp, e_model, e_model / e_sp)
        if n > CUT_GEOMETRY[3]:
            c_sp, c_model = host_cuts(sp), host_cuts(model)
            out[name + "_cuts"] = np.array(c_sp, np.int64)
            line += "  cuts %s model %s" % (c_sp, "same" if c_model == c_sp else c_model)
        print(line, flush=True)
    path = os.path.join(GOLD, "prep_filtfilt.npz")
    np.savez_compressed(path, **out)
    print("prep_filtfilt.npz %d KB" % (os.path.getsize(path) // 1024))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
