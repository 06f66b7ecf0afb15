"""The edge cases of the device-resident glue (csrc/glue_kernels.hpp, csrc/glue.hip) for tests/test_cpu_glue.py (the oracle alone, and the
conditions under which a device may be held to it) and tests/test_gpu_glue_edges.py / tools/glue_parity.py (the device against the oracle).
Everything here is seeded and runs on the CPU; the oracle results are computed once per process.

Bars (all taken from tests/test_gpu_glue.py and tests/test_gpu_rt_block.py, none new): pitch identical, pitchf 1e-6 relative with equal zero
sets; expand / protect, int16 scaling and the SOLA stitch bit-exact; change_rms 2e-6 and envelope_mix 1e-6 relative (atol 1e-9); the
resampler 5e-6 * max(1, max |want|); the phase vocoder no worse than the reference's own fp32 run, and 2e-8 RMS / 1e-7 max-abs up to
n = 1920, times n / 1920 above (the terms per output sample, and with them the accumulated rounding of the fp32 cosine, grow linearly in n)."""
import functools
import itertools
import math

import numpy as np
import torch

from conftest import load_golden
from oracle import glue_oracle

F0_RTOL = 1e-6
CHANGE_RMS_TOL = dict(rtol=2e-6, atol=1e-9)
ENVELOPE_TOL = dict(rtol=1e-6, atol=1e-9)
RESAMPLE_REL = 5e-6
MEL_MARGIN = 1e-9   # the device's fp64 log / pow may move the mel value by a few fp64 ulps (1e-13 at 255): four orders above that
HZ_MARGIN = 1e-9    # relative distance of a decoded Hz from the two thresholds of the chain (== 10 -> unvoiced, < 0.001 -> NaN)


def fades(n):
    fade_in = torch.sin(0.5 * np.pi * torch.linspace(0.0, 1.0, steps=n, dtype=torch.float32)) ** 2  # gui.py:841-855
    return fade_in, 1 - fade_in


# ---- 1. the f0 chain -----------------------------------------------------------------------------------------------------------------
PATTERN_MAX_N = 7
PATTERN_BINS = (60, 97, 131, 158, 189, 214, 240)    # frame i's salience peak: 63 .. 507 Hz, all different
PATTERN_PEAK = 0.9
PATTERN_KEYS = (0, -5.5)
POST_HZ = (61.7, 97.3, 110.0, 150.9, 220.5, 300.1, 440.0)   # frame i's f0 for f0_post (no decode in front)
POST_KEYS = (-12, 0, 5, 1.5)


def pattern_p_lens(n):
    return sorted(p for p in {1, 2, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1, 3 * n + 2} if p > 0)


def patterns():
    """(n, mask) for every voiced / unvoiced pattern of 1 .. 7 frames; bit i of mask: frame i is voiced."""
    return [(n, m) for n in range(1, PATTERN_MAX_N + 1) for m in range(1 << n)]


def pattern_salience(n, mask):
    """Zero except one peak of 0.9 per voiced frame, in the bin that decodes to that frame's pitch."""
    sal = np.zeros((n, 360), np.float32)
    for i in range(n):
        if (mask >> i) & 1:
            sal[i, PATTERN_BINS[i]] = np.float32(PATTERN_PEAK)
    return sal


def pattern_f0(n, mask):
    return np.array([POST_HZ[i] if (mask >> i) & 1 else 0.0 for i in range(n)], np.float64)


@functools.lru_cache(maxsize=None)
def rmvpe_pattern_cases():
    return tuple((n, m, p, k) for n, m in patterns() for p in pattern_p_lens(n) for k in PATTERN_KEYS)


@functools.lru_cache(maxsize=None)
def post_pattern_cases():
    return tuple((n, m, k) for n, m in patterns() for k in POST_KEYS)


def chain_parts(sal, p_len, key, thred=0.03):
    """The oracle's chain step by step: decoded Hz, mel before ``rint``, pitch, pitchf (for the conditions below)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        dec = glue_oracle.rmvpe_decode(sal, thred)
        f0 = glue_oracle.interpolate_f0(glue_oracle.resize_f0(dec, p_len))
        mel, f0k = glue_oracle.post_process_mel(f0, key)
    return dec, mel, np.rint(mel).astype(np.int64)[:p_len], f0k[:p_len].astype(np.float32)


def oracle_rmvpe_f0(sal, p_len, key):
    with np.errstate(invalid="ignore", divide="ignore"):
        return glue_oracle.rmvpe_f0(sal, p_len, key, 0.03)


def oracle_f0_post(f0, key):
    mel, f0k = glue_oracle.post_process_mel(np.array(f0, np.float64), key)
    pitch, _ = glue_oracle.post_process(np.array(f0, np.float64), key)
    return mel, pitch.astype(np.int64), f0k.astype(np.float32)


def mel_margin(mel):
    """Distance of the mel values from the nearest .5 boundary of ``rint`` (the clamped ends 1 and 255 are 0.5 away)."""
    mel = np.asarray(mel, np.float64)
    return float(np.abs(mel - np.floor(mel) - 0.5).min()) if mel.size else 0.5


def hz_margin(dec):
    """Relative distance of the voiced decoded values from 10.0 (-> 0) and 0.001 (-> NaN in _resize_f0).  A value that IS 0 came from
    cents == 0, where 2 ** 0 is exactly 1 on any conforming pow."""
    v = np.asarray(dec, np.float64)
    v = v[v != 0]
    return float(min(np.abs(v / 10.0 - 1).min(), np.abs(v / 0.001 - 1).min())) if v.size else 1.0


@functools.lru_cache(maxsize=None)
def rmvpe_pattern_oracle():
    """(pitch, pitchf) of ``glue_oracle.rmvpe_f0`` per case of rmvpe_pattern_cases()."""
    return tuple(oracle_rmvpe_f0(pattern_salience(n, m), p, k) for n, m, p, k in rmvpe_pattern_cases())


@functools.lru_cache(maxsize=None)
def post_pattern_oracle():
    return tuple(oracle_f0_post(pattern_f0(n, m), k)[1:] for n, m, k in post_pattern_cases())


# Lane l of the decode's wave reads bins l, l + 64, ...: 3|67 and 10|74 tie INSIDE a lane; 3|68 ties across lanes with the first maximum in
# the lower lane, 10|67 with the first maximum in the higher lane (the butterfly must compare indices, not lanes).
DECODE_EDGE_NS = (13, 11, 1, 2, 3, 5)
DECODE_EDGE_ROWS = ("peak@0", "peak@3", "peak@356", "peak@359", "tie 3|67 (one lane)", "tie 10|74 (one lane)", "all 0.2", "all 0",
                    "max == 0.03", "max == nextafter(0.03)", "ordinary", "tie 3|68 (two lanes)", "tie 10|67 (two lanes, first in the higher)")


@functools.lru_cache(maxsize=None)
def decode_edge_salience():
    """13 frames, and its first 11 (neither a multiple of the 4 frames per block).  The bump rows stand on a noise floor below the threshold, so a window that
    reads past either end of a row, or into the neighbouring row, reads something that is not zero."""
    rng = np.random.default_rng(360)
    sal = (rng.random((13, 360), dtype=np.float32) * np.float32(0.02)).astype(np.float32)

    def bump(row, centre, height=0.9):
        for w in range(-6, 7):
            if 0 <= centre + w < 360:
                sal[row, centre + w] += np.float32(height * math.exp(-0.5 * (w / 2.0) ** 2))

    for row, centre in enumerate((0, 3, 356, 359)):
        bump(row, centre)
    sal[4, 3] = sal[4, 67] = np.float32(0.5)
    sal[5, 10] = sal[5, 74] = np.float32(0.5)
    sal[6, :] = np.float32(0.2)
    sal[7, :] = 0
    sal[8, :] *= np.float32(0.5)
    sal[8, 100] = np.float32(0.03)
    sal[9, :] *= np.float32(0.5)
    sal[9, 100] = np.nextafter(np.float32(0.03), np.float32(1))
    bump(10, 150)
    sal[11, 3] = sal[11, 68] = np.float32(0.5)
    sal[12, 10] = sal[12, 67] = np.float32(0.5)
    sal.setflags(write=False)
    return sal


THRESHOLD_N = 10240    # (n + p_len) * 8 and 2 n * 8 bytes == 160 KiB: the last size whose work arrays live in LDS


@functools.lru_cache(maxsize=None)
def threshold_salience():
    """Synthetic voiced runs as in test_f0_chain_has_no_length_limit, THRESHOLD_N frames."""
    rng = np.random.default_rng(10240)
    n = THRESHOLD_N
    sal = (rng.random((n, 360), dtype=np.float32) * 0.02).astype(np.float32)
    centre = (150 + 100 * np.sin(np.arange(n) / 40.0)).astype(int)
    voiced = (np.arange(n) % 300) >= 45
    voiced[-200:] = False
    for w_ in range(-4, 5):
        sal[np.arange(n)[voiced], centre[voiced] + w_] += np.float32(0.9 * np.exp(-0.5 * (w_ / 2.0) ** 2))
    sal.setflags(write=False)
    return sal


THRESHOLD_RMVPE = ((THRESHOLD_N, THRESHOLD_N, 3), (THRESHOLD_N, THRESHOLD_N + 1, 3))   # (n, p_len, key): last in LDS, first in global
THRESHOLD_POST = ((THRESHOLD_N, 3), (THRESHOLD_N + 1, 3))                              # (n, key): both clamps of the mel scale are reached


@functools.lru_cache(maxsize=None)
def threshold_f0(n):
    rng = np.random.default_rng(n)
    f0 = rng.uniform(40, 1300, n)
    f0[rng.random(n) < 0.2] = 0.0
    f0.setflags(write=False)
    return f0


@functools.lru_cache(maxsize=None)
def threshold_oracle():
    sal = threshold_salience()
    return (tuple(chain_parts(sal[:n], p, k) for n, p, k in THRESHOLD_RMVPE), tuple(oracle_f0_post(threshold_f0(n), k) for n, k in THRESHOLD_POST))


# ---- 2. expand + protect -------------------------------------------------------------------------------------------------------------
PROTECT_PITCHF = (0.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0))), 1.0, 220.0)
PROTECTS = (0.0, 0.33, math.nextafter(0.5, 0.0), 0.5)   # the last but one: below 0.5 as a double (the mix runs), 0.5 as a float32


@functools.lru_cache(maxsize=None)
def expand_cases():
    """(d, nq, p_len, protect, feats [1, nq, d], pitchf [1, 2 nq]); every pitchf value lands on frame 0 of some case."""
    out = []
    g = torch.Generator().manual_seed(255)
    for d, nq in itertools.product((1, 255, 256, 257, 768), (1, 2, 5)):
        for p_len, protect in itertools.product(sorted({1, 2 * nq - 1, 2 * nq}), PROTECTS):
            feats = 0.5 * torch.randn(1, nq, d, generator=g)
            pitchf = torch.tensor([[PROTECT_PITCHF[(t + len(out)) % 5] for t in range(2 * nq)]], dtype=torch.float32)
            out.append((d, nq, p_len, protect, feats, pitchf))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expand_oracle():
    return tuple(glue_oracle.expand_protect(f, f, pf, protect, p_len) for _, _, p_len, protect, f, pf in expand_cases())


# ---- 3. int16 scaling ----------------------------------------------------------------------------------------------------------------
INT16_NS = (1, 255, 256, 257, 65535, 65536, 65537, 66305)   # 256 blocks x 256 threads = 65536 per grid stride
INT16_KINDS = ("tail -2.5", "zeros", "peak float32(0.99)", "peak 0.5")


@functools.lru_cache(maxsize=None)
def int16_cases():
    """(n, kind, audio).  "tail": the largest magnitude, -2.5, is the LAST sample alone; every other sample is within +-0.1."""
    out = []
    for n in INT16_NS:
        rng = np.random.default_rng(n)
        base = rng.uniform(-0.1, 0.1, n).astype(np.float32)
        for kind in INT16_KINDS:
            a = base.copy()
            if kind == "tail -2.5":
                a[n - 1] = np.float32(-2.5)
            elif kind == "zeros":
                a[:] = 0
            elif kind == "peak float32(0.99)":
                a[n // 2] = np.float32(0.99)
            else:
                a[n // 2] = np.float32(0.5)
            a.setflags(write=False)
            out.append((n, kind, a))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def int16_oracle():
    return tuple(glue_oracle.scale_int16_range(a) for _, _, a in int16_cases())


# ---- 4. SOLA -------------------------------------------------------------------------------------------------------------------------
SOLA_TIES = ((7, 300, 600, 5, 500), (256, 300, 600, 40, 500), (7, 300, 0, 0, 500), (7, 300, 255, 5, 500), (7, 300, 256, 5, 500))
SOLA_LDS_FIT = (7, 19000, 400, 5, 100)      # (2 * 19000 + 400) * 4 bytes == 150 KiB: the largest geometry served
SOLA_LDS_OVER = (7, 19000, 401, 5, 100)     # four bytes more: refused
ERR_NOMEM = -4                              # include/rvcmi.h


def integer_pattern(P):
    """One period of integers in [-3, 3]; P is its shortest period (asserted by the CPU test through shortest_period)."""
    return torch.randint(-3, 4, (P,), generator=torch.Generator().manual_seed(P)).float()


def shortest_period(pat):
    P = int(pat.numel())
    return next(p for p in range(1, P + 1) if torch.equal(pat, torch.roll(pat, p)))


def sola_tie_case(P, Lb, Ls, o0, block):
    """The chunk repeats an integer pattern of period P and the buffer is the chunk at o0: every product and sum is an integer below
    2^24, exact in fp32 and fp64 in any order, so offsets o0, o0 + P, ... give the SAME quotient and the first of them must win."""
    n = Ls + block + Lb
    x = integer_pattern(P)[torch.arange(n) % P].clone()
    return dict(name="ties P%d Lb%d Ls%d" % (P, Lb, Ls), x=x, buf=x[o0:o0 + Lb].clone(), Lb=Lb, Ls=Ls, block=block, expect=o0)


@functools.lru_cache(maxsize=None)
def sola_cases():
    out = [sola_tie_case(*c) for c in SOLA_TIES]
    g = torch.Generator().manual_seed(1057)
    Lb, Ls, block = 300, 600, 500
    out.append(dict(name="zero chunk", x=torch.zeros(Ls + block + Lb), buf=torch.randn(Lb, generator=g), Lb=Lb, Ls=Ls, block=block, expect=0))
    out.append(dict(name="zero buffer", x=0.3 * torch.randn(Ls + block + Lb, generator=g), buf=torch.zeros(Lb), Lb=Lb, Ls=Ls, block=block,
                    expect=None))
    Lb, Ls, block = 300, 100, 100   # block < Lb: the new tail starts inside the cross-faded part
    x = 0.3 * torch.randn(Ls + block + Lb, generator=g)
    out.append(dict(name="block < Lb", x=x, buf=0.9 * x[37:37 + Lb] + 0.01 * torch.randn(Lb, generator=g), Lb=Lb, Ls=Ls, block=block, expect=37))
    out.append(dict(name="Lb = 1", x=0.3 * torch.randn(50 + 20 + 1, generator=g), buf=torch.tensor([0.25]), Lb=1, Ls=50, block=20, expect=None))
    out.append(dict(sola_tie_case(*SOLA_LDS_FIT), name="150 KiB of LDS"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def sola_oracle():
    """(block, new buffer, offset) per case of sola_cases()."""
    return tuple(glue_oracle.sola(c["x"], c["buf"], *fades(c["Lb"]), c["block"], c["Ls"]) for c in sola_cases())


# ---- 5. the envelope mixes -----------------------------------------------------------------------------------------------------------
MIX_RATES = (0.0, 0.25, 1.0)
CHANGE_RMS_GEOM = ((16, 7, 48, 21), (16, 8, 48, 24), (601, 2000, 1803, 6001), (100, 1000, 37, 333))   # (sr1, n1, sr2, n2)
ENVELOPE_GEOM = ((400, 12001), (441, 6000), (400, 399), (400, 400), (1, 300))                        # (zc, n)


def _with_silence(rng, n, amp, lo, hi):
    x = (amp * rng.standard_normal(n)).astype(np.float32)
    x[int(lo * n): max(int(hi * n), int(lo * n) + 1)] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def change_rms_cases():
    """(sr1, n1, sr2, n2, rate, data1, data2): a silent stretch in each signal (long enough for a frame RMS of zero where the case has
    more than two frames) and a very quiet one in data2 (the 1e-6 floor)."""
    out = []
    for sr1, n1, sr2, n2 in CHANGE_RMS_GEOM:
        rng = np.random.default_rng(sr1 * 1000 + n1)
        d1 = _with_silence(rng, n1, 0.3, 0.2, 0.7)
        d2 = _with_silence(rng, n2, 0.2, 0.5, 0.9)
        d2[: n2 // 8] *= np.float32(1e-7)
        for a in (d1, d2):
            a.setflags(write=False)
        out.extend((sr1, n1, sr2, n2, rate, d1, d2) for rate in MIX_RATES)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def change_rms_oracle():
    return tuple(glue_oracle.change_rms(d1, sr1, d2.copy(), sr2, rate) for sr1, _, sr2, _, rate, d1, d2 in change_rms_cases())


@functools.lru_cache(maxsize=None)
def envelope_cases():
    """(zc, n, rate, input, wav)."""
    out = []
    for zc, n in ENVELOPE_GEOM:
        rng = np.random.default_rng(zc * 100003 + n)
        inp = _with_silence(rng, n + 37, 0.3, 0.1, 0.45)
        wav = _with_silence(rng, n, 0.2, 0.5, 0.85)
        wav[: n // 8] *= np.float32(1e-4)
        for a in (inp, wav):
            a.setflags(write=False)
        out.extend((zc, n, rate, inp, wav) for rate in MIX_RATES)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def envelope_oracle():
    return tuple(glue_oracle.envelope_mix(inp, wav, zc, rate) for zc, _, rate, inp, wav in envelope_cases())


# ---- 6. the resampler ----------------------------------------------------------------------------------------------------------------
# 423 -> 400 has a filter half-width of 7 input samples; 1000 samples leave the last block of 256 outputs, and the last group of
# `new` output phases, partial for both 538 -> 480 (893 out) and 357 -> 400 (1121 out)
RESAMPLE_GEOM = ((423, 400, 1), (423, 400, 3), (423, 400, 6), (538, 480, 1000), (357, 400, 1000))


@functools.lru_cache(maxsize=None)
def resample_cases():
    out = []
    for orig, new, n in RESAMPLE_GEOM:
        x = np.random.default_rng(orig + n).standard_normal(n).astype(np.float32)
        out.append((orig, new, n, x, glue_oracle.sinc_resample(x, orig, new)))
    return tuple(out)


# ---- 7. the phase vocoder ------------------------------------------------------------------------------------------------------------
PV_EDGE_SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096)
PV_CASES = ("harm", "zero_a", "same")
PV_MAX_N = 4096


def rms(x):
    return float(np.sqrt(np.mean(np.asarray(x, np.float64) ** 2)))


def pv_bars(n):
    s = max(1.0, n / 1920.0)
    return 2e-8 * s, 1e-7 * s


def pv_case(n, case):
    """-> (a, b, fade_out, fade_in, ref32 as float64, ref64) of tests/golden/gui_phase_vocoder.npz (tools/make_golden_gui.py)."""
    d = pv_golden()
    k = "n%d_%s" % (n, case)
    return d[k + "_a"], d[k + "_b"], d["n%d_fade_out" % n], d["n%d_fade_in" % n], d[k + "_ref32"].astype(np.float64), d[k + "_ref64"]


@functools.lru_cache(maxsize=None)
def pv_golden():
    return load_golden("gui_phase_vocoder")


def pv_errors(got, r32, r64):
    """(device RMS, device max-abs, reference-fp32 RMS, reference-fp32 max-abs) against the reference's function in fp64."""
    e_dev, e_32 = np.asarray(got, np.float64) - r64, r32 - r64
    return rms(e_dev), float(np.abs(e_dev).max()), rms(e_32), float(np.abs(e_32).max())


def pv_check(n, got, r32, r64):
    """The bars of section 7: the relative criteria wherever the reference's fp32 run has an error at all, the absolute ones always."""
    r_dev, m_dev, r_32, m_32 = pv_errors(got, r32, r64)
    bar_rms, bar_max = pv_bars(n)
    assert np.isfinite(got).all()
    if r_32 > 0:
        assert r_dev <= r_32, "n %d: rms %.2e vs the reference's fp32 %.2e" % (n, r_dev, r_32)
        assert m_dev <= 1.5 * m_32, "n %d: max %.2e vs %.2e" % (n, m_dev, m_32)
    assert r_dev <= bar_rms and m_dev <= bar_max, "n %d: rms %.2e (bar %.2e), max %.2e (bar %.2e)" % (n, r_dev, bar_rms, m_dev, bar_max)
