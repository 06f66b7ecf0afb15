"""TEST INFRASTRUCTURE ONLY -- the generator's excitation and realtime resampling, restated rounding by rounding (numpy, CPU).

What is in front of the generator's layers (csrc/nsf_source_kernels.hpp: k_phase_scan, k_sine_source, k_interp_linear, k_interp_linear_ragged;
reference: rvc/layers/generators.py:148-194, rvc/layers/nsf.py:57-61,155-162) has no fp64 "truth" to be held to: the reference computes it in float32,
and the float32 steps ARE the semantics (an fp32 phase of magnitude 0.49 * T, an fp32 source index of magnitude T * upp).  So the oracles here follow
the float32 chain step by step and leave open only what no IEEE rule fixes:

  ``phase``              nothing is open.  Every increment is a multiple of 2^-25, every prefix sum an exact integer in those units below 2^53, so the
                         float64 sums of torch's CPU cumsum and of the kernel's partitioned scan are exact in ANY order and the one rounding to float32
                         is the same everywhere.  The result is the phase bit for bit.
  ``har_interval``       sinf and tanhf are library functions: each may be ``L_SIN`` / ``L_TANH`` ulp off the correctly rounded value.  Everything between
                         them is float32 arithmetic with one rounding per operation (the kernel's ``fp contract(off)`` region) and monotone in the sine.
  ``interp_admissible``  the source index ``scale * (o + 0.5) - 0.5`` is float32 arithmetic that a compiler may or may not contract into one fma: both
                         roundings are admitted, and the three operations of ``l0 * r[i0] + l1 * r[i1]`` may round separately or fused.

``variant=`` names a WRONG excitation / interpolation (tests/test_cpu_source.py: the bars must reject each).
"""
from __future__ import annotations

import collections

import numpy as np

f32, f64 = np.float32, np.float64

# The liberty granted to the device's (and the reference's) sinf and tanhf, in float32 ulps of the correctly rounded result.  4 ulp is what the project
# already grants tanhf (tests/nsf_cases.py: "tanh moved by +-4 ulp") and the OpenCL full-profile bound for sin, which the device library follows.
# It is a property of the libraries, not of a device run: it is not to be widened to make one pass.
L_SIN = 4
L_TANH = 4

TWO_PI_F32 = f32(6.2831855)  # float32(2 * pi): what ``2 * torch.pi * rad`` multiplies a float32 tensor by, and the kernel's literal
UNIT = 2.0 ** -25            # every phase increment is a multiple of this (see ``increments``)

PHASE_VARIANTS = ("seq_f32", "fused_factor", "shift_frame", "no_wrap")
SOURCE_VARIANTS = ("n_from_0", "uv_ge", "amp_swapped", "two_pi_f64")
INTERP_VARIANTS = ("align_corners", "no_half_pixel", "no_clamp_low", "i1_unclamped")


def ulp32(x):
    """The float32 ulp of the binade of |x| (float64 in, float64 out; 2^-149 at and below the subnormals)"""
    x = np.abs(np.asarray(x, dtype=f64))
    _, e = np.frexp(x)  # |x| in [2^(e-1), 2^e)
    return np.where(x == 0, 2.0 ** -149, np.ldexp(1.0, np.maximum(e - 24, -149)))


# ---- phase ---------------------------------------------------------------------------------------------------------------------------------

def increments(f0, sr, upp, variant=None):
    """w[b][t] = fmod(f0 / sr * upp + 0.5, 1) - 0.5 for EVERY frame, in float32 with one rounding per operation (k_phase_scan; generators.py:154-156)"""
    f = np.asarray(f0, dtype=f32)
    if variant == "fused_factor":
        rad = f * (f32(upp) / f32(sr))
    else:
        rad = (f / f32(sr)) * f32(upp)
    if variant == "no_wrap":
        return rad
    return np.fmod(rad + f32(0.5), f32(1.0)) - f32(0.5)


def is_on_grid(w):
    """Is every increment a multiple of 2^-25?  (The premise of ``phase``: rad + 0.5 >= 0.5 has an ulp of 2^-24 or more, fmod and the subtraction are exact.)"""
    k = np.asarray(w, dtype=f64) / UNIT
    return bool(np.all(k == np.rint(k)) and np.all(np.abs(k) <= 2.0 ** 25))


def phase(f0, sr, upp, variant=None):
    """f0 [B, T] -> the float32 phase per frame [B, T]: phase[t] = fmod(float32(sum_{tau < t} w[tau]), 1), phase[0] = 0"""
    w = increments(f0, sr, upp, variant)
    B, T = w.shape
    if variant == "seq_f32":  # a float32 accumulator, frame by frame
        pref = np.zeros((B, T), dtype=f32)
        for t in range(1, T):
            pref[:, t] = pref[:, t - 1] + w[:, t - 1]
        return np.fmod(pref, f32(1.0))
    if variant == "no_wrap":  # (off the 2^-25 grid: accumulated in float64 as torch would)
        pref = np.concatenate([np.zeros((B, 1)), np.cumsum(w[:, :-1].astype(f64), axis=1)], axis=1)
        return np.fmod(pref.astype(f32), f32(1.0))
    assert is_on_grid(w), "a phase increment is no multiple of 2^-25: the prefix sums are not order-independent"
    k = np.rint(w.astype(f64) / UNIT).astype(np.int64)
    if variant == "shift_frame":  # frame t already carries its own increment
        pref = np.cumsum(k, axis=1)
    else:
        pref = np.concatenate([np.zeros((B, 1), dtype=np.int64), np.cumsum(k[:, :-1], axis=1)], axis=1)
    assert np.all(np.abs(pref) < 2 ** 53)
    return np.fmod((pref.astype(f64) * UNIT).astype(f32), f32(1.0))  # int64 -> float64 and the scaling are exact; ONE rounding, to nearest even


def phase_kernel_partition(f0, sr, upp, threads=256, wave=64):
    """k_phase_scan's own order of summation, step by step in float64: ``per = ceil((T - 1) / 256)`` frames per thread summed in sequence, an inclusive
    scan over the 64 lanes of a wave in log steps, the waves' totals added in wave order, then each thread's frames again in sequence."""
    w = increments(f0, sr, upp).astype(f64)
    B, T = w.shape
    n = T - 1
    per = (n + threads - 1) // threads
    ph = np.zeros((B, T), dtype=f32)
    for b in range(B):
        beg = [min(n, t * per) for t in range(threads)]
        end = [min(n, beg[t] + per) for t in range(threads)]
        local = np.zeros(threads)
        for t in range(threads):
            for i in range(beg[t], end[t]):
                local[t] += w[b, i]
        incl = local.copy()
        off = 1
        while off < wave:
            prev = incl.copy()
            for t in range(threads):
                if t % wave >= off:
                    incl[t] = prev[t] + prev[t - off]
            off <<= 1
        wsum = [incl[v * wave + wave - 1] for v in range(threads // wave)]
        for t in range(threads):
            run = incl[t] - local[t]
            for v in range(t // wave):
                run += wsum[v]
            for i in range(beg[t], end[t]):
                run += w[b, i]
                ph[b, i + 1] = np.fmod(f32(run), f32(1.0))
    return ph


# ---- sine source + tanh(Linear(1, 1)) ------------------------------------------------------------------------------------------------------

def har_interval(f0, noise, sr, upp, lw, lb, L_sin=L_SIN, L_tanh=L_TANH, variant=None):
    """f0 [B, T], noise [B, T * upp] or None -> (lo, hi, centre), float64 [B, 1, T * upp]: every float32 ``har`` that k_sine_source's chain can give with
    sinf within ``L_sin`` and tanhf within ``L_tanh`` ulp lies in [lo, hi]; ``centre`` is the chain at the correctly rounded sine, with tanh left in float64.

    arg = fl(6.2831855f * fl(fl(fl(f0 / sr) * n) + phase)), n = 1..upp;  S = sin(arg) in float64;
    v = fl(fl(fl(fl(fl(S * 0.1f) * uv) + fl(amp * nz)) * lw) + lb), evaluated in float32 at S -+ L_sin ulp (the chain is monotone in S);  tanh in float64, -+ L_tanh ulp."""
    f = np.asarray(f0, dtype=f32)
    B, T = f.shape
    ph = phase(f, sr, upp, variant if variant in PHASE_VARIANTS else None)
    n = np.arange(upp, dtype=f32) if variant == "n_from_0" else np.arange(1, upp + 1, dtype=f32)
    rad = (f / f32(sr))[:, :, None] * n[None, None, :] + ph[:, :, None]
    assert rad.dtype == f32
    if variant == "two_pi_f64":
        S = np.sin(2.0 * np.pi * rad.astype(f64))
    else:
        S = np.sin((TWO_PI_F32 * rad).astype(f64))
    voiced = (f >= 0) if variant == "uv_ge" else (f > 0)
    uv = voiced.astype(f32)[:, :, None]
    a_v, a_u = f32(0.003), f32(0.1) / f32(3.0)
    amp = np.where(voiced, a_u, a_v) if variant == "amp_swapped" else np.where(voiced, a_v, a_u)
    nz = np.zeros((B, T, upp), dtype=f32) if noise is None else np.asarray(noise, dtype=f32).reshape(B, T, upp)
    an = amp.astype(f32)[:, :, None] * nz
    lw, lb = f32(lw), f32(lb)

    def chain(s):  # float32 in, float32 out, one rounding per operation
        v = ((s * f32(0.1)) * uv + an) * lw + lb
        assert v.dtype == f32
        return v.astype(f64)

    u = ulp32(S)
    # round-to-nearest of an end never excludes an admissible float32: it lands on the first float32 inside the end, or outside it
    va = chain(np.clip(S - L_sin * u, -1.0, 1.0).astype(f32))
    vb = chain(np.clip(S + L_sin * u, -1.0, 1.0).astype(f32))
    ta, tb = np.tanh(np.minimum(va, vb)), np.tanh(np.maximum(va, vb))
    lo, hi = ta - L_tanh * ulp32(ta), tb + L_tanh * ulp32(tb)
    centre = np.tanh(chain(S.astype(f32)))
    shape = (B, 1, T * upp)
    return lo.reshape(shape), hi.reshape(shape), centre.reshape(shape)


# ---- F.interpolate(mode="linear", align_corners=False) along the last axis -------------------------------------------------------------------

# y: the value in float64, tol: 2 ulp32(max(|r[i0]|, |r[i1]|)) -- two products (l <= 1: half an ulp of the operand each) and one add (half an ulp of at
# most the larger operand), rounded separately or fused: 1.5 ulp at most, nothing measured; src, i0, l0, l1, r0, r1: the float32 index this rounding gives, the sample it selects, the weights, the two samples read
Candidate = collections.namedtuple("Candidate", "name y tol src i0 l0 l1 r0 r1")


def interp_admissible(r, Lout, variant=None):
    """rows r [.., Lin] -> the candidate results of ``interp_linear_at`` [.., Lout], one per admissible rounding of the float32 source index:
    "separate": src = fl(fl(scale * (o + 0.5f)) - 0.5f);  "fused": src rounded once from the exact scale * (o + 0.5) - 0.5;  scale = fl(fl(Lin) / fl(Lout))."""
    r = np.asarray(r, dtype=f32)
    Lin = r.shape[-1]
    rows = r.reshape(-1, Lin)
    o = np.arange(Lout, dtype=f32)
    scale = f32(Lin) / f32(Lout)
    if variant == "align_corners":
        scale = f32(Lin - 1) / f32(max(Lout - 1, 1))
        srcs = {"separate": scale * o, "fused": scale * o}
    elif variant == "no_half_pixel":
        srcs = {"separate": scale * o, "fused": scale * o}
    else:
        oh = o + f32(0.5)  # exact below 2^23
        srcs = {"separate": scale * oh - f32(0.5), "fused": (f64(scale) * oh.astype(f64) - 0.5).astype(f32)}  # (a 24 x 21 bit product: exact in float64)
    flat = np.concatenate([rows.astype(f64).ravel(), [2.0]])  # "i1_unclamped" reads on into the next row (behind the last row: a 2.0 no row holds)
    base = (np.arange(rows.shape[0], dtype=np.int64) * Lin)[:, None]
    out = []
    for name, src in srcs.items():
        assert src.dtype == f32
        if variant != "no_clamp_low":
            src = np.where(src < 0, f32(0), src)
        i0 = np.minimum(np.trunc(src).astype(np.int64), Lin - 1)  # (int)src truncates towards zero
        i1 = i0 + 1 if variant == "i1_unclamped" else i0 + (i0 < Lin - 1)
        l1 = src - i0.astype(f32)
        l0 = f32(1.0) - l1
        assert l1.dtype == f32 and l0.dtype == f32
        r0, r1 = flat[base + i0[None, :]], flat[base + i1[None, :]]
        y = l0.astype(f64)[None, :] * r0 + l1.astype(f64)[None, :] * r1
        tol = 2.0 * ulp32(np.maximum(np.abs(r0), np.abs(r1)))
        shape = r.shape[:-1] + (Lout,)
        out.append(Candidate(name, y.reshape(shape), tol.reshape(shape), src, i0, l0, l1, r0.reshape(shape), r1.reshape(shape)))
    return out


def interp_within(got, cands):
    """-> bool mask: which samples of ``got`` lie within ``tol`` of at least one candidate"""
    g = np.asarray(got, dtype=f64)
    ok = np.zeros(g.shape, dtype=bool)
    for c in cands:
        ok |= np.abs(g - c.y) <= c.tol
    return ok
