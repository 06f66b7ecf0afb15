"""The checker of the excitation's kernels checked (no GPU): oracle/source_oracle.py against the reference's own float32 evaluation (oracle/nsf_oracle.py, torch
on the CPU), over the cases of tests/source_cases.py that tests/test_gpu_source.py runs on the device.

  * The phase is bit-determined.  Every increment is a multiple of 2^-25, so ``phase`` (exact integer prefix sums, one rounding), torch's CPU cumsum (the
    reference's path) and k_phase_scan's partition (per-thread sums, 64-lane scan, wave totals, restated step by step in float64) agree bit for bit on
    every case: the set of frames on which a device may differ from the oracle is EMPTY, and that is asserted.
  * ``har_interval`` holds the reference's float32 evaluation with zero samples outside, on every case.
  * Every named wrong variant leaves the interval (or the interpolation's admissible band), with a floor on how many samples do.
  * torch's float32 F.interpolate lies inside ``interp_admissible`` on every sample; its distance to the float64 interpolation (printed) is the float32
    index's own error -- orders above the band, which is why the oracle is not the float64 interpolation.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import source_cases as sc  # noqa: E402
from oracle import source_oracle as so  # noqa: E402


def _pick(T, kind, cfg="v2_48k", **kw):
    got = [c for c in sc.HAR_CASES if (c.cfg, c.B, c.T, c.kind) == (cfg, 1, T, kind) and all(getattr(c, k) == v for k, v in kw.items())]
    assert got, (T, kind)
    return got[0]


# ---- the phase ---------------------------------------------------------------------------------------------------------------------------------

def _torch_phase(f0, sr, upp):
    """oracle/nsf_oracle.sine_source's lines for the phase (generators.py:154-158), torch on the CPU"""
    f0 = f0.unsqueeze(-1)
    rad = f0 / sr * torch.arange(1, upp + 1, dtype=f0.dtype)
    rad2 = torch.fmod(rad[:, :-1, -1:].float() + 0.5, 1.0) - 0.5
    return F.pad(rad2.cumsum(dim=1).fmod(1.0), (0, 0, 1, 0))[..., 0].numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("c", sc.HAR_CASES, ids=sc.case_id)
def test_the_phase_is_bit_determined(c):
    cfg, f0 = sc.CONFIGS[c.cfg], sc.inputs(c)["f0"]
    assert so.is_on_grid(so.increments(f0.numpy(), cfg.sr, cfg.upp)), "an increment off the 2^-25 grid"
    ph = so.phase(f0.numpy(), cfg.sr, cfg.upp)
    assert ph.dtype == np.float32 and ph.shape == (c.B, c.T)
    differs_torch = np.flatnonzero(_bits(ph) != _bits(_torch_phase(f0, cfg.sr, cfg.upp)))
    differs_kernel = np.flatnonzero(_bits(ph) != _bits(so.phase_kernel_partition(f0.numpy(), cfg.sr, cfg.upp)))
    print("%s: phase in [%.6f, %.6f], frames differing from torch's cumsum %d, from the kernel's partition %d" % (
        sc.case_id(c), ph.min(), ph.max(), differs_torch.size, differs_kernel.size))
    assert differs_torch.size == 0 and differs_kernel.size == 0, "the exclusion set is not empty"


def test_the_phase_cases_reach_what_they_are_there_for():
    cfg = sc.CONFIGS["v2_48k"]
    pref = lambda c: np.cumsum(so.increments(sc.inputs(c)["f0"].numpy(), cfg.sr, cfg.upp).astype(np.float64), axis=1)  # noqa: E731
    assert pref(_pick(1201, "up")).max() > 500 and pref(_pick(1201, "down")).min() < -500       # a coarse fp32 prefix, either sign
    assert so.phase(sc.inputs(_pick(258, "down"))["f0"].numpy(), cfg.sr, cfg.upp).min() < 0     # fmodf's negative phase
    w = so.increments(sc.inputs(_pick(258, "halfgrid"))["f0"].numpy(), cfg.sr, cfg.upp)
    assert (w == -0.5).any() and (w > 0.4999).any()                                             # the wrap, both sides
    assert not so.increments(sc.inputs(_pick(258, "grid"))["f0"].numpy(), cfg.sr, cfg.upp).any()


# ---- the interval ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", sc.HAR_CASES, ids=sc.case_id)
def test_the_interval_holds_the_reference(c):
    r = sc.har_record(c, sc.reference_har(c))
    print("%s: reference outside %d of %d, worst %.2f ulp from the centre at %s, %.2f of the way to the interval's edge; interval width median %.2e max %.2e" % (
        r["case"], r["outside"], r["samples"], r["worst_ulp"], r["worst_at"], r["worst_share"], r["width_median"], r["width_max"]))
    assert r["outside"] == 0, r["first_outside"]


def _frames_left(c, variant):
    """-> (mask of frames with a sample of the variant's float32 evaluation outside the case's interval [B, T], the share of samples outside)"""
    upp = sc.CONFIGS[c.cfg].upp
    lo, hi, _ = sc.interval(c)
    wrong = so.har_interval(*_args(c), variant=variant)[2].astype(np.float32)
    out = sc.outside(wrong, lo, hi).reshape(c.B, c.T, upp)
    return out.any(axis=2), float(out.mean())


def _args(c):
    cfg, x = sc.CONFIGS[c.cfg], sc.inputs(c)
    return (x["f0"].numpy(), None if x["noise"] is None else x["noise"].numpy(), cfg.sr, cfg.upp, *sc.linear_of(c.cfg, c.linear))


PHASE_SEP = [("fused_factor", _pick(258, "halfgrid")), ("fused_factor", _pick(258, "halfgrid", "v1_40k")), ("fused_factor", _pick(258, "halfgrid", "v2_32k")),
             ("seq_f32", _pick(258, "up")), ("seq_f32", _pick(258, "down")), ("seq_f32", _pick(1201, "up")), ("seq_f32", _pick(1201, "down")),
             ("shift_frame", _pick(258, "onset")), ("shift_frame", _pick(2, "onset")), ("shift_frame", _pick(258, "rand")),
             ("no_wrap", _pick(258, "up")), ("no_wrap", _pick(258, "rand"))]


@pytest.mark.parametrize("variant,c", PHASE_SEP, ids=["%s-%s" % (v, sc.case_id(c)) for v, c in PHASE_SEP])
def test_wrong_phases_leave_the_interval(variant, c):
    """Floor: at least one sample outside in EVERY affected frame.  Affected = voiced, and the wrong phase far enough from the right one that the sine must move
    by more than the interval is wide: a phase off by d moves sin(2 pi (x + phase)) by 2 sin(pi d) cos(.), a frame of f0 >= sr / (2 upp) covers half a turn and so
    holds a sample with |cos| >= 0.9, and har = tanh(lw (0.1 sin + ..) + lb) moves by 0.1 |lw| sech^2 of that: affected when
    0.1 |lw| min(sech^2) 2 sin(pi d) 0.9 > 2 max(hi - lo)  (twice the width: the wrong chain's own rounding of the sine's argument may take one back)."""
    cfg, f0 = sc.CONFIGS[c.cfg], sc.inputs(c)["f0"].numpy()
    lw, _ = sc.linear_of(c.cfg, c.linear)
    lo, hi, centre = sc.interval(c)
    d = np.abs(so.phase(f0, cfg.sr, cfg.upp, variant).astype(np.float64) - so.phase(f0, cfg.sr, cfg.upp).astype(np.float64))
    need = 2 * (hi - lo).max() / (0.1 * abs(lw) * (1 - centre ** 2).min() * 2 * 0.9)
    affected = (f0 >= cfg.sr / (2 * cfg.upp)) & (np.abs(np.sin(np.pi * d)) > need)
    left, share = _frames_left(c, variant)
    print("%s %s: phase differs on %d frames (up to %.2e), affected %d of %d (sin(pi d) > %.2e), frames with a sample outside %d, samples outside %.1f %%" % (
        variant, sc.case_id(c), (d > 0).sum(), d.max(), affected.sum(), d.size, need, left.sum(), 100 * share))
    assert affected.sum() >= 1, "the case does not show the variant"
    assert left[affected].all(), "%d affected frames stay inside" % (~left[affected]).sum()


SOURCE_SEP = [(v, c) for c in (_pick(258, "rand"), _pick(258, "rand", "v2_32k")) for v in so.SOURCE_VARIANTS]


@pytest.mark.parametrize("variant,c", SOURCE_SEP, ids=["%s-%s" % (v, sc.case_id(c)) for v, c in SOURCE_SEP])
def test_wrong_sources_leave_the_interval(variant, c):
    """Floors, a sample outside in every frame the variant touches: "n_from_0" every voiced frame (the sine one sample late: a phase off by f0 / sr >= 1e-3);
    "uv_ge" every unvoiced frame and "amp_swapped" every frame (the noise at ten times or a tenth of its amplitude, on 480 samples); "two_pi_f64" every voiced
    frame of f0 >= 800 Hz: there the argument passes 2 pi 8 = 50, float32(2 pi) is 1.75e-7 above 2 pi (1.4e-6 on the argument) and the product's own rounding is up
    to 1.9e-6, which moves har by up to 0.22 x 3.3e-6 = 7e-7 against a width of 4.5e-7 at most."""
    cfg, f0 = sc.CONFIGS[c.cfg], sc.inputs(c)["f0"].numpy()
    touched = {"n_from_0": f0 > 0, "uv_ge": f0 == 0, "amp_swapped": np.ones_like(f0, dtype=bool), "two_pi_f64": f0 >= 800.0}[variant]
    left, share = _frames_left(c, variant)
    print("%s %s: touched frames %d of %d, frames with a sample outside %d, samples outside %.1f %%" % (variant, sc.case_id(c), touched.sum(), f0.size, left.sum(), 100 * share))
    assert touched.sum() >= 20 and (f0 == 0).sum() >= 20 and (f0 > 0).sum() >= 20, "the case is not mixed"
    assert left[touched].all(), "%d touched frames stay inside" % (~left[touched]).sum()


# ---- the interpolation -------------------------------------------------------------------------------------------------------------------------

def _rows(c, shape):
    """The rows the realtime path interpolates: "har" [B, 1, T * upp] (the reference's excitation) or "z" [B, inter, T]"""
    return sc.reference_har(c) if shape == "har" else sc.inputs(c)["z"].numpy()


@pytest.mark.parametrize("shape", ["har", "z"])
@pytest.mark.parametrize("c", sc.INTERP_CASES, ids=sc.case_id)
def test_the_band_holds_the_reference_interpolation(c, shape):
    r = _rows(c, shape)
    Lin, Lout = r.shape[-1], (c.n_res * sc.CONFIGS[c.cfg].upp if shape == "har" else c.n_res)
    cands = so.interp_admissible(r, Lout)
    with torch.no_grad():
        t32 = F.interpolate(torch.from_numpy(r), size=Lout, mode="linear").numpy()
        t64 = F.interpolate(torch.from_numpy(r).double(), size=Lout, mode="linear").numpy()
    ok = so.interp_within(t32, cands)
    # the float32 index is within 2 ulp32(Lin) of the exact one (scale's rounding carried to the end of the row, the product's, the subtraction's), and the
    # interpolant is piecewise linear: it moves by no more than that times the steepest step of the row, plus the band itself
    step = float(np.abs(np.diff(r.astype(np.float64), axis=-1)).max()) if Lin > 1 else 0.0
    dist = float(np.abs(t32 - t64).max())
    s = sc.shares(t32, r)
    print("%s %s %d -> %d: torch f32 outside the band %d of %d; bit-equal to %s; the index roundings differ on %d samples of a row; torch f32 vs f64 max %.2e (index bound %.2e, band %.2e)" % (
        sc.case_id(c), shape, Lin, Lout, (~ok).sum(), ok.size, {k[6:]: "%.4f" % v for k, v in s.items() if k.startswith("equal_") and k != "equal_torch_f32"},
        s["index_roundings_differ_per_row"], dist, 2 * so.ulp32(Lin) * step, float(cands[0].tol.max())))
    assert ok.all()
    assert dist <= 2 * so.ulp32(Lin) * step + float(cands[0].tol.max())


# upsampling cases (the two edge variants show nowhere else); a one-sample z row (T = 1) has no slope, only the read behind its end shows there
INTERP_SEP = [(c, v, s) for c in sc.INTERP_CASES if c.n_res > c.T for v in so.INTERP_VARIANTS for s in ("har", "z") if not (s == "z" and c.T == 1 and v != "i1_unclamped")]


@pytest.mark.parametrize("c,variant,shape", INTERP_SEP, ids=["%s-%s-%s" % (sc.case_id(c), v, s) for c, v, s in INTERP_SEP])
def test_wrong_interpolations_leave_the_band(c, variant, shape):
    """Floors.  "align_corners" / "no_half_pixel" move the source position of (nearly) every sample by a fraction of a step: at least half of all samples leave.
    "no_clamp_low" extrapolates in front of the first input sample, "i1_unclamped" reads the next row's first sample behind the last (upsampling only: the samples with
    src < 0 and src > Lin - 1): at least one sample of that edge leaves in at least half of the rows, and nothing leaves anywhere else."""
    r = _rows(c, shape)
    Lin, Lout = r.shape[-1], (c.n_res * sc.CONFIGS[c.cfg].upp if shape == "har" else c.n_res)
    wrong = so.interp_admissible(r, Lout, variant)[1].y.astype(np.float32)
    out = ~so.interp_within(wrong, so.interp_admissible(r, Lout))
    rows = out.reshape(-1, Lout)
    src = (Lin / Lout) * (np.arange(Lout) + 0.5) - 0.5
    edge = {"no_clamp_low": src < 1e-6, "i1_unclamped": src > Lin - 1 - 1e-6}.get(variant)  # (1e-6: a float32 index that should be the edge itself may land beside it)
    print("%s %s %s: %d of %d samples outside%s" % (sc.case_id(c), shape, variant, out.sum(), out.size,
                                                    "" if edge is None else "; edge of %d samples, rows with one outside %d of %d" % (edge.sum(), rows[:, edge].any(axis=1).sum(), rows.shape[0])))
    if edge is None:
        # the float32 index resolves the variant's shift only where the shift exceeds its ulp (a har row of 96000 samples ends on steps of 2^-7)
        ref = {"align_corners": np.arange(Lout) * ((Lin - 1) / max(Lout - 1, 1)), "no_half_pixel": (Lin / Lout) * np.arange(Lout)}[variant]
        resolved = np.abs(ref - src) > 2 * so.ulp32(np.maximum(src, 1.0))
        print("   the float32 index resolves the shift on %.1f %% of a row" % (100 * resolved.mean()))
        assert resolved.any() and out.mean() >= 0.5 * resolved.mean()
    elif variant == "i1_unclamped" and 0.5 * (1 - Lin / Lout) <= so.ulp32(Lin):
        assert not out.any()  # the last index, Lin - 1 + (1 - Lin / Lout) / 2, rounds to Lin - 1 in float32: the weight of the read behind the end is zero
    else:
        assert edge.sum() >= 1 and rows[:, edge].any(axis=1).sum() >= max(1, rows.shape[0] // 2)
        assert not rows[:, ~edge].any()
