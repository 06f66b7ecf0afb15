"""Shared pieces of the excitation's tests (tests/test_cpu_source.py, tests/test_gpu_source.py) and of tools/source_parity.py: the seeded cases, the
oracles of oracle/source_oracle.py applied to them, and one case run on the device.

Sizes are the smallest at which each thing can go wrong.  k_phase_scan gives each of its 256 threads ``per = ceil((T - 1) / 256)`` frames:

    T      T - 1   per   what it exercises
    1      0       0     no increments
    2      1       1     one thread busy
    3      2       1     two threads busy
    256    255     1     one thread idle
    257    256     1     every thread busy
    258    257     2     129 threads busy; two waves idle
    513    512     2     every thread busy
    514    513     3     171 threads busy
    1201   1200    5     240 threads busy; the last wave partly idle

f0 kinds: "synth" (oracle/synth.make_f0), "rand" (uniform 60..1100 Hz, 20 % unvoiced), "up" / "down" (constant, f0 / sr * upp with a fractional part of
0.49 / 0.51: the prefix grows to 0.49 T, where fp32 steps are coarse / goes negative, where fmodf returns a negative phase), "halfgrid" ((k + 1/2) sr / upp,
k = 0..10, and the float32 neighbours either side: one rounding step of the divide-then-multiply flips the increment between +0.5 and -0.5), "grid"
(k sr / upp: voiced with a zero increment), "unvoiced", "onset" (frame 0 voiced, the rest 0), "mixed" (row b of a batch is "rand", "up", "down" in turn).
``linear``: "seeded" = the weights of oracle/synth.make_dec_weights (lw = 2.5, lb = 0.1), "identity" = lw = 1, lb = 0 (the tightest interval).
A "har" tap ends the forward after two launches, so the long cases cost no more than their copy.
"""
import collections
import functools
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import nsf_cases as nc  # noqa: E402
from oracle import nsf_layer_oracle as lo  # noqa: E402
from oracle import nsf_oracle, synth  # noqa: E402
from oracle import source_oracle as so  # noqa: E402

CONFIGS = nsf_oracle.CONFIGS
MAX_B, MAX_T = 3, 1201  # one handle per config serves every "har" case
WEIGHT_SEED = 1234

Case = collections.namedtuple("Case", "cfg B T kind noise linear seed", defaults=("rand", True, "seeded", 0))
# (T, n_res): the realtime resampling of har (to n_res * upp samples) and of z (to n_res frames); B = 2, so that a read past a row's end lands in another row
Interp = collections.namedtuple("Interp", "cfg T n_res seed B", defaults=(0, 2))

HAR_CASES = (
    # the smallest sequences
    Case("v2_48k", 1, 1, "up", seed=1), Case("v2_48k", 1, 1, "unvoiced", seed=2), Case("v2_48k", 1, 2, "up", seed=3), Case("v2_48k", 1, 2, "onset", seed=4),
    Case("v2_48k", 1, 3, "up", seed=5), Case("v2_48k", 1, 3, "down", seed=6),
    # the partition's edges, each with a growing, a negative and a random prefix
    *(Case("v2_48k", 1, T, kind, seed=10 + 3 * i + j) for i, T in enumerate((256, 257, 258, 513, 514, 1201)) for j, kind in enumerate(("up", "down", "rand"))),
    # every other f0 pattern, at two frames per thread
    Case("v2_48k", 1, 258, "halfgrid", seed=30), Case("v2_48k", 1, 258, "grid", seed=31), Case("v2_48k", 1, 258, "unvoiced", seed=32),
    Case("v2_48k", 1, 258, "onset", seed=33), Case("v2_48k", 1, 258, "synth", seed=34), Case("v2_48k", 1, 1201, "synth", seed=35),
    Case("v2_48k", 1, 1201, "halfgrid", seed=36),
    # no noise, the identity linear layer (the tightest interval), both
    Case("v2_48k", 1, 258, "rand", False, seed=40), Case("v2_48k", 1, 258, "rand", True, "identity", seed=41), Case("v2_48k", 1, 258, "up", False, "identity", seed=42),
    Case("v2_48k", 1, 514, "halfgrid", False, "identity", seed=43),
    # three different rows: the row indexing of both kernels
    Case("v2_48k", 3, 258, "mixed", seed=50), Case("v2_48k", 3, 3, "mixed", seed=51),
    # the other shipped (sr, upp)
    Case("v1_40k", 1, 258, "up", seed=60), Case("v1_40k", 1, 1201, "rand", seed=61), Case("v1_40k", 1, 258, "halfgrid", seed=62),
    Case("v2_32k", 1, 258, "rand", seed=63), Case("v2_32k", 1, 1201, "down", seed=64), Case("v2_32k", 1, 258, "halfgrid", seed=65),
)

INTERP_CASES = tuple(Interp("v2_48k", T, n, 70 + i) for i, (T, n) in enumerate(
    ((64, 72), (64, 57), (64, 65), (64, 63), (64, 1), (1, 3), (2, 1), (3, 64), (200, 201)))) + (Interp("v1_40k", 64, 72, 80),)
INTERP_IDENTITY = (Interp("v2_48k", 64, 64, 81), Interp("v2_48k", 1, 1, 82))  # no interpolation may happen at all
INTERP_Z_CASES = tuple(c for c in INTERP_CASES if c.cfg == "v2_48k" and (c.T, c.n_res) in ((64, 72), (64, 57), (3, 64), (64, 1)))


def case_id(c):
    if isinstance(c, Interp):
        return "%s-B%d-T%d-nres%d" % (c.cfg, c.B, c.T, c.n_res)
    return "%s-B%d-T%d-%s%s%s" % (c.cfg, c.B, c.T, c.kind, "" if c.noise else "-nonoise", "" if c.linear == "seeded" else "-" + c.linear)


@functools.lru_cache(maxsize=None)
def weights(cfg_name, linear="seeded"):
    w = synth.make_dec_weights(CONFIGS[cfg_name], WEIGHT_SEED)
    if linear == "identity":
        w["m_source.l_linear.weight"] = torch.tensor([[1.0]])
        w["m_source.l_linear.bias"] = torch.tensor([0.0])
    return w


def linear_of(cfg_name, linear):
    w = weights(cfg_name, linear)
    return float(w["m_source.l_linear.weight"].reshape(())), float(w["m_source.l_linear.bias"].reshape(()))


def make_f0(kind, cfg, B, T, seed):
    """-> float32 [B, T]"""
    step = cfg.sr / cfg.upp  # 100 Hz in every shipped config: f0 = k * step turns the phase k times per frame
    rng = np.random.default_rng(1000 + seed)
    rows = []
    for b in range(B):
        k = ("rand", "up", "down")[b % 3] if kind == "mixed" else kind
        if k == "synth":
            f = synth.make_f0(B, T)[b].numpy()
        elif k == "rand":
            f = rng.uniform(60.0, 1100.0, T)
            f[rng.random(T) < 0.2] = 0.0
        elif k in ("up", "down"):
            f = np.full(T, (2 + b + (0.49 if k == "up" else 0.51)) * step)
        elif k == "halfgrid":
            c = ((np.arange(11) + 0.5) * step).astype(np.float32)
            f = np.roll(np.resize(np.stack([np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(1e9))], 1).ravel(), T), 5 * b)
        elif k == "grid":
            f = np.roll(np.resize(np.arange(1, 11) * step, T), 3 * b)
        elif k == "unvoiced":
            f = np.zeros(T)
        elif k == "onset":
            f = np.zeros(T)
            f[0] = 220.0 * (1 + b)
        else:
            raise ValueError(k)
        rows.append(np.asarray(f, dtype=np.float32))
    return torch.from_numpy(np.stack(rows))


@functools.lru_cache(maxsize=None)
def inputs(c):
    """-> {"z", "g", "f0", "noise"} of a Case or an Interp (noise None where the case runs without); computed once, never changed"""
    cfg = CONFIGS[c.cfg]
    z, _, g = synth.make_dec_inputs(cfg, c.B, c.T, 2000 + c.seed)
    kind, noise = (c.kind, c.noise) if isinstance(c, Case) else ("rand", True)
    return {"z": z, "g": g, "f0": make_f0(kind, cfg, c.B, c.T, c.seed),
            "noise": nsf_oracle.reference_noise(c.B, c.T, cfg.upp, 3000 + c.seed) if noise else None}


@functools.lru_cache(maxsize=4)
def interval(c, variant=None):
    """-> (lo, hi, centre) of oracle/source_oracle.har_interval for the case, float64 [B, 1, T * upp]"""
    cfg, x = CONFIGS[c.cfg], inputs(c)
    lw, lb = linear_of(c.cfg, c.linear)
    return so.har_interval(x["f0"].numpy(), None if x["noise"] is None else x["noise"].numpy(), cfg.sr, cfg.upp, lw, lb, variant=variant)


def reference_har(c):
    """The reference's own float32 evaluation (nsf_oracle.har_source, torch on the CPU) -> float32 numpy [B, 1, T * upp]"""
    cfg, x = CONFIGS[c.cfg], inputs(c)
    with torch.no_grad():
        return nsf_oracle.har_source(weights(c.cfg, getattr(c, "linear", "seeded")), x["f0"], cfg.upp, cfg.sr, x["noise"]).numpy()


def outside(har, lo, hi):
    har = np.asarray(har, dtype=np.float64)
    return (har < lo) | (har > hi)


def har_record(c, har):
    """``har`` [B, 1, T * upp] against the case's interval -> plain data: how many samples lie outside; the worst distance from the interval's centre in
    float32 ulps and where it occurs (item, frame, sample of the frame) -- over the samples with |centre| >= 1 / 64: near a zero of har = tanh(lw s + lb) the
    sum lw s + lb cancels, its error is an ulp of its OPERANDS, and in ulps of the tiny result that is thousands, for the reference too; and the worst
    distance as a share of the interval's half on that side (1 = on its edge), over all samples"""
    upp = CONFIGS[c.cfg].upp
    lo, hi, centre = interval(c)
    assert har.shape == lo.shape, (har.shape, lo.shape)
    e = np.asarray(har, dtype=np.float64) - centre
    d = np.where(np.abs(centre) >= 1.0 / 64, np.abs(e) / so.ulp32(centre), 0.0)
    share = np.where(e >= 0, e / (hi - centre), -e / (centre - lo))
    out = outside(har, lo, hi)
    i = int(np.argmax(d))
    b, s = divmod(i, c.T * upp)
    first = [int(v) for v in np.flatnonzero(out.ravel())[:8]]
    return {"case": case_id(c), "samples": int(d.size), "outside": int(out.sum()), "first_outside": [[v // (c.T * upp), v % (c.T * upp) // upp, v % upp] for v in first],
            "worst_ulp": float(d.ravel()[i]), "worst_at": {"item": b, "frame": s // upp, "sample": s % upp}, "worst_share": float(share.max()),
            "width_median": float(np.median(hi - lo)), "width_max": float((hi - lo).max())}


def shares(got, plain):
    """The interpolated rows ``got`` against ``interp_admissible`` of the rows ``plain`` they were made from -> plain data: samples outside the band; on how
    many samples the two roundings of the source index differ; the share of samples bit-equal to each rounding of the index combined with each rounding of
    l0 * r[i0] + l1 * r[i1] ("once": the exact sum rounded, "fma0" / "fma1": the product with l0 / l1 rounded, the other fused into the add, "sep": both products
    rounded), and to torch's float32 F.interpolate on the CPU"""
    got, plain = np.asarray(got, dtype=np.float32), np.asarray(plain, dtype=np.float32)
    Lout = got.shape[-1]
    cands = so.interp_admissible(plain, Lout)
    ok = so.interp_within(got, cands)
    with torch.no_grad():
        th = F.interpolate(torch.from_numpy(plain).reshape(-1, 1, plain.shape[-1]), size=Lout, mode="linear").numpy().reshape(got.shape)
    rec = {"samples": int(got.size), "outside": int((~ok).sum()), "index_roundings_differ_per_row": int((cands[0].src != cands[1].src).sum()),
           "equal_torch_f32": float((got == th).mean())}
    for cd in cands:
        for name, y in output_roundings(cd).items():
            rec["equal_%s_%s" % (cd.name, name)] = float((got == y).mean())
    return rec


def output_roundings(cd):
    """The float32 results of l0 * r[i0] + l1 * r[i1] for one candidate, by where the three operations round (products of two float32 are exact in float64)"""
    a, b = cd.l0.astype(np.float64) * cd.r0, cd.l1.astype(np.float64) * cd.r1
    ra, rb = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    return {"once": (a + b).astype(np.float32), "fma0": (ra + b).astype(np.float32), "fma1": (a + rb).astype(np.float32), "sep": (ra + rb).astype(np.float32)}


def pre_bars(c, z_rows):
    """The fp64 conv_pre + cond of oracle/nsf_layer_oracle.py (no operand rounding: the fp32 path) on the interpolated ``z_rows`` [B, inter, n_res], its float32
    evaluation, and the bars tests/nsf_cases.py derives for a layer of that kind whose tap is stored as fp32"""
    cfg, x, w = CONFIGS[c.cfg], inputs(c), weights(c.cfg)
    with torch.no_grad():
        y64 = lo.Layers(cfg, w, "f64", None).pre(z_rows, x["g"])
        y32 = lo.Layers(cfg, w, "f32", None).pre(z_rows, x["g"])
    return {"y": y64, **nc.bars_of(y32, y64, False, nc.kind_of("pre"))}


# ---- on the device (tests/test_gpu_source.py, tools/source_parity.py) -----------------------------------------------------------------------

_HANDLES = {}


def handle(cfg_name, linear, operand, device):
    """One generator per (config, linear layer, operand type), kept for the whole run (the fp32 one serves T = 258 at most: the operand type does not enter
    the excitation, which is asserted once, and its "pre" cases are short)"""
    import rvc_amd

    key = (cfg_name, linear, operand, str(device))
    max_B, max_T = MAX_B, MAX_T if operand != "fp32" else 258
    if key not in _HANDLES:
        _HANDLES[key] = rvc_amd.NSFGeneratorHIP(vars(CONFIGS[cfg_name]), weights(cfg_name, linear), device=device, operand=operand, max_B=max_B, max_T=max_T)
    return _HANDLES[key]


def release_handles():
    """Drop the generators (each owns a workspace sized for B = 3, T = 1201)"""
    _HANDLES.clear()


def device_tap(c, gen, device, what="har", n_res=None):
    """The tap of case ``c``, fetched twice and bit-equal -> float32 numpy"""
    x = inputs(c)
    args = (x["z"].to(device), x["f0"].to(device), x["g"].to(device))
    kw = dict(n_res=n_res, noise=None if x["noise"] is None else x["noise"].to(device))
    if x["noise"] is None:
        # the Python wrapper draws noise when it is given none; the C entry point takes a null pointer.  Zeros are the same excitation: amp * 0 = 0 exactly.
        kw["noise"] = torch.zeros(c.B, c.T * CONFIGS[c.cfg].upp, device=device)
    a, b = gen.debug_tap(what, *args, **kw), gen.debug_tap(what, *args, **kw)
    assert torch.equal(a, b), "%s: tap %s differs between two calls" % (case_id(c), what)
    assert bool(torch.isfinite(a).all()), what
    return a.numpy()


def device_har_case(c, device):
    """-> (record, har): the "har" tap of the fp16-operand handle against the interval"""
    har = device_tap(c, handle(c.cfg, c.linear, "fp16", device), device)
    return har_record(c, har), har


def device_interp_case(c, device):
    """-> (record, plain, got): the "har" tap under n_res against ``interp_admissible`` of the device's own plain tap of the same inputs"""
    gen = handle(c.cfg, "seeded", "fp16", device)
    plain, got = device_tap(c, gen, device), device_tap(c, gen, device, n_res=c.n_res)
    upp = CONFIGS[c.cfg].upp
    assert plain.shape == (c.B, 1, c.T * upp) and got.shape == (c.B, 1, c.n_res * upp), (plain.shape, got.shape)
    rec = {"case": case_id(c), "bit_equal_to_plain": bool(c.n_res == c.T and np.array_equal(plain, got))}
    if c.n_res != c.T:
        rec.update(shares(got, plain))
    return rec, plain, got


def device_z_case(c, device):
    """-> record: the "pre" tap of an fp32-operand handle under n_res against the fp64 conv_pre + cond applied to each admissible interpolation of z (rounded
    to float32, as the kernel stores it), at the bars of ``pre_bars``"""
    gen = handle(c.cfg, "seeded", "fp32", device)
    got = torch.from_numpy(device_tap(c, gen, device, "pre", n_res=c.n_res))
    rec = {"case": case_id(c), "candidates": []}
    for cd in so.interp_admissible(inputs(c)["z"].numpy(), c.n_res):
        b = pre_bars(c, torch.from_numpy(cd.y.astype(np.float32)))
        assert got.shape == b["y"].shape, (got.shape, b["y"].shape)
        rms, mx = nc.err(got, b["y"])
        rec["candidates"].append({"index": cd.name, "rms": rms, "max": mx, **{k: b[k] for k in ("floor_rms", "floor_max", "bar_rms", "bar_max")},
                                  "within_bars": bool(rms <= b["bar_rms"] and mx <= b["bar_max"])})
    return rec
