"""Fixtures of the quiet-point search that cuts a long input (infer/modules/vc/pipeline.py:219-236) -> tests/golden/cut_points.npz.

Expected values come from the reference's own statements: at fixture time only, the statements of ``Pipeline.pipeline`` from
``audio_pad = np.pad(...)`` to the end of the ``opt_ts`` loop are taken out of the reference's source text (``ast``) and executed
in a namespace that holds ``np``, ``audio`` and a ``self`` with ``window / t_center / t_query / t_max``; none of that text is
stored.  Per case the file keeps the geometry, the expected ``opt_ts``, the sha256 of the window sums
``audio_sum[t - t_query : t + t_query]`` (all cuts, concatenated) and, for the small cases, the sums themselves.  Inputs are stored
only when small.  The big ones are RECIPES (``long_input`` / ``periodic_input`` below): ``default_rng(seed).integers`` and exact
fp64 operations only (integer-valued samples and envelopes, scaling by powers of two), so that a test regenerates them bit for bit
on any numpy; the stored sha256 of the input is checked first.

    python tools/make_golden_cuts.py          (needs the reference tree: RVC_REFERENCE, default as oracle/make_golden.py)
"""
import ast
import hashlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SR, WINDOW = 16000, 160
STORE_SUMS_BELOW = 8192  # doubles


# ---- recipes (imported by the tests and by tools/cut_points_time.py) ----------------------------------------------------------------
def long_input(seed: int, n: int) -> np.ndarray:
    """A file-sized float64 signal with loud and quiet quarter-second stretches, from integers alone: int16-range samples times an
    integer envelope (a power of two per block, 1 in a quiet block), scaled by 2^-27 (|x| <= 0.5).  Every step is exact in fp64."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-32767, 32768, size=n).astype(np.float64)
    nb = (n + 3999) // 4000
    level = np.left_shift(1, rng.integers(4, 12, size=nb))
    level[rng.integers(0, 4, size=nb) == 0] = 1
    env = np.repeat(level, 4000)[:n].astype(np.float64)
    return np.ldexp(v * env, -27)


def periodic_input(seed: int, n: int) -> np.ndarray:
    """Period exactly 160, magnitudes with full 53-bit mantissas spread over six decades (2^0 .. 2^20): every window of 160 samples
    holds the same multiset of values, so all window sums are equal up to rounding and the argmin is decided by the ORDER of the
    adds alone."""
    rng = np.random.default_rng(seed)
    mant = rng.integers(2 ** 52, 2 ** 53, size=160).astype(np.float64)  # exact: below 2^53
    e = rng.integers(0, 21, size=160)
    sign = (rng.integers(0, 2, size=160) * 2 - 1).astype(np.float64)
    base = sign * np.ldexp(mant, e - 74)
    return np.tile(base, n // 160 + 1)[:n].copy()


def small_input(seed: int, n: int) -> np.ndarray:
    """Non-zero integers in +-[1, 2000] times 2^-11: sums of 160 of them are exact, and the arrays compress well."""
    rng = np.random.default_rng(seed)
    return np.ldexp((rng.integers(1, 2001, size=n) * (rng.integers(0, 2, size=n) * 2 - 1)).astype(np.float64), -11)


def sha(a: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def window_sums(audio_sum, opt_geom, n):
    """``audio_sum[t - t_query : t + t_query]`` of every cut, concatenated (numpy cuts the last one off at the end of the signal)."""
    t_center, t_query = opt_geom
    parts = [audio_sum[t - t_query: t + t_query] for t in range(t_center, n, t_center)]
    return np.concatenate(parts) if parts else np.zeros(0)


# ---- the reference's statements ------------------------------------------------------------------------------------------------------
def load_reference():
    """-> (run(audio, window, t_center, t_query, t_max) -> (opt_ts, audio_sum or None), bh, ah) from the reference's pipeline.py."""
    sys.path.insert(0, ROOT)
    from oracle.make_golden import REF

    path = os.path.join(REF, "infer", "modules", "vc", "pipeline.py")
    tree = ast.parse(open(path).read())
    from scipy import signal

    bh_ah = [s for s in tree.body if isinstance(s, ast.Assign) and isinstance(s.targets[0], ast.Tuple)
             and [getattr(e, "id", None) for e in s.targets[0].elts] == ["bh", "ah"]]
    assert len(bh_ah) == 1
    ns = {"signal": signal}
    exec(compile(ast.Module(body=bh_ah, type_ignores=[]), path, "exec"), ns)
    cls = [s for s in tree.body if isinstance(s, ast.ClassDef) and s.name == "Pipeline"][0]
    fn = [s for s in cls.body if isinstance(s, ast.FunctionDef) and s.name == "pipeline"][0]
    i = [k for k, s in enumerate(fn.body) if isinstance(s, ast.Assign) and getattr(s.targets[0], "id", None) == "audio_pad"][0]
    stmts = fn.body[i: i + 3]  # audio_pad = np.pad(...); opt_ts = []; if audio_pad.shape[0] > self.t_max: <sums, opt_ts loop>
    assert isinstance(stmts[1], ast.Assign) and stmts[1].targets[0].id == "opt_ts" and isinstance(stmts[2], ast.If)
    code = compile(ast.Module(body=stmts, type_ignores=[]), path, "exec")

    def run(audio, window, t_center, t_query, t_max):
        g = {"np": np, "audio": audio, "self": types.SimpleNamespace(window=window, t_center=t_center, t_query=t_query, t_max=t_max)}
        exec(code, g)
        return [int(t) for t in g["opt_ts"]], g.get("audio_sum")

    return run, ns["bh"], ns["ah"]


# ---- restatements that are "mathematically equal" (the order-sensitive case must tell them from the reference) ----------------------
def restated_offsets(audio, window, lo, hi):
    """argmin offsets within [lo, hi) of: numpy's pairwise sum, the reversed loop, a cumulative-sum difference."""
    p = np.abs(np.pad(audio, (window // 2, window // 2), mode="reflect"))
    n = audio.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(p, window)[:n]
    pairwise = win.sum(axis=1)
    rev = np.zeros(n)
    for i in reversed(range(window)):
        rev += p[i: i + n]
    c = np.concatenate([[0.0], np.cumsum(p)])
    diff = c[window: window + n] - c[:n]
    return {k: int(np.argmin(v[lo:hi])) for k, v in (("pairwise", pairwise), ("reversed", rev), ("cumsum", diff))}


def main():
    run, bh, ah = load_reference()
    from scipy import signal

    from oracle import synth

    out, names = {}, []

    def add(name, audio, window, t_center, t_query, t_max, kind, seed=0):
        opt_ts, audio_sum = run(audio, window, t_center, t_query, t_max)
        n = audio.shape[0]
        sums = window_sums(audio_sum, (t_center, t_query), n) if audio_sum is not None else np.zeros(0)
        p = name + "_"
        out[p + "geom"] = np.array([window, t_center, t_query, t_max, n], np.int64)
        out[p + "opt_ts"] = np.array(opt_ts, np.int64)
        out[p + "kind"], out[p + "seed"] = kind, seed
        out[p + "input_sha256"], out[p + "sums_sha256"] = sha(audio), sha(sums)
        if kind == "stored":
            out[p + "audio"] = audio
        if sums.size and sums.size < STORE_SUMS_BELOW:
            out[p + "sums"] = sums
        names.append(name)
        print("%-22s n %9d  cuts %-40s sums %s" % (name, n, opt_ts if len(opt_ts) < 6 else "%d cuts" % len(opt_ts), out[p + "sums_sha256"][:12]))
        return opt_ts

    # 1. production geometries (configs/config.py x_query, x_center, x_max) at 70 s, 200 s, 305 s
    for gi, (xq, xc, xm) in enumerate(((10, 60, 65), (6, 38, 41), (5, 30, 32))):
        for li, secs in enumerate((70, 200, 305)):
            seed = 100 + 10 * gi + li
            got = add("prod_q%d_c%d_%ds" % (xq, xc, secs), long_input(seed, secs * SR), WINDOW, xc * SR, xq * SR, xm * SR, "long", seed)
            assert len(got) == len(range(xc * SR, secs * SR, xc * SR)) > 0
    # 2. the test suite's geometry x_query = x_center = x_max = 1 on the real thing: make_audio16k through filtfilt, stored
    a = np.ascontiguousarray(signal.filtfilt(bh, ah, synth.make_audio16k(50000)))
    assert a.dtype == np.float64
    add("suite_50000", a, WINDOW, SR, SR, SR, "stored")
    # 3. order-sensitive
    seed = 7
    while True:
        a = periodic_input(seed, 40000)
        got = add("order_sensitive", a, WINDOW, 16000, 8000, 16000, "periodic", seed)
        ref_off = got[0] - 8000
        others = restated_offsets(a, WINDOW, 8000, 24000)
        print("    reference offset %d, restatements %s" % (ref_off, others))
        if all(v != ref_off for v in others.values()):
            break
        names.pop()
        seed += 1
    # 4. ties and 5. ends, small geometry: window 160, t_center 4000, t_query 1100 (search window [2900, 5100) = sum-kernel tiles
    #    [2900, 3924) [3924, 4948) [4948, 5100)); audio_sum[j] covers audio[j - 80 .. j + 79]
    W, TC, TQ, TM = 160, 4000, 1100, 4100

    def small(seed, n, zero=(), scale=()):
        a = small_input(seed, n)
        for lo, hi in zero:
            a[lo:hi] = 0.0
        for lo, hi, e in scale:
            a[lo:hi] = np.ldexp(a[lo:hi], e)
        return a

    assert add("zeros_in_tile", small(1, 9000, zero=[(3200, 3600)]), W, TC, TQ, TM, "stored")[0] == 3280
    assert add("zeros_straddle_tiles", small(2, 9000, zero=[(3700, 4100)]), W, TC, TQ, TM, "stored")[0] == 3780
    assert add("tie_first_and_last_tile", small(3, 9000, zero=[(3000, 3200), (4900, 5100)]), W, TC, TQ, TM, "stored")[0] == 3080
    assert add("min_at_first", small(4, 9000, zero=[(2820, 2980)]), W, TC, TQ, TM, "stored")[0] == 2900
    assert add("min_at_last", small(5, 9000, zero=[(5019, 5179)]), W, TC, TQ, TM, "stored")[0] == 5099
    assert add("at_threshold", small(6, 4100), W, TC, TQ, 4260, "stored") == []                # n + 160 == t_max: no search
    assert len(add("above_threshold", small(6, 4101), W, TC, TQ, 4260, "stored")) == 1         # one sample more: one cut
    assert len(add("just_above_t_center", small(7, 4001), W, TC, TQ, TM, "stored")) == 1
    got = add("right_reflection", small(8, 4101, scale=[(4101 - 120, 4101, -10)]), W, TC, TQ, TM, "stored")
    assert got[0] >= 4101 - 79, got                                                            # its window reaches the reflected samples
    # 6. subnormal magnitudes (integers times 2^-1040, about 1e-313 .. 2e-310) in one quiet stretch: flushed to zero they would tie
    a = small(9, 9000, scale=[(3300, 3700, -1029)])
    assert 0 < np.abs(a[3300:3700]).max() < 2.3e-308
    got = add("subnormal", a, W, TC, TQ, TM, "stored")
    flushed = a.copy()
    flushed[3300:3700] = 0.0
    assert run(flushed, W, TC, TQ, TM)[0][0] != got[0], "the subnormal case does not tell a flush-to-zero sum from the reference"
    out["names"] = np.array(names)
    path = os.path.join(GOLD, "cut_points.npz")
    np.savez_compressed(path, **out)
    print("cut_points.npz %d KB, %d cases" % (os.path.getsize(path) // 1024, len(names)))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
