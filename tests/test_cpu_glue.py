"""The edge cases of tests/glue_cases.py on the ORACLE alone: pinned to the reference's own functions where a fixture exists
(tests/golden/glue_f0_patterns.npz, oracle/make_golden.py:glue_case), and the conditions under which tests/test_gpu_glue_edges.py may hold
the device to them bit for bit -- no coarse bin decided by the last ulps of a log, exact ties that really are exact, the thresholds hit."""
import numpy as np
import torch

import glue_cases as gc
from conftest import load_golden
from oracle import glue_oracle


def test_oracle_reproduces_the_reference_on_every_small_pattern():
    """Every voiced / unvoiced pattern of 1 .. 7 frames, nine target lengths, keys 0 and -5.5: ``glue_oracle.rmvpe_f0`` against the
    reference's _decode / _resize_f0 / _interpolate_f0 / post_process (the fixture), bit for bit.  The fixture's inputs are the cases."""
    d = load_golden("glue_f0_patterns")
    cases = gc.rmvpe_pattern_cases()
    assert len(cases) == 4512 and len(d["n"]) == len(cases)
    assert tuple(int(b) for b in d["bins"]) == gc.PATTERN_BINS and d["peak"] == np.float32(gc.PATTERN_PEAK)
    assert np.array_equal(np.array([c[:3] for c in cases]), np.stack([d["n"], d["mask"], d["p_len"]], 1))
    assert np.array_equal(np.array([c[3] for c in cases], np.float64), d["key"])
    dec = glue_oracle.rmvpe_decode(gc.pattern_salience(7, 127), 0.03)
    assert np.array_equal(dec, d["decoded_hz"]) and len(set(dec)) == 7 and dec.min() >= 60 and dec.max() <= 520
    off = d["off"]
    for c, (pitch, pitchf) in enumerate(gc.rmvpe_pattern_oracle()):
        assert pitch.dtype == np.int64 and pitchf.dtype == np.float32
        assert np.array_equal(pitch, d["pitch"][off[c]:off[c + 1]]) and np.array_equal(pitchf, d["pitchf"][off[c]:off[c + 1]]), cases[c]


def test_patterns_cover_the_gap_endings():
    """What the ``j < N - 1`` quirk of _interpolate_f0 decides: gaps that end at N - 2, at N - 1, and that do not end; and the patterns
    are complete (every mask of every length)."""
    assert [len([1 for n, _ in gc.patterns() if n == k]) for k in range(1, 8)] == [2, 4, 8, 16, 32, 64, 128]
    assert gc.pattern_p_lens(1) == [1, 2, 3, 5] and gc.pattern_p_lens(4) == [1, 2, 3, 4, 5, 7, 8, 9, 14]
    ends = set()
    for n, m in gc.patterns():
        v = [(m >> i) & 1 for i in range(n)]
        for i in range(n):
            if not v[i] and (i == 0 or v[i - 1]):
                j = next((k for k in range(i, n) if v[k]), None)
                ends.add("open" if j is None else n - j)   # the first voiced frame after the gap, counted from the end
    assert {"open", 1, 2, 3} <= ends


def _assert_chain_conditions(dec, mel, what):
    assert gc.mel_margin(mel) >= gc.MEL_MARGIN, "%s: a mel value %.3e from a rint boundary" % (what, gc.mel_margin(mel))
    assert gc.hz_margin(dec) >= gc.HZ_MARGIN, "%s: a decoded Hz %.3e (relative) from a threshold" % (what, gc.hz_margin(dec))


def test_f0_pattern_conditions_hold_for_every_case():
    """No case is dropped: every one of them keeps its mel values 1e-9 from a ``.5`` boundary and its decoded Hz off 10.0 and 0.001."""
    oracle = gc.rmvpe_pattern_oracle()
    for c, (n, m, p_len, key) in enumerate(gc.rmvpe_pattern_cases()):
        dec, mel, pitch, pitchf = gc.chain_parts(gc.pattern_salience(n, m), p_len, key)
        _assert_chain_conditions(dec, mel, (n, m, p_len, key))
        assert np.array_equal(pitch, oracle[c][0]) and np.array_equal(pitchf, oracle[c][1])   # the parts ARE the oracle's chain
    want = gc.post_pattern_oracle()
    assert len(want) == 254 * 4
    for c, (n, m, key) in enumerate(gc.post_pattern_cases()):
        mel, pitch, pitchf = gc.oracle_f0_post(gc.pattern_f0(n, m), key)
        assert gc.mel_margin(mel) >= gc.MEL_MARGIN, (n, m, key)
        assert np.array_equal(pitch, want[c][0]) and np.array_equal(pitchf == 0, np.array([not (m >> i) & 1 for i in range(n)]))
    assert len(set(gc.POST_HZ)) == 7 and min(gc.POST_HZ) >= 60 and max(gc.POST_HZ) <= 520


def test_decode_edges_are_the_edges():
    sal = gc.decode_edge_salience()
    assert sal.shape == (13, 360) and len(gc.DECODE_EDGE_ROWS) == 13 and 13 % 4 and 11 % 4 and gc.DECODE_EDGE_NS[:2] == (13, 11)
    am = np.argmax(sal, 1)
    assert list(am[:6]) == [0, 3, 356, 359, 3, 10] and am[6] == 0 and am[7] == 0
    for row, (b0, b1), same_lane in ((4, (3, 67), True), (5, (10, 74), True), (11, (3, 68), False), (12, (10, 67), False)):
        assert sal[row, b0] == sal[row, b1] == sal[row].max() and (sal[row] == sal[row].max()).sum() == 2 and am[row] == b0
        assert (b0 % 64 == b1 % 64) == same_lane   # lane l of the decode's wave reads bins l, l + 64, ...
    assert 10 % 64 > 67 % 64                       # row 12: the first maximum sits in the HIGHER lane
    assert (sal[6] == np.float32(0.2)).all() and not sal[7].any()
    assert sal[8].max() == np.float32(0.03) and sal[9].max() == np.nextafter(np.float32(0.03), np.float32(1))
    assert (sal[:4, :] > 0).all() and (sal[10] > 0).all()   # the floor: a window read outside its row would not read zeros
    with np.errstate(invalid="ignore", divide="ignore"):
        dec = glue_oracle.rmvpe_decode(sal, 0.03)
    assert list(dec > 0) == [True, True, True, True, True, True, True, False, False, True, True, True, True]
    # the first of two equal maxima: the window around bin 3 / 10, not the one around 67 / 68 / 74
    lo = lambda b: 10 * 2 ** ((20 * (b - 4) + 1997.3794084376191) / 1200)  # noqa: E731
    assert all(lo(3) < dec[r] < lo(3 + 8) for r in (4, 11)) and all(lo(10) < dec[r] < lo(10 + 8) for r in (5, 12))
    for n in gc.DECODE_EDGE_NS:
        dec, mel, pitch, pitchf = gc.chain_parts(sal[:n], n, 0)
        _assert_chain_conditions(dec, mel, "decode edges, n = %d" % n)
        assert all(np.array_equal(a, b) for a, b in zip((pitch, pitchf), gc.oracle_rmvpe_f0(sal[:n], n, 0)))


def test_work_array_threshold_cases_sit_on_the_threshold():
    n = gc.THRESHOLD_N
    assert (n + n) * 8 == 160 * 1024 and gc.THRESHOLD_RMVPE[0][:2] == (n, n) and gc.THRESHOLD_RMVPE[1][:2] == (n, n + 1)
    assert [c[0] for c in gc.THRESHOLD_POST] == [n, n + 1]
    rm, post = gc.threshold_oracle()
    for (n_, p_len, key), (dec, mel, pitch, pitchf) in zip(gc.THRESHOLD_RMVPE, rm):
        _assert_chain_conditions(dec, mel, (n_, p_len))
        assert 0 < (dec == 0).sum() < n_ and dec[-1] == 0 and dec[0] == 0 and len(set(pitch)) > 50   # leading, inner and trailing gaps
        assert all(np.array_equal(a, b) for a, b in zip((pitch, pitchf), gc.oracle_rmvpe_f0(gc.threshold_salience()[:n_], p_len, key)))
    for (n_, key), (mel, pitch, pitchf) in zip(gc.THRESHOLD_POST, post):
        assert gc.mel_margin(mel) >= gc.MEL_MARGIN and pitch.shape == (n_,) and {1, 255} <= set(pitch)


def test_expand_protect_cases():
    cases = gc.expand_cases()
    assert {c[0] for c in cases} == {1, 255, 256, 257, 768} and {c[1] for c in cases} == {1, 2, 5}
    assert all({c[2] for c in cases if c[1] == nq} == {1, 2 * nq - 1, 2 * nq} for nq in (1, 2, 5))
    assert gc.PROTECTS[2] < 0.5 and np.float32(gc.PROTECTS[2]) == np.float32(0.5) and gc.PROTECT_PITCHF[2] < 1 < gc.PROTECT_PITCHF[4]
    first = set()
    for (d, nq, p_len, protect, feats, pitchf), want in zip(cases, gc.expand_oracle()):
        assert want.shape == (1, p_len, d)
        first.add(float(pitchf[0, 0]))
        x2 = feats[0].repeat_interleave(2, 0)[:p_len]
        if protect >= 0.5:
            assert torch.equal(want[0], x2)
        else:  # pitchf < 1 (0, 0.5, just under 1) is protected: x * protect + x * (1 - protect); >= 1 passes through: x * 1 + x * 0
            prot = pitchf[0, :p_len] < 1
            pf = torch.where(prot, torch.tensor(protect, dtype=torch.float32), torch.tensor(1.0))[:, None]
            assert torch.equal(want[0], x2 * pf + x2 * (1 - pf))
    assert first == {float(np.float32(v)) for v in gc.PROTECT_PITCHF}


def test_int16_cases():
    cases, want = gc.int16_cases(), gc.int16_oracle()
    assert len(cases) == len(gc.INT16_NS) * 4
    for (n, kind, a), w in zip(cases, want):
        assert a.shape == w.shape == (n,)
        if kind == "tail -2.5":
            assert a[-1] == -2.5 and (n == 1 or np.abs(a[:-1]).max() <= 0.1)
            assert abs(float(np.abs(w).max()) - 32768 * 0.99) < 0.01 and abs(w[-1]) == np.abs(w).max()
        elif kind == "zeros":
            assert not w.any()
        elif kind == "peak 0.5":   # audio_max <= 1: plain * 32768, exact
            assert np.array_equal(w, a * np.float32(32768))
        else:                      # float32(0.99) / 0.99 > 1 in float64: the scaling branch, by less than float32 resolves
            assert np.abs(a).max() == np.float32(0.99) and float(np.float32(0.99)) / 0.99 > 1
            assert np.float32(32768 / (float(np.float32(0.99)) / 0.99)) == 32768 and np.array_equal(w, a * np.float32(32768))


def test_sola_ties_are_exact_and_the_first_wins():
    cases, want = gc.sola_cases(), gc.sola_oracle()
    tied = 0
    for c, (out, buf, off) in zip(cases, want):
        assert out.shape == (c["block"],) and buf.shape == (c["Lb"],) and c["x"].numel() == c["Ls"] + c["block"] + c["Lb"]
        if c["expect"] is not None:
            assert off == c["expect"], c["name"]
    for P, Lb, Ls, o0, block in gc.SOLA_TIES + (gc.SOLA_LDS_FIT,):
        pat = gc.integer_pattern(P)
        assert gc.shortest_period(pat) == P and pat.abs().max() <= 3 and torch.equal(pat, pat.round())
        assert Lb * 9 < 2 ** 24   # every partial sum is an integer fp32 holds exactly
        c = gc.sola_tie_case(P, Lb, Ls, o0, block)
        later = [o for o in range(o0 + P, Ls + 1, P)]
        for o in later:  # the same window, sample for sample: the same quotient whatever the arithmetic
            assert torch.equal(c["x"][o:o + Lb], c["buf"])
        tied += len(later)
        assert later or Ls < o0 + P
    assert tied > 100
    # thread t of the search owns offsets t, t + 256, ...: ties across threads (P = 7), inside one thread (P = 256), and thread 0 with one
    # and with two offsets (Ls = 255, 256)
    assert gc.SOLA_TIES[1][0] == 256 and {c[2] for c in gc.SOLA_TIES} >= {0, 255, 256}
    for P, Lb, Ls, o0, block in (gc.SOLA_LDS_FIT, gc.SOLA_LDS_OVER):
        assert ((2 * Lb + Ls) * 4 > 150 * 1024) == (Ls == 401)
    assert (2 * gc.SOLA_LDS_FIT[1] + gc.SOLA_LDS_FIT[2]) * 4 == 150 * 1024
    names = [c["name"] for c in cases]
    assert {"zero chunk", "zero buffer", "block < Lb", "Lb = 1", "150 KiB of LDS"} <= set(names)
    by = dict(zip(names, cases))
    assert not by["zero chunk"]["x"].any() and by["zero chunk"]["buf"].any() and not by["zero buffer"]["buf"].any()
    assert by["block < Lb"]["block"] < by["block < Lb"]["Lb"]


def test_envelope_cases_run_finite_on_the_oracle():
    cr = gc.change_rms_cases()
    assert len(cr) == 12 and {c[4] for c in cr} == {0.0, 0.25, 1.0}
    for (sr1, n1, sr2, n2, rate, d1, d2), want in zip(cr, gc.change_rms_oracle()):
        assert want.shape == (n2,) and np.isfinite(want).all() and (d1 == 0).any() and (d2 == 0).any()
    frames = [(1 + n1 // (sr1 // 2), 1 + n2 // (sr2 // 2)) for sr1, n1, sr2, n2 in gc.CHANGE_RMS_GEOM]
    assert frames[0] == (1, 1) and frames[1] == (2, 2) and (601 // 2 * 2) % 256 and 100 // 2 * 2 < 256
    assert glue_oracle.frame_rms(cr[6][5], 600, 300).min() == 0   # a whole frame of silence: rms1 == 0
    for (zc, n, rate, inp, wav), want in zip(gc.envelope_cases(), gc.envelope_oracle()):
        assert want.shape == (n,) and np.isfinite(want).all() and (inp[:n] == 0).any() and (wav == 0).any()
    assert [(n % zc != 0, n < zc, n == zc) for zc, n in gc.ENVELOPE_GEOM] == [(True, False, False), (True, False, False), (True, True, False),
                                                                              (False, False, True), (False, False, False)]
    assert gc.ENVELOPE_GEOM[4] == (1, 300)   # one frame per sample: the interpolation's input and output lengths coincide


def test_resample_cases():
    width = {}
    for orig, new, n, x, want in gc.resample_cases():
        g = np.gcd(orig, new)
        of, nf = orig // g, new // g
        width[(orig, new)] = int(np.ceil(6 * of / (min(of, nf) * 0.99)))
        assert want.shape == (-(-nf * n // of),) and np.isfinite(want).all()
        if n == 1000:
            assert want.shape[0] % 256 and want.shape[0] % nf
    assert width[(423, 400)] == 7 and sorted(c[2] for c in gc.resample_cases() if c[0] == 423) == [1, 3, 6]


def test_phase_vocoder_edge_fixture():
    """The extended fixture of tools/make_golden_gui.py: all sizes and cases present; the windows are all zero at n <= 2, where the
    reference's fp32 run equals its fp64 run exactly and only the absolute bars can apply."""
    assert gc.PV_EDGE_SIZES[-1] == gc.PV_MAX_N and gc.PV_MAX_N - 1 in gc.PV_EDGE_SIZES
    for n in gc.PV_EDGE_SIZES:
        for case in gc.PV_CASES:
            a, b, fo, fi, r32, r64 = gc.pv_case(n, case)
            assert a.shape == b.shape == fo.shape == fi.shape == r32.shape == r64.shape == (n,)
            assert a.dtype == np.float32 and r64.dtype == np.float64 and np.isfinite(r64).all()
            if n <= 2:
                assert not (fo * fi).any() and np.array_equal(r32, r64)
            gc.pv_check(n, r64.astype(np.float32), r32, r64)   # the correctly rounded result passes its own bars
    assert gc.pv_bars(1920) == (2e-8, 1e-7) and gc.pv_bars(64) == (2e-8, 1e-7) and gc.pv_bars(3840) == (4e-8, 2e-7)
