"""The device-resident glue (csrc/glue_kernels.hpp, csrc/glue.hip) against the oracle on the edge cases of tests/glue_cases.py: every small
voiced / unvoiced pattern through the f0 chain, argmax ties, windows that leave the salience map, the three LDS thresholds at and one over,
grid-stride tails, single frames, the smallest phase-vocoder sizes and the largest.  tests/test_cpu_glue.py pins those cases and their oracle
results (to the reference itself where a fixture exists) without a GPU.  Bars: tests/glue_cases.py, all of them the older suites' own.

A family with many cases collects its results on the device and reads them back once.  ``run_*`` return (case label, got, want) lists and
are shared with tools/glue_parity.py, which records the worst observed errors (profiles/glue_edges_parity.json)."""
import numpy as np
import pytest
import torch

import glue_cases as gc

pytestmark = pytest.mark.gpu


def _split(flat, sizes):
    return np.split(flat, np.cumsum(sizes)[:-1]) if len(sizes) > 1 else [flat]


def _check_f0(rows):
    for what, (pitch, pitchf), (want_p, want_f) in rows:
        assert pitch.shape == want_p.shape and pitchf.shape == want_f.shape, what
        assert np.array_equal(pitchf == 0, want_f == 0), "%s: the zero sets differ" % (what,)
        assert np.allclose(pitchf, want_f, rtol=gc.F0_RTOL, atol=0), "%s: pitchf differs (max rel %.2e)" % (
            what, np.max(np.abs(pitchf - want_f) / np.maximum(np.abs(want_f), 1e-9)))
        assert np.array_equal(pitch, want_p), "%s: %d coarse bins differ" % (what, int((pitch != want_p).sum()))


# ---- 1. the f0 chain -----------------------------------------------------------------------------------------------------------------
def run_rmvpe_patterns(gpu):
    import rvc_amd

    cases = gc.rmvpe_pattern_cases()
    # one upload per frame count: all 2^n saliences [2^n, n, 360]; a call reads its pattern's slice
    sal = {n: torch.from_numpy(np.stack([gc.pattern_salience(n, m) for m in range(1 << n)])).to(gpu) for n in range(1, gc.PATTERN_MAX_N + 1)}
    ps, fs = [], []
    for n, m, p_len, key in cases:
        pitch, pitchf = rvc_amd.glue.rmvpe_f0(sal[n][m], p_len, key, 0.03)
        ps.append(pitch[0])
        fs.append(pitchf[0])
    sizes = [c[2] for c in cases]
    got_p, got_f = _split(torch.cat(ps).cpu().numpy(), sizes), _split(torch.cat(fs).cpu().numpy(), sizes)
    return [(c, (p, f), w) for c, p, f, w in zip(cases, got_p, got_f, gc.rmvpe_pattern_oracle())]


def run_post_patterns(gpu):
    import rvc_amd

    cases = gc.post_pattern_cases()
    f0 = {(n, m): torch.from_numpy(gc.pattern_f0(n, m)).to(gpu) for n, m in gc.patterns()}
    ps, fs = [], []
    for n, m, key in cases:
        pitch, pitchf = rvc_amd.glue.f0_post(f0[(n, m)], key)
        ps.append(pitch[0])
        fs.append(pitchf[0])
    sizes = [c[0] for c in cases]
    got_p, got_f = _split(torch.cat(ps).cpu().numpy(), sizes), _split(torch.cat(fs).cpu().numpy(), sizes)
    return [(c, (p, f), w) for c, p, f, w in zip(cases, got_p, got_f, gc.post_pattern_oracle())]


def run_decode_edges(gpu):
    import rvc_amd

    host = gc.decode_edge_salience()
    sal = torch.from_numpy(host.copy()).to(gpu)
    rows = []
    for n in gc.DECODE_EDGE_NS:
        pitch, pitchf = rvc_amd.glue.rmvpe_f0(sal[:n], n, 0, 0.03)
        rows.append(("decode edges, first %d frames" % n, (pitch[0].cpu().numpy(), pitchf[0].cpu().numpy()), gc.oracle_rmvpe_f0(host[:n], n, 0)))
    return rows


def run_f0_thresholds(gpu):
    import rvc_amd

    want_rm, want_post = gc.threshold_oracle()
    sal = torch.from_numpy(gc.threshold_salience().copy()).to(gpu)
    rows = []
    for (n, p_len, key), (_, _, want_p, want_f) in zip(gc.THRESHOLD_RMVPE, want_rm):
        pitch, pitchf = rvc_amd.glue.rmvpe_f0(sal[:n], p_len, key, 0.03)
        rows.append(("rmvpe_f0 n %d p_len %d" % (n, p_len), (pitch[0].cpu().numpy(), pitchf[0].cpu().numpy()), (want_p, want_f)))
    for (n, key), (_, want_p, want_f) in zip(gc.THRESHOLD_POST, want_post):
        pitch, pitchf = rvc_amd.glue.f0_post(torch.from_numpy(gc.threshold_f0(n).copy()).to(gpu), key)
        rows.append(("f0_post n %d" % n, (pitch[0].cpu().numpy(), pitchf[0].cpu().numpy()), (want_p, want_f)))
    return rows


def test_rmvpe_f0_on_every_small_pattern(gpu):
    """Decode, resize, interpolation and binning on all 254 patterns of 1 .. 7 frames x nine target lengths x keys 0 and -5.5."""
    _check_f0(run_rmvpe_patterns(gpu))


def test_f0_post_on_every_small_pattern(gpu):
    _check_f0(run_post_patterns(gpu))


def test_rmvpe_decode_edges(gpu):
    """Windows off either end of the map, equal maxima inside a lane and across lanes, a flat row, a zero row, the threshold itself."""
    _check_f0(run_decode_edges(gpu))


def test_f0_work_arrays_at_the_lds_threshold(gpu):
    """10 240 frames: exactly 160 KiB of dynamic LDS (the launch must be granted), and one frame more: the global work arrays."""
    _check_f0(run_f0_thresholds(gpu))


# ---- 2. expand + protect -------------------------------------------------------------------------------------------------------------
def run_expand(gpu):
    import rvc_amd

    cases = gc.expand_cases()
    outs = [rvc_amd.glue.retrieve_blend_expand(f.to(gpu), None, 0.0, pf.to(gpu), protect, p_len) for _, _, p_len, protect, f, pf in cases]
    shapes = [tuple(o.shape) for o in outs]
    flat = torch.cat([o.reshape(-1) for o in outs]).cpu()
    got = [g.reshape(s) for g, s in zip(torch.split(flat, [int(np.prod(s)) for s in shapes]), shapes)]
    return [("d %d nq %d p_len %d protect %r" % c[:4], g, w) for c, g, w in zip(cases, got, gc.expand_oracle())]


def test_expand_protect_edges(gpu):
    for what, got, want in run_expand(gpu):
        assert got.shape == want.shape, what
        assert torch.equal(got, want), "%s: max abs diff %.3e" % (what, (got - want).abs().max())


# ---- 3. int16 scaling ----------------------------------------------------------------------------------------------------------------
def run_int16(gpu):
    import rvc_amd

    cases = gc.int16_cases()
    outs = [rvc_amd.glue.scale_int16_range(torch.from_numpy(a.copy()).to(gpu)) for _, _, a in cases]
    got = _split(torch.cat(outs).cpu().numpy(), [c[0] for c in cases])
    return [("n %d, %s" % c[:2], g, w) for c, g, w in zip(cases, got, gc.int16_oracle())]


def test_scale_int16_range_edges(gpu):
    for what, got, want in run_int16(gpu):
        assert np.array_equal(got, want), "%s: %d samples differ" % (what, int((got != want).sum()))


# ---- 4. SOLA -------------------------------------------------------------------------------------------------------------------------
def run_sola(gpu):
    import rvc_amd

    rows = []
    for c, (want_out, want_buf, want_off) in zip(gc.sola_cases(), gc.sola_oracle()):
        fade_in, fade_out = (w.to(gpu) for w in gc.fades(c["Lb"]))
        buf = c["buf"].to(gpu).clone()
        out, off = rvc_amd.glue.sola(c["x"].to(gpu), buf, fade_in, fade_out, c["block"], c["Ls"], return_offset=True)
        rows.append((c["name"], (out, buf, off), (want_out, want_buf, want_off)))
    return [(name, (out.cpu(), buf.cpu(), int(off.item())), want) for name, (out, buf, off), want in rows]


def test_sola_ties_and_degenerate_geometries(gpu):
    for what, (out, buf, off), (want_out, want_buf, want_off) in run_sola(gpu):
        assert off == want_off, "%s: offset %d, the oracle's %d" % (what, off, want_off)
        assert torch.equal(out, want_out) and torch.equal(buf, want_buf), what


def test_sola_refuses_one_sample_over_the_lds_limit(gpu):
    """(2 * 19000 + 401) * 4 bytes: ERR_NOMEM, and neither the output nor the buffer is touched."""
    from rvc_amd import _lib

    c = gc.sola_tie_case(*gc.SOLA_LDS_OVER)
    fade_in, fade_out = (w.to(gpu) for w in gc.fades(c["Lb"]))
    x, buf = c["x"].to(gpu), c["buf"].to(gpu).clone()
    out = torch.full((c["block"],), -7.0, device=gpu)
    off = torch.full((1,), -7, device=gpu, dtype=torch.int32)
    with torch.cuda.device(gpu):
        rc = _lib.lib().rvcmi_glue_sola(_lib.ptr(x), x.numel(), _lib.ptr(buf), c["Lb"], c["Ls"], _lib.ptr(fade_in), _lib.ptr(fade_out), c["block"],
                                        _lib.ptr(out), _lib.ptr(off), _lib.stream_ptr(gpu))
    torch.cuda.synchronize(gpu)
    assert rc == gc.ERR_NOMEM
    assert bool((out == -7.0).all()) and int(off.item()) == -7 and torch.equal(buf.cpu(), c["buf"])
    import rvc_amd

    with pytest.raises(rvc_amd.RvcmiError) as e:
        rvc_amd.glue.sola(x, buf, fade_in, fade_out, c["block"], c["Ls"])
    assert e.value.code == gc.ERR_NOMEM and torch.equal(buf.cpu(), c["buf"])


# ---- 5. the envelope mixes -----------------------------------------------------------------------------------------------------------
def run_change_rms(gpu):
    import rvc_amd

    cases = gc.change_rms_cases()
    outs = []
    for sr1, n1, sr2, n2, rate, d1, d2 in cases:
        t2 = torch.from_numpy(d2.copy()).to(gpu)
        out = rvc_amd.glue.change_rms(torch.from_numpy(d1.copy()).to(gpu), sr1, t2, sr2, rate)
        assert out.data_ptr() == t2.data_ptr()
        outs.append(out)
    got = _split(torch.cat(outs).cpu().numpy(), [c[3] for c in cases])
    return [("sr %d n %d -> sr %d n %d, rate %g" % c[:5], g, w) for c, g, w in zip(cases, got, gc.change_rms_oracle())]


def run_envelope_mix(gpu):
    import rvc_amd

    cases = gc.envelope_cases()
    outs = []
    for zc, n, rate, inp, wav in cases:
        w = torch.from_numpy(wav.copy()).to(gpu)
        out = rvc_amd.glue.envelope_mix(torch.from_numpy(inp.copy()).to(gpu), w, zc, rate)
        assert out.data_ptr() == w.data_ptr()
        outs.append(out)
    got = _split(torch.cat(outs).cpu().numpy(), [c[1] for c in cases])
    return [("zc %d n %d rate %g" % c[:3], g, w) for c, g, w in zip(cases, got, gc.envelope_oracle())]


def _max_rel(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-9)))


def test_change_rms_single_frames_and_odd_rates(gpu):
    for what, got, want in run_change_rms(gpu):
        assert np.isfinite(got).all(), what
        assert np.allclose(got, want, **gc.CHANGE_RMS_TOL), "%s: max rel %.2e" % (what, _max_rel(got, want))


def test_envelope_mix_ragged_and_single_frames(gpu):
    for what, got, want in run_envelope_mix(gpu):
        assert np.isfinite(got).all(), what
        assert np.allclose(got, want, **gc.ENVELOPE_TOL), "%s: max rel %.2e" % (what, _max_rel(got, want))


# ---- 6. the resampler ----------------------------------------------------------------------------------------------------------------
def run_resample(gpu):
    import rvc_amd

    return [("%d -> %d, n %d" % (orig, new, n), rvc_amd.SincResample(orig, new, gpu)(torch.from_numpy(x).to(gpu)).cpu().numpy(), want)
            for orig, new, n, x, want in gc.resample_cases()]


def test_sinc_resample_short_inputs_and_partial_blocks(gpu):
    for what, got, want in run_resample(gpu):
        assert got.shape == want.shape, what
        assert np.abs(got - want).max() <= gc.RESAMPLE_REL * max(1.0, np.abs(want).max()), "%s: max abs %.2e" % (what, np.abs(got - want).max())


# ---- 7. the phase vocoder ------------------------------------------------------------------------------------------------------------
def run_phase_vocoder(gpu, n):
    import rvc_amd

    rows = []
    for case in gc.PV_CASES:
        a, b, fo, fi, r32, r64 = gc.pv_case(n, case)
        got = rvc_amd.glue.phase_vocoder(*(torch.from_numpy(v).to(gpu) for v in (a, b, fo, fi))).cpu().numpy()
        rows.append(("n %d %s" % (n, case), got, (r32, r64)))
    return rows


@pytest.mark.parametrize("n", gc.PV_EDGE_SIZES)
def test_phase_vocoder_edge_sizes(n, gpu):
    """Measured on an MI355X (profiles/glue_edges_parity.json)."""
    for what, got, (r32, r64) in run_phase_vocoder(gpu, n):
        gc.pv_check(n, got, r32, r64)


def test_phase_vocoder_refuses_one_over_the_size_limit(gpu):
    import rvc_amd
    from rvc_amd import _lib

    n = gc.PV_MAX_N + 1
    a = torch.zeros(n, device=gpu)
    out = torch.full((n,), -7.0, device=gpu)
    scratch = torch.zeros(3 * (n // 2 + 1), device=gpu, dtype=torch.float64)
    with torch.cuda.device(gpu):
        rc = _lib.lib().rvcmi_glue_phase_vocoder(_lib.ptr(a), _lib.ptr(a), _lib.ptr(a), _lib.ptr(a), n, _lib.ptr(out), _lib.ptr(scratch), _lib.stream_ptr(gpu))
    torch.cuda.synchronize(gpu)
    assert rc == _lib.ERR_INVALID and bool((out == -7.0).all()) and not bool(scratch.any())
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.glue.phase_vocoder(a, a, a, a)
