"""The input preparation of ``Pipeline.pipeline`` on the device: ``glue.filtfilt`` (scipy.signal.filtfilt with scipy's defaults,
infer/modules/vc/pipeline.py:23,221) against scipy and against the exact values of tools/make_golden_prep.py, and the rebound
pipeline with ``RVCMI_DEVICE_PREP=1``.

Tolerances.  Inputs of at most ``glue.filtfilt_exact_len`` samples: none, int64 bit patterns.  Longer inputs cannot equal scipy bit for
bit (the recurrence has five poles of radius 0.981 .. 0.994; any two fp64 evaluation orders end about 5e-8 apart), so they are
compared with the EXACT result (np.longdouble, stored rounded to fp64): max|device - exact| <= 2 x max|scipy - exact| over the
fixture's positions, scipy's deviation computed here.  The factor 2: an independent fp64 evaluation has scipy's own noise level, and
its maximum over a file varied between 0.77x and 1.28x scipy's on the CPU model of the kernel; 2x keeps that spread out of the test
and still fails anything that loses a digit."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
from scipy import signal

import prep_cases
from conftest import load_golden, rms
from oracle import nsf_oracle, synth
from test_gpu_dropin import _CpuSpy, _pipeline_fixture, make_cpt, rvc_tree  # noqa: F401  (skeleton checkout, synthetic checkpoint)

pytestmark = pytest.mark.gpu
BH, AH = signal.butter(N=5, Wn=48, btype="high", fs=16000)
SR = 16000


def bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int64)


def seeded(n, seed, dtype):
    rng = np.random.default_rng(seed)
    return (0.3 * rng.standard_normal(n) + 0.05 + 0.2 * np.sin(np.arange(n) * 0.07)).astype(dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_inputs_that_fit_one_lane_equal_scipy_bit_for_bit(dtype, gpu):
    """From ``padlen + 1`` samples up to ``filtfilt_exact_len`` every thread starts at sample 0 from scipy's own initial state: the
    result equals ``scipy.signal.filtfilt`` as int64 bit patterns, float32 and float64 inputs, alone and inside a ragged batch.  Also
    for another filter order, for exact zeros (the signs of zeros included) and for the optional reflection pad (a pure copy)."""
    from rvc_amd import glue

    top = glue.filtfilt_exact_len(BH, AH)
    assert top == glue.filt_warmup(AH) + glue.FILT_LANE - 36
    lengths = [19, 20, 37, 100, 1023, 1024, 1025, 4097, 9000, top - 1, top]
    xs = [seeded(n, 100 + i, dtype) for i, n in enumerate(lengths)]
    xs[3][:] = 0.0
    xs[4][100:600] = 0.0
    want = [signal.filtfilt(BH, AH, x) for x in xs]
    devx = [torch.from_numpy(x).to(gpu) for x in xs]
    for x, w, n in zip(devx, want, lengths):
        got = glue.filtfilt(x, BH, AH)
        assert got.dtype == torch.float64 and got.shape == (n,)
        bad = np.nonzero(bits(got) != bits(w))[0]
        assert bad.size == 0, "n = %d: %d samples differ from scipy, first at %d: %r vs %r" % (n, bad.size, bad[0], float(got[bad[0]]), w[bad[0]])
    batch = glue.filtfilt(devx, BH, AH)
    assert len(batch) == len(xs)
    for got, w, n in zip(batch, want, lengths):
        assert np.array_equal(bits(got), bits(w)), "n = %d inside the ragged batch" % n
    # highpass16k is that filter
    assert np.array_equal(bits(glue.highpass16k(devx[7])), bits(want[7]))
    # another order (8) and a filter with len(b) != len(a)
    for b, a in (signal.butter(8, 0.1, "high"), ([0.5, 0.25], [2.0, -1.0, 0.25]), signal.butter(1, 0.3)):
        n = min(glue.filtfilt_exact_len(b, a), 6000)
        x = seeded(n, 7, dtype)
        assert np.array_equal(bits(glue.filtfilt(torch.from_numpy(x).to(gpu), b, a)), bits(signal.filtfilt(b, a, x)))
    # the reflection pad
    y, yp = glue.filtfilt(devx[8], BH, AH, reflect_pad=3000)
    assert np.array_equal(bits(y), bits(want[8])) and np.array_equal(bits(yp), bits(np.pad(want[8], (3000, 3000), mode="reflect")))


@pytest.mark.parametrize("name", prep_cases.names())
def test_multi_lane_inputs_are_as_close_to_the_exact_result_as_scipy_is(name, gpu):
    """max|device - exact| <= 2 x max|scipy - exact| at the fixture's positions (module docstring).  Measured on the MI355X
    (device / scipy, each in units of 1e-8; the ratio): tone_noise_dc_5s 3.015 / 2.363 = 1.28, zeros_stretch_7s 2.298 / 1.994 = 1.15,
    int16_quantised_4s 2.381 / 2.695 = 0.88, envelope_80s 2.588 / 2.108 = 1.23, int16_envelope_72s 2.503 / 2.549 = 0.98 -- the device
    values are, bit for bit, those of the CPU model of the kernel (tools/make_golden_prep.py ``lane_model``)."""
    from rvc_amd import glue

    c = prep_cases.load(name)
    assert c.x.shape[0] // glue.FILT_LANE >= 8 and c.x.shape[0] > glue.filtfilt_exact_len(c.b, c.a)
    sp = signal.filtfilt(c.b, c.a, c.x)
    dev = glue.filtfilt(torch.from_numpy(c.x).to(gpu), c.b, c.a).cpu().numpy()
    e_sp = float(np.abs(sp[c.idx] - c.exact).max())
    e_dev = float(np.abs(dev[c.idx] - c.exact).max())
    print("PREP_ACCURACY %s n %d %s scipy-exact %.4e device-exact %.4e ratio %.3f device-scipy %.4e" % (
        name, c.x.shape[0], c.x.dtype, e_sp, e_dev, e_dev / e_sp, float(np.abs(dev - sp).max())))
    assert 0 < e_sp < 1e-7, "scipy itself is %.3e from the exact values: the fixture does not describe this input" % e_sp
    assert e_dev <= 2 * e_sp, "device %.4e from the exact result, scipy %.4e: ratio %.2f > 2" % (e_dev, e_sp, e_dev / e_sp)


def _raw_call(gpu, xs, pad, guard=4096):
    """rvcmi_glue_filtfilt straight through the C ABI on NaN-filled buffers with guard bands.  -> (out, out_pad, scratch) whole."""
    import rvc_amd
    from rvc_amd import glue

    bn, an, zi, order, padlen, warm = glue._filt_plan(BH, AH)
    L = rvc_amd._lib.lib()
    lengths = [int(x.numel()) for x in xs]
    total, B = sum(lengths), len(xs)
    flat = torch.cat(xs)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(lengths)]), dtype=torch.int64, device=gpu)
    nan = float("nan")
    out = torch.full((total + 2 * guard,), nan, device=gpu, dtype=torch.float64)
    out_pad = torch.full((total + 2 * pad * B + 2 * guard,), nan, device=gpu, dtype=torch.float64)
    nbytes = int(L.rvcmi_glue_filtfilt_scratch_bytes(B, total, order))
    scratch = torch.full((nbytes // 8 + 2 * guard,), nan, device=gpu, dtype=torch.float64)
    p = lambda t, o=0: C.c_void_p(t.data_ptr() + 8 * o)  # noqa: E731
    d = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    rvc_amd._lib.check(L.rvcmi_glue_filtfilt(p(flat), 1 if flat.dtype == torch.float64 else 0, p(offsets), B, max(lengths), total, d(bn), d(an),
                                             d(zi), order, warm, p(out, guard), p(out_pad, guard) if pad else None, pad, p(scratch, guard),
                                             nbytes, C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
    torch.cuda.synchronize(gpu)
    return out, out_pad, scratch, lengths


def test_a_batch_equals_separate_calls_runs_repeat_and_nothing_is_written_outside(gpu):
    from rvc_amd import glue

    lengths = [50000, 19, 13001, 160000, 12253, 2048, 33333]
    pad, guard = 16000, 4096
    for dtype in (np.float32, np.float64):
        xs = [torch.from_numpy(seeded(n, 40 + i, dtype)).to(gpu) for i, n in enumerate(lengths)]
        alone = [glue.filtfilt(x, BH, AH) for x in xs]
        batch = glue.filtfilt(xs, BH, AH)
        again = glue.filtfilt(xs, BH, AH)
        for i, n in enumerate(lengths):
            assert np.array_equal(bits(batch[i]), bits(alone[i])), "item %d (n = %d) differs between the batch and its own call" % (i, n)
            assert np.array_equal(bits(again[i]), bits(batch[i])), "item %d differs between two runs" % i
            assert bool(torch.isfinite(batch[i]).all())
        # guard bands: out, the padded output and the scratch are written inside their ranges only
        big = [x for x in xs if x.numel() > pad]
        out, out_pad, scratch, lens = _raw_call(gpu, big, pad, guard)
        total, B = sum(lens), len(lens)
        for buf, used in ((out, total), (out_pad, total + 2 * pad * B), (scratch, total + 36 * B)):
            assert bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + used:]).all()), "a write outside the buffer's range"
            assert bool(torch.isfinite(buf[guard: guard + used]).all())
        o = 0
        for i, x in enumerate(big):
            n = lens[i]
            y = out[guard + o: guard + o + n]
            assert np.array_equal(bits(y), bits(alone[lengths.index(n)]))
            yp = out_pad[guard + o + 2 * pad * i: guard + o + n + 2 * pad * (i + 1)]
            assert np.array_equal(bits(yp), bits(torch.nn.functional.pad(y[None, None], (pad, pad), mode="reflect")[0, 0]))
            o += n
        # an item not longer than the pad: its padded range is left alone, everything else is written
        out, out_pad, _, lens = _raw_call(gpu, [xs[0], xs[2]], pad, guard)
        assert bool(torch.isfinite(out_pad[guard: guard + 50000 + 2 * pad]).all())
        assert bool(torch.isnan(out_pad[guard + 50000 + 2 * pad:]).all()) and bool(torch.isfinite(out[guard: guard + 63001]).all())


@pytest.mark.parametrize("name", prep_cases.long_names())
def test_cuts_of_the_long_inputs_are_those_of_the_scipy_filtered_signal(name, gpu):
    """``glue.cut_points`` on the device-filtered signal finds the positions the host loop finds on the scipy-filtered one (x_center
    38, x_query 6).  This is a property of THESE inputs, verified on the CPU model when the fixture was made, not a guarantee: the
    two signals differ by about 5e-8, and a near-tie between two window sums could move a cut to another, equally quiet, sample."""
    import rvc_amd.pipeline as rp
    from rvc_amd import glue

    c = prep_cases.load(name)
    w, tc, tq, tm = prep_cases.CUT_GEOMETRY
    sp = signal.filtfilt(c.b, c.a, c.x)
    state = types.SimpleNamespace(window=w, t_center=tc, t_query=tq, t_max=tm)
    host = rp._cut_points(state, sp, np.pad(sp, (w // 2, w // 2), mode="reflect"))
    assert host == c.cuts and len(host) >= 1
    dev = glue.filtfilt(torch.from_numpy(c.x).to(gpu), c.b, c.a)
    assert glue.cut_points(dev, w, tc, tq).tolist() == host
    # ... and through the pipeline's own helper, which takes the device tensor as it is (no upload, no host loop)
    opt_ts, a64 = rp._file_cuts(state, dev, gpu)
    assert opt_ts == host and a64.data_ptr() == dev.data_ptr()


def test_device_casts_round_as_the_host_casts(gpu):
    """fp64 -> fp32 and fp64 -> fp16 on the device give the bits of ``torch.as_tensor(numpy_f64).float()`` / ``.half()`` on the host
    (what ``hubert_device`` / ``change_rms`` did to the host-filtered signal).  The fp16 inputs include values just above a tie of the
    fp16 grid by less than fp32 resolves: rounding through fp32 and rounding directly differ there."""
    rng = np.random.default_rng(3)
    g = rng.standard_normal(20000).astype(np.float16).astype(np.float64)
    ulp = np.spacing(g.astype(np.float16)).astype(np.float64)
    v = np.concatenate([g + 0.5 * np.abs(ulp) * (1 + 2.0 ** -30), g - 0.5 * np.abs(ulp) * (1 + 2.0 ** -30), rng.standard_normal(20000) * 0.3,
                        rng.standard_normal(1000) * 1e-6])
    host = torch.as_tensor(v)
    dev = host.to(gpu)
    assert torch.equal(host.half().view(torch.int16), dev.half().cpu().view(torch.int16))
    assert torch.equal(host.float().view(torch.int32), dev.float().cpu().view(torch.int32))


def _fail(what):
    def f(*a, **k):
        pytest.fail(what + " ran")
    return f


def test_pipeline_with_the_switch_on_meets_the_reference_and_the_host_prepares_nothing(rvc_tree, gpu, tmp_path, monkeypatch):  # noqa: F811
    """``Pipeline.pipeline`` on the fixture of the REAL reference (pipeline_v2_48k_3seg) with ``RVCMI_DEVICE_PREP=1``: within the
    suite's 1e-3 RMS bar, three HuBERT calls, ``signal.filtfilt`` and ``np.pad`` never run, and exactly one tensor -- the finished
    audio -- crosses to the host."""
    from rvc_amd import glue

    import rvc_amd.pipeline as rp

    d, cfg, pl, pipe, net_g, audio, pitch, pitchf = _pipeline_fixture(gpu, rvc_tree, tmp_path)
    monkeypatch.setenv("RVCMI_DEVICE_PREP", "1")
    # 2.4 s of audio is below the length from which the device filter is the faster one: left to itself the pipeline prepares this
    # input on the host even with the switch on.  The threshold is a speed choice, not part of the arithmetic, and is pinned to 0
    # here like the kernel families elsewhere in the suite.
    assert audio.shape[0] < rp.DEVICE_PREP_MIN_SAMPLES and rp._device_prep(pipe, [audio], gpu) == [None]
    monkeypatch.setattr(rp, "DEVICE_PREP_MIN_SAMPLES", 0)
    calls = []
    real = glue.filtfilt_flat
    monkeypatch.setattr(glue, "filtfilt_flat", lambda flat, lengths, *a, **k: (calls.append((flat.dtype, list(lengths))), real(flat, lengths, *a, **k))[1])
    monkeypatch.setattr(pl.signal, "filtfilt", _fail("signal.filtfilt"))
    monkeypatch.setattr(np, "pad", _fail("np.pad"))
    spy = _CpuSpy(monkeypatch)
    hub = synth.FakeHubert(768, int(d["seed"]))
    times = [0, 0, 0]
    out = pipe.pipeline(hub, net_g, int(d["sid"]), audio.copy(), times, 0, (pitch, pitchf), "", 0.75, 2, 3, cfg.sr, 0, 1, "v2", float(d["protect"]))
    assert calls == [(torch.from_numpy(audio[:1]).dtype, [audio.shape[0]])]  # uploaded once, in its own dtype, one call
    assert hub.calls == 3 and isinstance(out, np.ndarray) and out.shape == d["out"].shape
    assert spy.calls == [tuple(d["out"].shape)], "host hops: %s" % spy.calls
    e = rms(out / 32768.0, d["out"] / 32768.0)
    print("PREP_PIPELINE 3seg RMS %.3e" % e)
    assert e <= 1e-3, "Pipeline.pipeline with the device preparation: RMS %.3e vs the reference" % e


def _webui_pipe(gpu, tmp_path, device_prep=False, **cfg_over):
    import rvc_amd
    from oracle import ivf_oracle as io

    d = load_golden("pipeline_v2_48k_webui")
    seed = int(d["seed"])
    cfg = nsf_oracle.CONFIGS["v2_48k"]
    rvc_amd.install(device=gpu, operand="fp16", device_prep=device_prep)
    import infer.modules.vc.pipeline as pl
    import rvc.synthesizer as rs

    net_g, _ = rs.get_synthesizer(make_cpt(seed), gpu)
    config = types.SimpleNamespace(device=gpu, **{k[4:]: (bool(d[k]) if k == "cfg_is_half" else int(d[k])) for k in d if k.startswith("cfg_")})
    for k, v in cfg_over.items():
        setattr(config, k, v)
    pipe = pl.Pipeline(cfg.sr, config)
    fake = synth.FakeRMVPE(gpu, seed)
    pipe.f0_gen = types.SimpleNamespace(rmvpe=fake, is_half=False, device=gpu)  # no ``calculate``: a host estimator would raise
    path = str(tmp_path / "added.index")
    io.write_index(synth.make_ivf(int(d["index_n"]), int(d["index_d"]), seed=int(d["index_seed"])), path)
    tail = (int(d["f0_up_key"]), "rmvpe", path, float(d["index_rate"]), 1, int(d["filter_radius"]), cfg.sr, 0, 0.25, "v2", float(d["protect"]))
    return d, seed, pl, pipe, net_g, tail


def test_long_input_with_the_switch_on_is_cut_where_the_host_prepared_one_is(rvc_tree, gpu, tmp_path, monkeypatch):  # noqa: F811
    """A four-segment input through ``pipeline_hip``: ``install(device_prep=True)`` gives the cut list of the default (host
    ``filtfilt``) run and a waveform within the 1e-3 bar of it; with the switch on the host filter, ``np.pad`` and the host cut loop
    never run, RMVPE and ``change_rms`` read the device signal, and one tensor crosses to the host.  ``RVCMI_DEVICE_PREP=0``
    overrides the installed switch."""
    import rvc_amd
    import rvc_amd.pipeline as rp
    from rvc_amd import glue

    d, seed, pl, pipe, net_g, tail = _webui_pipe(gpu, tmp_path, device_prep=True)
    assert rp.DEVICE_PREP is True
    monkeypatch.setattr(rp, "DEVICE_PREP_MIN_SAMPLES", 0)  # (a 3 s input: below the length from which the device filter is faster)
    long_a = synth.make_audio16k(50000, seed + 4)
    hub = synth.FakeHubert(768, seed)
    cuts, filt = [], []
    real_cut, real_filt = glue.cut_points, glue.filtfilt_flat
    monkeypatch.setattr(glue, "cut_points", lambda *a, **k: (lambda r: (cuts.append(r.tolist()), r)[1])(real_cut(*a, **k)))
    monkeypatch.setattr(glue, "filtfilt_flat", lambda *a, **k: (filt.append(1), real_filt(*a, **k))[1])

    def convert():
        torch.manual_seed(5)
        hub.calls = 0
        return pipe.pipeline(hub, net_g, int(d["sid"]), long_a.copy(), [0, 0, 0], *tail)

    monkeypatch.setenv("RVCMI_DEVICE_PREP", "0")
    off = convert()
    assert hub.calls == 4 and filt == [] and len(cuts) == 1 and len(cuts[0]) == 3
    monkeypatch.delenv("RVCMI_DEVICE_PREP")
    monkeypatch.setattr(pl.signal, "filtfilt", _fail("signal.filtfilt"))
    monkeypatch.setattr(rp, "_cut_points", _fail("the host cut loop"))
    real_pad = np.pad
    monkeypatch.setattr(np, "pad", _fail("np.pad"))
    spy = _CpuSpy(monkeypatch)
    on = convert()
    monkeypatch.setattr(np, "pad", real_pad)
    assert hub.calls == 4 and filt == [1] and len(cuts) == 2
    assert cuts[1] == cuts[0], "the device-prepared signal is cut at %s, the host-prepared one at %s" % (cuts[1], cuts[0])
    assert spy.calls == [tuple(on.shape)], "host hops: %s" % spy.calls
    e = rms(on / 32768.0, off / 32768.0)
    print("PREP_PIPELINE long on-vs-off RMS %.3e" % e)
    assert on.shape == off.shape and e <= 1e-3
    rvc_amd.uninstall()
    assert rp.DEVICE_PREP is False


def test_convert_files_with_the_switch_on_equals_the_per_file_pipeline_bit_for_bit(rvc_tree, gpu, tmp_path, monkeypatch):  # noqa: F811
    """Five files (one to four segments, one shorter than ``t_pad``, which the host prepares) through ``convert_files`` with
    ``RVCMI_DEVICE_PREP=1``: ONE filter call for the whole group, and every waveform is bit-equal to ``Pipeline.pipeline`` for that
    file alone with the switch on (kernel families pinned as in the convert_files test of test_gpu_dropin.py)."""
    from rvc_amd import glue

    d, seed, pl, pipe, net_g, tail = _webui_pipe(gpu, tmp_path)
    for key, val in (("RB_STREAM", 0), ("NO_RB_SPLIT", 1)):
        net_g.dec.set_option(key, val)
    for key, val in (("FR_NJ", 1), ("FR_FFN_SPLIT", 1), ("FR_WN_SPLIT", 1)):
        net_g._rvcmi_front.set_option(key, val)
    import rvc_amd.pipeline as rp

    monkeypatch.setenv("RVCMI_DEVICE_PREP", "1")
    monkeypatch.setattr(rp, "DEVICE_PREP_MIN_SAMPLES", 0)
    n0 = int(d["n_audio"])
    audios = [synth.make_audio16k(n0, seed), synth.make_audio16k(16000 * 2 + 77, seed + 1), synth.make_audio16k(pipe.t_pad - 100, seed + 2),
              synth.make_audio16k(pipe.t_pad + 1, seed + 3), synth.make_audio16k(50000, seed + 4)]
    hub = synth.FakeHubert(768, seed)
    filt = []
    real_filt = glue.filtfilt_flat
    monkeypatch.setattr(glue, "filtfilt_flat", lambda flat, lengths, *a, **k: (filt.append(list(lengths)), real_filt(flat, lengths, *a, **k))[1])
    torch.manual_seed(5)
    seq = [pipe.pipeline(hub, net_g, int(d["sid"]), a.copy(), [0, 0, 0], *tail) for a in audios]
    served = [a.shape[0] for a in audios if a.shape[0] > pipe.t_pad]
    assert filt == [[n] for n in served] and len(served) == 4
    del filt[:]
    torch.manual_seed(5)
    bat = pipe.convert_files(hub, net_g, int(d["sid"]), [a.copy() for a in audios], [0, 0, 0], *tail)
    assert filt == [served], "the group was filtered in %d calls: %s" % (len(filt), filt)
    for i, (o, r) in enumerate(zip(bat, seq)):
        assert o.shape == r.shape and np.array_equal(o, r), "file %d: batched vs per-file max diff %g" % (i, float(np.abs(o - r).max()))


def test_inputs_under_t_max_with_the_switch_on_never_visit_the_host(rvc_tree, gpu, tmp_path, monkeypatch):  # noqa: F811
    """The common case: a clip that is not cut at all (x_max 3: ``n + window <= t_max``).  With the switch on it is filtered and padded
    on the device, ``_file_cuts`` answers ``[]`` without touching it, and nothing but the finished audio crosses to the host -- for
    ``Pipeline.pipeline`` and for every file of a ``convert_files`` group (one filter call for the group).  ``signal.filtfilt``,
    ``np.pad``, the host cut loop and the device cut search are patched to fail."""
    import rvc_amd.pipeline as rp
    from rvc_amd import glue

    d, seed, pl, pipe, net_g, tail = _webui_pipe(gpu, tmp_path, x_center=2, x_max=3)
    assert pipe.t_max == 48000 and pipe.t_pad == 16000
    monkeypatch.setenv("RVCMI_DEVICE_PREP", "1")
    monkeypatch.setattr(rp, "DEVICE_PREP_MIN_SAMPLES", 0)
    audios = [synth.make_audio16k(n, seed + 1 + i) for i, n in enumerate((30000, 20000, 47000))]
    assert all(a.shape[0] > pipe.t_pad and a.shape[0] + pipe.window <= pipe.t_max for a in audios)
    x = torch.from_numpy(audios[0].astype(np.float64)).to(gpu)
    hub = synth.FakeHubert(768, seed)
    filt = []
    real_filt = glue.filtfilt_flat
    monkeypatch.setattr(glue, "filtfilt_flat", lambda flat, lengths, *a, **k: (filt.append(list(lengths)), real_filt(flat, lengths, *a, **k))[1])
    monkeypatch.setattr(pl.signal, "filtfilt", _fail("signal.filtfilt"))
    monkeypatch.setattr(rp, "_cut_points", _fail("the host cut loop"))
    monkeypatch.setattr(glue, "cut_points", _fail("the device cut search"))
    monkeypatch.setattr(np, "pad", _fail("np.pad"))
    spy = _CpuSpy(monkeypatch)
    opt_ts, a64 = rp._file_cuts(pipe, x, gpu)
    assert opt_ts == [] and a64 is x and spy.calls == []
    torch.manual_seed(5)
    one = pipe.pipeline(hub, net_g, int(d["sid"]), audios[0].copy(), [0, 0, 0], *tail)
    assert hub.calls == 1 and filt == [[30000]]
    assert spy.calls == [tuple(one.shape)], "host hops of one short file: %s" % spy.calls
    del spy.calls[:], filt[:]
    hub.calls = 0
    torch.manual_seed(5)
    bat = pipe.convert_files(hub, net_g, int(d["sid"]), [a.copy() for a in audios], [0, 0, 0], *tail)
    assert hub.calls == 3 and filt == [[30000, 20000, 47000]]
    assert spy.calls == [tuple(o.shape) for o in bat], "host hops of a group of short files: %s" % spy.calls
    assert len(bat) == 3 and all(np.isfinite(o).all() and o.shape[0] > 0 for o in bat) and bat[0].shape == one.shape


def test_switch_off_is_the_default_and_the_device_filter_never_runs(rvc_tree, gpu, tmp_path, monkeypatch):  # noqa: F811
    """Without ``install(device_prep=True)`` / ``RVCMI_DEVICE_PREP=1`` the pipeline is the parent's: ``glue.filtfilt`` /
    ``filtfilt_flat`` are patched to fail and never run, the host ``filtfilt`` does, and the reference fixture is met."""
    import rvc_amd.pipeline as rp
    from rvc_amd import glue

    d, cfg, pl, pipe, net_g, audio, pitch, pitchf = _pipeline_fixture(gpu, rvc_tree, tmp_path)
    monkeypatch.delenv("RVCMI_DEVICE_PREP", raising=False)
    assert rp.DEVICE_PREP is False and not rp._device_prep_on()
    monkeypatch.setattr(glue, "filtfilt", _fail("glue.filtfilt"))
    monkeypatch.setattr(glue, "filtfilt_flat", _fail("glue.filtfilt_flat"))
    host = []
    real = pl.signal.filtfilt
    monkeypatch.setattr(pl.signal, "filtfilt", lambda *a, **k: (host.append(1), real(*a, **k))[1])
    hub = synth.FakeHubert(768, int(d["seed"]))
    out = pipe.pipeline(hub, net_g, int(d["sid"]), audio.copy(), [0, 0, 0], 0, (pitch, pitchf), "", 0.75, 2, 3, cfg.sr, 0, 1, "v2", float(d["protect"]))
    assert host == [1] and hub.calls == 3
    assert rms(out / 32768.0, d["out"] / 32768.0) <= 1e-3
