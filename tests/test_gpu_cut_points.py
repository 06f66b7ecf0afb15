"""The quiet-point search that cuts a long input (infer/modules/vc/pipeline.py:219-236) on the device: ``glue.cut_points`` against
the fixtures of tools/make_golden_cuts.py (the reference's own statements, executed), and its use in the rebound pipeline.

Tolerance: none.  Every window sum is the same 160 IEEE fp64 additions in the same order as numpy's passes, so the sums are
compared as bit patterns (int64 views / sha256 of the bytes) and the cuts with ``torch.equal``."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import cut_cases
from conftest import load_golden
from make_golden_cuts import sha, small_input
from oracle import nsf_oracle, synth
from test_gpu_dropin import make_cpt, rvc_tree  # noqa: F401  (the skeleton-checkout fixture and the synthetic checkpoint)

pytestmark = pytest.mark.gpu
W, TC, TQ = 160, 4000, 1100  # the small geometry of the fixture's tie / end cases: search window [2900, 5100) = three kernel tiles


def valid_sums(c, sums):
    """[cuts, 2 t_query] device sums -> what numpy's slices hold: every row up to the end of the signal, concatenated."""
    rows = [sums[i, :ln] for i, ln in enumerate(c.lengths())]
    return torch.cat(rows).cpu().numpy() if rows else np.zeros(0)


@pytest.mark.parametrize("name", cut_cases.names())
def test_cuts_and_window_sums_equal_the_reference_bit_for_bit(name, gpu, monkeypatch):
    import rvc_amd
    import rvc_amd.pipeline as rp

    c = cut_cases.load(name)
    state = c.state()
    # as the pipeline asks: the reference's condition first, then the device search; the host loop must not be what answers
    calls = []
    real = rvc_amd.glue.cut_points
    monkeypatch.setattr(rvc_amd.glue, "cut_points", lambda *a, **k: (calls.append(a[1:]), real(*a, **k))[1])
    if c.searched():
        monkeypatch.setattr(rp, "_cut_points", lambda *a: pytest.fail("host loop ran"))
    opt_ts, a64 = rp._file_cuts(state, c.audio, gpu)
    assert opt_ts == c.opt_ts
    if not c.searched():
        assert calls == [] and a64 is None and c.opt_ts == []  # at the threshold: no cuts and no call
        return
    assert calls == [(c.window, c.t_center, c.t_query)]
    assert a64.dtype == torch.float64 and np.array_equal(a64.cpu().numpy().view(np.int64), c.audio.view(np.int64))
    cuts, sums = real(a64, c.window, c.t_center, c.t_query, return_sums=True)
    assert cuts.dtype == torch.int64 and torch.equal(cuts.cpu(), torch.tensor(c.opt_ts, dtype=torch.int64))
    assert sums.shape == (len(c.opt_ts), 2 * c.t_query)
    got = valid_sums(c, sums)
    if c.sums is not None:
        bad = np.nonzero(got.view(np.int64) != c.sums.view(np.int64))[0]
        assert bad.size == 0, "%d window sums differ in their bits, first at %d: %r vs %r" % (bad.size, bad[0], got[bad[0]], c.sums[bad[0]])
    assert sha(got) == c.sums_sha256, "the window sums are not the reference's, bit for bit"
    # beyond the end of the signal nothing is written (the wrapper's NaN fill stays)
    for i, ln in enumerate(c.lengths()):
        assert bool(torch.isnan(sums[i, ln:]).all())


def test_graph_replay_other_stream_and_repeat_give_the_same_bits(gpu):
    import rvc_amd

    a = cut_cases.load("zeros_in_tile")
    b = cut_cases.load("min_at_last")
    assert (a.n, a.window, a.t_center, a.t_query) == (b.n, b.window, b.t_center, b.t_query)
    xa, xb = torch.from_numpy(a.audio).to(gpu), torch.from_numpy(b.audio).to(gpu)
    c1, s1 = rvc_amd.glue.cut_points(xa, a.window, a.t_center, a.t_query, return_sums=True)
    c2, s2 = rvc_amd.glue.cut_points(xa, a.window, a.t_center, a.t_query, return_sums=True)
    assert c1.tolist() == a.opt_ts and torch.equal(c1, c2) and torch.equal(s1.view(torch.int64), s2.view(torch.int64))
    # a non-default stream
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        c3, s3 = rvc_amd.glue.cut_points(xa, a.window, a.t_center, a.t_query, return_sums=True)
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize(gpu)
    assert torch.equal(c3, c1) and torch.equal(s3.view(torch.int64), s1.view(torch.int64))
    # captured once, replayed on another input of the same geometry
    x = xa.clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cg, sg = rvc_amd.glue.cut_points(x, a.window, a.t_center, a.t_query, return_sums=True)
    x.copy_(xb)
    g.replay()
    torch.cuda.synchronize(gpu)
    assert cg.tolist() == b.opt_ts
    assert sha(valid_sums(b, sg)) == b.sums_sha256
    x.copy_(xa)
    g.replay()
    torch.cuda.synchronize(gpu)
    assert torch.equal(cg, c1) and torch.equal(sg.view(torch.int64), s1.view(torch.int64))


def test_invalid_arguments_are_refused_and_launch_nothing(gpu):
    import rvc_amd

    L = rvc_amd._lib.lib()
    x = torch.from_numpy(small_input(11, 9000)).to(gpu)
    cuts = torch.full((8,), -7, device=gpu, dtype=torch.int64)
    scratch = torch.zeros(4096, device=gpu, dtype=torch.uint8)
    st = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for n, w, tc, tq, room in ((9000, 161, TC, TQ, 8), (9000, 0, TC, TQ, 8), (9000, 1026, TC, TQ, 8), (160, 160, 100, 50, 8),
                               (9000, W, TC, TC + 1, 8), (9000, W, TC, TQ, 1)):
        rc = L.rvcmi_glue_cut_points(p(x), n, w, tc, tq, p(cuts), room, C.c_void_p(None), p(scratch), st)
        assert rc == rvc_amd._lib.ERR_INVALID, (n, w, tc, tq, room)
    torch.cuda.synchronize(gpu)
    assert bool((cuts == -7).all()) and bool((scratch == 0).all())
    for w, tc, tq in ((161, TC, TQ), (1026, TC, TQ), (W, TC, TC + 1)):
        with pytest.raises(rvc_amd.RvcmiError) as e:
            rvc_amd.glue.cut_points(x, w, tc, tq)
        assert e.value.code == rvc_amd._lib.ERR_INVALID
    with pytest.raises(TypeError):
        rvc_amd.glue.cut_points(x.float(), W, TC, TQ)
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.glue.cut_points(x.cpu(), W, TC, TQ)
    # the largest window the staging holds is served, and still equals the host loop
    state = types.SimpleNamespace(window=1024, t_center=TC, t_query=TQ, t_max=0)
    import rvc_amd.pipeline as rp

    host = rp._cut_points(state, x.cpu().numpy(), np.pad(x.cpu().numpy(), (512, 512), mode="reflect"))
    assert rvc_amd.glue.cut_points(x, 1024, TC, TQ).tolist() == host


def test_nan_divergence_is_the_documented_one(gpu):
    """The reference raises IndexError as soon as a search window holds a NaN sum (``seg == seg.min()`` is all False).  An
    enqueue-only call cannot raise on data: a NaN is never the minimum, and a window of nothing but NaN yields its first position."""
    import rvc_amd
    import rvc_amd.pipeline as rp

    state = types.SimpleNamespace(window=W, t_center=TC, t_query=TQ, t_max=0)
    a = small_input(12, 9000)
    a[3000] = np.nan  # the 160 sums whose window holds it are NaN; the rest of both search windows is untouched
    pad = np.pad(a, (W // 2, W // 2), mode="reflect")
    with pytest.raises(IndexError):
        rp._cut_points(state, a, pad)
    audio_sum = np.zeros_like(a)
    for i in range(W):
        audio_sum += np.abs(pad[i: i - W])
    assert np.isnan(audio_sum[2921:3081]).all() and int(np.isnan(audio_sum).sum()) == 160
    want = [t - TQ + int(np.nanargmin(audio_sum[t - TQ: t + TQ])) for t in (4000, 8000)]  # first minimum of the sums that are numbers
    assert rvc_amd.glue.cut_points(torch.from_numpy(a).to(gpu), W, TC, TQ).tolist() == want
    a = small_input(13, 9000)
    a[2700:5300] = np.nan  # the whole first window
    b = a.copy()
    b[2700:5300] = 1.0
    want2 = rp._cut_points(state, b, np.pad(b, (W // 2, W // 2), mode="reflect"))[1]
    assert rvc_amd.glue.cut_points(torch.from_numpy(a).to(gpu), W, TC, TQ).tolist() == [TC - TQ, want2]


def test_pipeline_cuts_long_files_on_the_device_and_nothing_moves(rvc_tree, gpu, tmp_path, monkeypatch):  # noqa: F811
    """The rebound ``Pipeline.pipeline`` (skeleton ``Pipeline``, FakeHubert / FakeRMVPE, an index file, rms_mix_rate 0.25) on a
    four-segment input: with the device search (the host ``_cut_points`` patched to raise) the waveform equals, bit for bit, the one
    under ``RVCMI_DEVICE_CUTS=0``; ``glue.cut_points`` runs once per long file and not at all for a file under ``t_max``;
    ``t_query > t_center`` takes the host path; ``change_rms`` gets the same float32 signal from the shared upload as from its own."""
    import rvc_amd
    import rvc_amd.pipeline as rp
    from oracle import ivf_oracle as io

    d = load_golden("pipeline_v2_48k_webui")
    seed = int(d["seed"])
    cfg = nsf_oracle.CONFIGS["v2_48k"]
    rvc_amd.install(device=gpu, operand="fp16")
    import infer.modules.vc.pipeline as pl
    import rvc.synthesizer as rs

    net_g, _ = rs.get_synthesizer(make_cpt(seed), gpu)
    config = types.SimpleNamespace(device=gpu, **{k[4:]: (bool(d[k]) if k == "cfg_is_half" else int(d[k])) for k in d if k.startswith("cfg_")})
    pipe = pl.Pipeline(cfg.sr, config)
    assert pipe.t_max == 16000 and pipe.t_query == pipe.t_center == 16000
    pipe.f0_gen = types.SimpleNamespace(rmvpe=synth.FakeRMVPE(gpu, seed), is_half=False, device=gpu)
    path = str(tmp_path / "added.index")
    io.write_index(synth.make_ivf(int(d["index_n"]), int(d["index_d"]), seed=int(d["index_seed"])), path)
    hub = synth.FakeHubert(768, seed)
    tail = (int(d["f0_up_key"]), "rmvpe", path, float(d["index_rate"]), 1, int(d["filter_radius"]), cfg.sr, 0, 0.25, "v2", float(d["protect"]))
    long_a, short_a = synth.make_audio16k(50000, seed + 4), synth.make_audio16k(15000, seed + 5)

    cut_calls, rms_in, host_calls = [], [], []
    real_cut, real_rms, real_host = rvc_amd.glue.cut_points, rvc_amd.glue.change_rms, rp._cut_points
    monkeypatch.setattr(rvc_amd.glue, "cut_points", lambda *a, **k: (cut_calls.append(int(a[0].numel())), real_cut(*a, **k))[1])
    monkeypatch.setattr(rvc_amd.glue, "change_rms", lambda *a: (rms_in.append(a[0].clone()), real_rms(*a))[1])

    def convert(a):
        torch.manual_seed(5)
        return pipe.pipeline(hub, net_g, int(d["sid"]), a.copy(), [0, 0, 0], *tail)

    # the host loop (and change_rms's own float32 upload)
    monkeypatch.setenv("RVCMI_DEVICE_CUTS", "0")
    hub.calls = 0
    host_out = convert(long_a)
    assert hub.calls == 4 and cut_calls == []
    # the device search; the host loop must not run
    monkeypatch.delenv("RVCMI_DEVICE_CUTS")
    monkeypatch.setattr(rp, "_cut_points", lambda *a: pytest.fail("the host loop ran for a long file"))
    hub.calls = 0
    dev_out = convert(long_a)
    assert hub.calls == 4 and cut_calls == [50000]
    assert dev_out.shape == host_out.shape and np.array_equal(dev_out, host_out)
    assert len(rms_in) == 2 and rms_in[0].dtype == rms_in[1].dtype == torch.float32 and torch.equal(rms_in[0], rms_in[1])
    # several files: one call per long file, before the batch is formed
    del cut_calls[:]
    monkeypatch.setattr(rp, "_cut_points", real_host)
    torch.manual_seed(5)
    outs = pipe.convert_files(hub, net_g, int(d["sid"]), [long_a.copy(), short_a.copy(), long_a.copy()], [0, 0, 0], *tail)
    assert cut_calls == [50000, 50000] and len(outs) == 3
    # a file under t_max: no call
    del cut_calls[:]
    convert(short_a)
    assert cut_calls == []
    # t_query > t_center: the kernel refuses it, the pipeline asks the host (numpy's negative slice start wraps there, so the host
    # answer for this input is the reference's own error; a recording stand-in returns the cuts of the regular geometry instead)
    good = real_host(pipe, *(lambda f: (f, np.pad(f, (80, 80), mode="reflect")))(pl.signal.filtfilt(pl.bh, pl.ah, long_a)))
    monkeypatch.setattr(rp, "_cut_points", lambda *a: (host_calls.append(1), good)[1])
    pipe.t_query = pipe.t_center + 1
    out_q = convert(long_a)
    assert host_calls == [1] and cut_calls == [] and np.array_equal(out_q, host_out)
