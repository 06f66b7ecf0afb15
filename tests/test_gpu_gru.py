"""The bidirectional GRU of the RMVPE network (rvc/f0/e2e.py:50-67) on csrc/gru.hip -- beyond the SURVEY.md section 8 scope table -- against
torch's own ``nn.GRU`` in fp32 on the CPU (the plain PyTorch fp32 reference of the same op).  Tolerance: fp16 operands (x, W_ih, W_hh, the
broadcast copy of h) with fp32 accumulation and state: <= 2e-3 RMS / 1e-2 max-abs on outputs in (-1, 1).

That comparison cannot tell the kernel's design (1e-4 RMS from the operand rounding alone) from a kernel that is wrong in the fifth digit, so the
second half of this file holds ``rvcmi_gru_forward`` / ``rvcmi_gru_forward_ragged`` to the fp64 oracle WITH the operand rounding
(oracle/gru_oracle.py) at the bars derived in tests/gru_cases.py (3x / 4x the noise floor of an fp32 evaluation; tests/test_cpu_gru.py shows what
they exclude), at the shapes where the kernels take another path; the torch comparison stays as a coarse second opinion."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gru_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _pair(seed, input_size=384, gain=1.0):
    torch.manual_seed(seed)
    ref = torch.nn.GRU(input_size, 256, num_layers=1, batch_first=True, bidirectional=True).eval()
    if gain != 1.0:
        with torch.no_grad():
            for p in ref.parameters():
                p.mul_(gain)
    return ref


@pytest.mark.parametrize("B,T,seed,gain", [(1, 1, 0, 1.0), (2, 7, 1, 1.0), (1, 1216, 2, 1.0), (3, 301, 3, 2.5), (64, 40, 4, 1.0)])
def test_gru_hip_matches_torch_fp32(B, T, seed, gain, gpu):
    import rvc_amd

    ref = _pair(seed, gain=gain)
    x = torch.randn(B, T, 384, generator=torch.Generator().manual_seed(100 + seed))
    with torch.no_grad():
        y_ref, hn_ref = ref(x)
    m = rvc_amd.GRUHIP(ref, device=gpu)
    y, hn = m(x.to(gpu))
    torch.cuda.synchronize()
    assert y.shape == y_ref.shape and hn.shape == hn_ref.shape and y.dtype == torch.float32
    e = (y.cpu() - y_ref)
    rms, mx = float(e.pow(2).mean().sqrt()), float(e.abs().max())
    assert torch.isfinite(y).all() and rms <= 2e-3 and mx <= 1e-2, "B=%d T=%d gain %.1f: RMS %.3e max %.3e" % (B, T, gain, rms, mx)
    assert float((hn.cpu() - hn_ref).abs().max()) <= 1e-2
    # h_n is the last forward / first backward output row
    assert torch.equal(hn[0], y[:, -1, :256]) and torch.equal(hn[1], y[:, 0, 256:])
    # deterministic
    y2, _ = m(x.to(gpu))
    assert torch.equal(y, y2)


def test_gru_hip_half_input_and_other_input_size(gpu):
    import rvc_amd

    ref = _pair(7, input_size=64)
    x = torch.randn(2, 50, 64, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        y_ref, _ = ref(x)
    y, hn = rvc_amd.GRUHIP(ref, device=gpu)(x.to(gpu).half())
    assert y.dtype == torch.float16 and hn.dtype == torch.float16
    assert float((y.float().cpu() - y_ref).abs().max()) <= 1e-2


def test_accelerate_rmvpe_swaps_the_gru_of_the_proxy_network_only(gpu):
    """``accelerate_rmvpe`` on the architecture proxy of rvc/f0/e2e.py (tools/e2e_proxies.py): one module replaced, the salience within the
    fp16 tolerance of the all-PyTorch network; an unsupported GRU (hidden 128) is left alone; a CPU model is left alone."""
    import rvc_amd
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from e2e_proxies import _SalienceNet

    torch.manual_seed(3)
    net = _SalienceNet().eval().to(gpu)
    mel = torch.randn(1, 128, 64, device=gpu)
    with torch.no_grad():
        want = net(mel)
        assert rvc_amd.accelerate_rmvpe(net) == 1 and isinstance(net.gru, rvc_amd.GRUHIP)
        got = net(mel)
    assert got.shape == want.shape and float((got - want).abs().max()) <= 5e-3
    small = torch.nn.Sequential(torch.nn.GRU(64, 128, batch_first=True, bidirectional=True)).to(gpu)
    assert rvc_amd.accelerate_rmvpe(small) == 0 and isinstance(small[0], torch.nn.GRU)
    cpu_net = torch.nn.Sequential(torch.nn.GRU(64, 256, batch_first=True, bidirectional=True))
    assert rvc_amd.accelerate_rmvpe(cpu_net) == 0


def test_gru_hip_rejects_what_it_does_not_implement(gpu):
    import rvc_amd

    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.GRUHIP(torch.nn.GRU(384, 256, num_layers=2, batch_first=True, bidirectional=True), device=gpu)
    m = rvc_amd.GRUHIP(_pair(0), device=gpu)
    with pytest.raises(rvc_amd.RvcmiError):
        m(torch.zeros(1, 4, 384))  # CPU input: no fallback
    with pytest.raises(ValueError):
        m(torch.zeros(1, 4, 100, device=gpu))


def test_rebound_pipeline_swaps_the_gru_once_and_honours_the_opt_out(gpu, monkeypatch):
    """``pipeline._rmvpe_on_device`` (the f0 step of the rebound ``Pipeline.pipeline``): the first call swaps the network's GRU for the HIP one,
    ``RVCMI_RMVPE_GRU=0`` leaves torch's in place; both produce a pitch track of the asked length."""
    import types

    import numpy as np
    import rvc_amd
    import rvc_amd.pipeline as rp

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from e2e_proxies import RmvpeProxy

    audio = (0.3 * np.sin(2 * np.pi * 220.0 * np.arange(16000 * 2) / 16000.0)).astype(np.float32)
    p_len = audio.shape[0] // 160
    for env, want in (("0", 0), ("1", 1)):
        monkeypatch.setenv("RVCMI_RMVPE_GRU", env)
        r = RmvpeProxy(gpu, half=True)
        me = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=r, is_half=True, device=gpu))
        pitch, pitchf = rp._rmvpe_on_device(me, audio, p_len, 0)
        assert r._rvcmi_gru == want and isinstance(r.model.gru, rvc_amd.GRUHIP) == bool(want)
        assert pitch.shape[-1] == p_len and pitchf.shape[-1] == p_len and torch.isfinite(pitchf).all()
        rp._rmvpe_on_device(me, audio, p_len, 0)  # (second call: nothing left to swap)
        assert r._rvcmi_gru == want


def test_accelerate_f0_rmvpe_is_idempotent_and_tolerates_foreign_objects(gpu, monkeypatch):
    """The helper both rebound callers use (``Pipeline.pipeline`` and the realtime ``RVC.infer``): swaps once, remembers the count, leaves an
    object without a torch network alone."""
    import types

    from rvc_amd.gru import accelerate_f0_rmvpe

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from e2e_proxies import RmvpeProxy

    monkeypatch.delenv("RVCMI_RMVPE_GRU", raising=False)
    r = RmvpeProxy(gpu, half=False)
    assert accelerate_f0_rmvpe(r) == 1 and accelerate_f0_rmvpe(r) == 1 and r._rvcmi_gru == 1
    onnx_like = types.SimpleNamespace(model=object())
    assert accelerate_f0_rmvpe(onnx_like) == 0 and onnx_like._rvcmi_gru == 0


def test_realtime_f0_chain_replayed_from_a_hipgraph_equals_the_eager_chain(gpu, monkeypatch):
    """``realtime._rmvpe_f0_graphed``: the fixed-length f0 window of the realtime loop (mel STFT -> the RMVPE architecture proxy incl. the HIP
    GRU -> salience decode) is captured after three eager blocks and replayed; every replay must give what the eager chain gives for the same
    waveform (same kernels; to the network's own run-to-run noise).  ``RVCMI_RT_GRAPH=0`` never captures."""
    import types

    import rvc_amd.pipeline as rp
    from rvc_amd import realtime as rt

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from e2e_proxies import RmvpeProxy

    monkeypatch.delenv("RVCMI_RMVPE_GRU", raising=False)
    monkeypatch.delenv("RVCMI_RT_GRAPH", raising=False)
    n = rt.f0_extractor_frame(4096, "rmvpe", 160)
    p_len = n // 160
    me = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=RmvpeProxy(gpu, half=True), is_half=True, device=gpu))
    g = torch.Generator().manual_seed(1)
    for i in range(7):
        wav = (0.2 * torch.randn(n, generator=g)).to(gpu)
        pitch, pitchf = rt._rmvpe_f0_graphed(me, wav, p_len, 0)
        pitch, pitchf = pitch.clone(), pitchf.clone()
        entry = next(iter(me._rvcmi_f0_graphs.values()))
        assert ("graph" in entry) == (i >= rt.RT_GRAPH_AFTER - 1), (i, list(entry))
        want = rp._rmvpe_on_device(me, wav, p_len, 0)
        # (two EAGER runs of this network already differ in the last bits -- MIOpen's convolutions are not run-to-run deterministic -- so: to 1e-3)
        assert pitch.shape == (1, p_len) and int((pitch - want[0]).abs().max()) <= 1, "block %d: coarse pitch differs" % i
        assert torch.allclose(pitchf, want[1], rtol=1e-3, atol=0) and float(pitchf.max()) > 0, "block %d: replay differs from the eager chain" % i
    assert len(me._rvcmi_f0_graphs) == 1

    # the replay must follow its INPUT (the proxy's random weights make a nearly input-independent salience): the same mel front end in front of a
    # parameter-free 'network' whose salience peak moves with the signal's level
    class Tiny(torch.nn.Module):
        def forward(self, mel):  # [1, 128, T] log-mel -> [1, T, 360]: a salience bump whose bin follows the frame's level
            c = 180.0 + 25.0 * mel.float().mean(dim=1)
            bins = torch.arange(360, device=mel.device, dtype=torch.float32)
            return torch.exp(-0.5 * ((bins[None, None, :] - c[..., None]) / 3.0) ** 2).to(mel.dtype)

    tiny = RmvpeProxy(gpu, half=False)
    tiny.model = Tiny().to(gpu)
    me3 = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=tiny, is_half=False, device=gpu))
    outs = []
    for i in range(6):
        t = torch.arange(n, device=gpu) / 16000.0
        wav = 0.05 * (i + 1) * torch.sin(2 * torch.pi * 220.0 * t)
        pitch, pitchf = rt._rmvpe_f0_graphed(me3, wav, p_len, 0)
        want = rp._rmvpe_on_device(me3, wav, p_len, 0)
        assert torch.allclose(pitchf, want[1], rtol=1e-4, atol=0) and int((pitch - want[0]).abs().max()) <= 1, "tiny network, block %d" % i
        outs.append(pitchf.clone())
    assert "graph" in next(iter(me3._rvcmi_f0_graphs.values()))
    assert not torch.allclose(outs[-1], outs[-2], rtol=1e-2), "two replays with different inputs gave the same f0: the static input is not read"
    monkeypatch.setenv("RVCMI_RT_GRAPH", "0")
    me2 = types.SimpleNamespace(f0_gen=types.SimpleNamespace(rmvpe=RmvpeProxy(gpu, half=True), is_half=True, device=gpu))
    for i in range(5):
        rt._rmvpe_f0_graphed(me2, wav, p_len, 0)
    assert not getattr(me2, "_rvcmi_f0_graphs", None)


# ---------------------------------------------------------------- against the fp16-operand fp64 oracle, through the C ABI

CANARY = 3  # rows of NaN behind the last row the call may write


def _p(t):
    return C.c_void_p(t.data_ptr())


def _forward(m, x16, gpu):
    """``rvcmi_gru_forward`` on x16 [B, T, I] fp16 -> (y [B * T + CANARY, 512], hn [2, B, 256]), both prefilled with NaN"""
    from rvc_amd import _lib

    B, T = x16.shape[:2]
    y = torch.full((B * T + CANARY, 512), float("nan"), device=gpu)
    hn = torch.full((2, B, 256), float("nan"), device=gpu)
    _lib.check(_lib.lib().rvcmi_gru_forward(m._h, B, T, _p(x16), _p(y), _p(hn), C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
    torch.cuda.synchronize()
    return y, hn


def _within_bars(y, hn, b, what):
    """y [B, T, 512], hn [2, B, 256] from the device against the oracle and bars ``b`` of tests/gru_cases.py; prints the ratios to the floor."""
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(hn).all()), what
    rms, mx = gc.err(y.cpu().numpy(), b["y"])
    print("%s: HIP vs f64 oracle RMS %.3e max %.3e = %.2f x floor_rms, %.2f x floor_max (bars %.3e / %.3e)"
          % (what, rms, mx, rms / b["floor_rms"], mx / b["floor_max"], b["bar_rms"], b["bar_max"]))
    assert rms <= b["bar_rms"] and mx <= b["bar_max"], "%s: RMS %.3e (bar %.3e) max %.3e (bar %.3e)" % (what, rms, b["bar_rms"], mx, b["bar_max"])
    assert gc.err(hn.cpu().numpy(), b["hn"])[1] <= b["bar_max"], what
    # h_n is the last forward / first backward output row, bit for bit
    assert torch.equal(hn[0], y[:, -1, :256]) and torch.equal(hn[1], y[:, 0, 256:]), what


@pytest.mark.parametrize("c", gc.TABLE, ids=gc.case_id)
def test_gru_hip_against_the_fp16_operand_oracle(c, gpu):
    import rvc_amd

    m = rvc_amd.GRUHIP(gc.module(c), device=gpu)
    x16 = gc.inputs(c).half().to(gpu).contiguous()
    rows = c.B * c.T
    y, hn = _forward(m, x16, gpu)
    _within_bars(y[:rows].view(c.B, c.T, 512), hn, gc.bars(c), gc.case_id(c))
    y2, hn2 = _forward(m, x16, gpu)
    assert torch.equal(y2[:rows], y[:rows]) and torch.equal(hn2, hn), "a second call gave other bits"
    assert bool(torch.isnan(y[rows:]).all()) and bool(torch.isnan(y2[rows:]).all()), "written past the last row"


def test_ragged_gru_of_odd_lengths_against_the_oracle(gpu):
    """Lengths that are no multiple of 32 (1, 2, 33, 7, 64, 3 rows packed): every sequence within the bars of its own oracle, bit-equal to its
    own dense call, its ``h_n`` column its own last / first row, nothing written behind the last sequence."""
    import rvc_amd
    from rvc_amd import _lib

    gru, x, off = gc.ragged_case()
    m = rvc_amd.GRUHIP(gru, device=gpu)
    n, R = len(off) - 1, off[-1]
    off_d = torch.tensor(off, dtype=torch.int32, device=gpu)
    xd = x.half().to(gpu).contiguous()
    y = torch.full((R + CANARY, 512), float("nan"), device=gpu)
    hn = torch.full((2, n, 256), float("nan"), device=gpu)
    _lib.check(_lib.lib().rvcmi_gru_forward_ragged(m._h, n, (C.c_int * len(off))(*off), _p(off_d), _p(xd), _p(y), _p(hn),
                                                   C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
    torch.cuda.synchronize()
    for i, b in enumerate(gc.ragged_bars()):
        T = off[i + 1] - off[i]
        yi, hi = _forward(m, xd[off[i]: off[i + 1]][None].contiguous(), gpu)
        assert torch.equal(y[off[i]: off[i + 1]], yi[:T]) and torch.equal(hn[:, i], hi[:, 0]), "sequence %d differs from its dense call" % i
        assert bool(torch.isnan(yi[T:]).all())
        _within_bars(y[None, off[i]: off[i + 1]], hn[:, i: i + 1], {**b, "y": b["y"][None], "hn": b["hn"][:, None]}, "ragged sequence %d, T %d" % (i, T))
    assert bool(torch.isnan(y[R:]).all()), "written behind the last sequence"


def test_a_graph_captured_before_the_workspace_grew_still_replays(gpu):
    """``gru_run`` keeps the projection workspace it outgrows (``retired``): a forward captured at T = 32 must replay unchanged after an eager
    call at T = 96 has replaced the workspace.  One linear chain of two kernels; the replay against an eager call on a second, fresh handle."""
    import rvc_amd

    c = gc.Case(1, 32, 384, 17)
    ref = gc.module(c)
    m = rvc_amd.GRUHIP(ref, device=gpu)
    g = torch.Generator().manual_seed(18)
    static = torch.randn(1, 32, 384, generator=g).half().to(gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side), torch.no_grad():
        m(static)  # warm-up: the workspace is allocated here, outside the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        y_static, hn_static = m(static)
    with torch.no_grad():
        y96, _ = m(torch.randn(1, 96, 384, generator=g).half().to(gpu))  # the workspace grows, outside any capture
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y96).all())
    x_new = torch.randn(1, 32, 384, generator=g).half().to(gpu)
    static.copy_(x_new)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
        y_want, hn_want = rvc_amd.GRUHIP(ref, device=gpu)(x_new)
    torch.cuda.synchronize()
    assert torch.equal(y_static, y_want) and torch.equal(hn_static, hn_want), "the replay after the growth differs from an eager call"
    del graph


def test_forward_refuses_a_cpu_input(gpu):
    import rvc_amd

    m = rvc_amd.GRUHIP(gc.module(gc.Case(1, 4, 384, 17)), device=gpu)
    assert m._device == torch.device("cuda", torch.device(gpu).index if torch.device(gpu).index is not None else torch.cuda.current_device())
    with pytest.raises(rvc_amd.RvcmiError, match="must live on the GPU"):
        m(torch.zeros(1, 4, 384))
    y, hn = m(torch.zeros(1, 4, 384, device=gpu))  # the handle goes on working
    assert tuple(y.shape) == (1, 4, 512) and tuple(hn.shape) == (2, 1, 256) and bool(torch.isfinite(y).all())


def test_forward_refuses_an_input_on_another_gpu(gpu):
    """(A launch on the handle's device with a foreign stream and foreign pointers otherwise.)"""
    import rvc_amd

    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU: no second device to hold the foreign input")
    m = rvc_amd.GRUHIP(gc.module(gc.Case(1, 4, 384, 17)), device=gpu)
    other = (m._device.index + 1) % torch.cuda.device_count()
    with pytest.raises(rvc_amd.RvcmiError, match="the input is on cuda:%d, the weights on %s" % (other, m._device)):
        m(torch.zeros(1, 4, 384, device="cuda:%d" % other))


def test_gru_forward_rejects_more_sequences_than_the_grid_has_rows(gpu):
    """B > 65535 (grid y of one block per (direction, sequence)) is an argument error, found before the workspace is touched; the handle goes on
    working."""
    import rvc_amd
    from rvc_amd import _lib

    c = gc.TABLE[3]
    assert (c.B, c.T, c.I) == (2, 7, 384)
    m = rvc_amd.GRUHIP(gc.module(c), device=gpu)
    B = 65536
    x16 = torch.zeros(B, 1, 384, device=gpu, dtype=torch.float16)  # (full-size buffers: a call that got through would stay in bounds)
    y = torch.empty(B, 512, device=gpu)
    with pytest.raises(rvc_amd.RvcmiError, match="65535") as e:
        _lib.check(_lib.lib().rvcmi_gru_forward(m._h, B, 1, _p(x16), _p(y), None, C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)))
    assert e.value.code == -1  # RVCMI_ERR_INVALID, not a failed launch
    torch.cuda.synchronize()
    yy, hn = _forward(m, gc.inputs(c).half().to(gpu).contiguous(), gpu)
    _within_bars(yy[:c.B * c.T].view(c.B, c.T, 512), hn, gc.bars(c), "after the refusal, " + gc.case_id(c))
