"""HuBERT's convolutional feature extractor on csrc/hubert_fe.hip.

  * the whole extractor against the fp64 oracle of tests/hubert_cases.py (fp16 rounding where the kernel rounds) at the bars derived there:
    one to three frames, the GEMM kernel's M tile one under / at / one over at the last layer and at layer 1, batches whose items differ
    in gain, both input dtypes, weights x 2.5, the zero, the small and the DC + noise (cancellation) inputs;
  * layers 1 - 6 through the debug entry on small-integer data, for which every fp16 product and fp32 sum is exact: BIT-equal to fp64;
  * determinism, a graph captured after a larger eager call, the module swap on transformers' model and on a fairseq-shaped stand-in,
    the models that must be left alone, the switch, and the errors.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import hubert_cases as hc  # noqa: E402

pytestmark = pytest.mark.gpu

_HANDLES = {}


def _hip(gpu, seed, wgain=1.0):
    import rvc_amd

    key = (seed, wgain)
    if key not in _HANDLES:
        _HANDLES[key] = rvc_amd.HubertFrontHIP.from_state_dict(hc.state_dict(hc.weights(seed, wgain), "fairseq"), gpu)
    return _HANDLES[key]


def _x(c, gpu):
    return torch.from_numpy(hc.inputs(c).copy()).to(gpu, torch.float16 if c.half else torch.float32)


@pytest.mark.parametrize("c", hc.TABLE, ids=hc.case_id)
def test_extractor_matches_the_fp64_oracle_at_the_derived_bars(gpu, c):
    b = hc.bars(c)
    x = _x(c, gpu)
    y = _hip(gpu, c.seed, c.wgain)(x)
    assert y.dtype == x.dtype and tuple(y.shape) == (c.B, 512, hc.frames(c.N)) == b["y"].shape
    assert y.transpose(1, 2).is_contiguous()
    got = y.double().cpu().numpy()
    assert np.isfinite(got).all()
    rms, mx = hc.err(got, b["y"])
    print("%s: rms %.3e (bar %.3e, floor %.3e)  max %.3e (bar %.3e, floor %.3e)  max|y| %.3e" % (
        hc.case_id(c), rms, b["bar_rms"], b["floor_rms"], mx, b["bar_max"], b["floor_max"], np.abs(b["y"]).max()))
    assert rms <= b["bar_rms"] and mx <= b["bar_max"]


@pytest.mark.parametrize("c", hc.LAYER0, ids=hc.case_id)
def test_layer_0_matches_the_fp64_oracle_at_its_own_bars(gpu, c):
    """Layer 0 (conv + GroupNorm + GELU) on its own, read from the caller's workspace: the rows a forward of one item leaves there."""
    b = hc.bars0(c)
    hip = _hip(gpu, c.seed, c.wgain)
    ws = torch.zeros(hip.workspace_bytes(1, c.N), device=gpu, dtype=torch.uint8)
    hip(_x(c, gpu), workspace=ws)
    first, L0 = hc.layer0_kept_rows(c.N)
    got = ws[:L0 * 512 * 2].view(torch.float16).view(L0, 512)[first:].double().cpu().numpy()
    assert got.shape == b["y"].shape and np.isfinite(got).all()
    rms, mx = hc.err(got, b["y"])
    print("%s layer 0: rms %.3e (bar %.3e, floor %.3e)  max %.3e (bar %.3e, floor %.3e)" % (hc.case_id(c), rms, b["bar_rms"], b["floor_rms"], mx, b["bar_max"],
                                                                                           b["floor_max"]))
    assert rms <= b["bar_rms"] and mx <= b["bar_max"]


def test_zero_input_gives_gelu_of_beta_after_layer_0(gpu):
    """All-zero input: variance 0, so layer 0 is GELU(beta) in every frame -- read from the caller's workspace, whose first buffer holds layer 0's
    rows (the rows past layer 2's are not overwritten) -- and the output is the same in every frame."""
    c = next(k for k in hc.TABLE if k.kind == "zero")
    hip = _hip(gpu, c.seed)
    ws = torch.zeros(hip.workspace_bytes(c.B, c.N), device=gpu, dtype=torch.uint8)
    y = hip(_x(c, gpu), workspace=ws)
    L0 = (c.N - 10) // 5 + 1
    rows = ws[:L0 * 512 * 2].view(torch.float16).view(L0, 512)
    beta = torch.from_numpy(hc.weights(c.seed)["beta"].copy()).double()
    want = torch.nn.functional.gelu(beta)
    last = rows[-1].double().cpu()
    assert torch.isfinite(last).all()
    ulp = torch.tensor([hc.ulp16(v) for v in want.tolist()], dtype=torch.float64)
    assert bool(((last - want).abs() <= ulp).all())
    assert torch.equal(rows[-1], rows[L0 // 2 + 5])
    assert torch.isfinite(y).all() and bool((y == y[:, :, :1]).all())


@pytest.mark.parametrize("taps,L_in", [(3, 257), (3, 260), (3, 7), (2, 256), (2, 259), (2, 5)])
def test_layers_1_to_6_are_bit_equal_to_fp64_on_small_integers(gpu, taps, L_in):
    """L_in odd and even; 128 and 129 output rows (the M tile and one over), and a handful."""
    from rvc_amd import hubert

    g = torch.Generator().manual_seed(taps * 1000 + L_in)
    B = 2
    x = torch.randint(-3, 4, (B, L_in, 512), generator=g).float()
    w = torch.randint(-2, 3, (512, 512, taps), generator=g).float()
    want = torch.nn.functional.conv1d(x.double().transpose(1, 2), w.double(), stride=2).transpose(1, 2)  # |sums| < 2^24: exact in fp32 too
    got = hubert.debug_conv(x.to(gpu, torch.float16), w)
    assert tuple(got.shape) == tuple(want.shape) == (B, (L_in - taps) // 2 + 1, 512)
    assert torch.equal(got.double().cpu(), want)


def test_two_forwards_are_bit_identical(gpu):
    c = hc.Case(2, 16000, 70)
    hip, x = _hip(gpu, c.seed), _x(c, gpu)
    a = hip(x).clone()
    b = hip(x)
    assert torch.equal(a, b)


def test_graph_captured_after_a_larger_eager_call_replays_bit_equal(gpu):
    import rvc_amd

    big, small = hc.Case(1, 16000, 71), hc.Case(1, 5040, 71)
    hip = _hip(gpu, 71)
    hip(_x(big, gpu))  # the handle's workspace has its size before the capture begins
    xs = _x(small, gpu)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = hip(xs)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    fresh = rvc_amd.HubertFrontHIP.from_state_dict(hc.state_dict(hc.weights(71), "hf"), gpu)
    assert torch.equal(y, fresh(xs))


def test_a_graph_captured_before_the_workspace_grew_still_replays(gpu):
    """The handle keeps the workspace it outgrows (``GrowBuf``): a forward captured at N = 800 on the handle's own workspace must replay unchanged
    after an eager call at N = 4000 has replaced it.  The replay against an eager call on a second, fresh handle."""
    import rvc_amd

    sd = hc.state_dict(hc.weights(72), "fairseq")
    hip = rvc_amd.HubertFrontHIP.from_state_dict(sd, gpu)  # (its own handle: the shared ones already hold larger workspaces)
    g = torch.Generator().manual_seed(73)
    static = torch.randn(1, 800, generator=g).to(gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        hip(static)  # warm-up: the workspace is allocated here, outside the capture
    torch.cuda.current_stream(gpu).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_static = hip(static)
    big = hip(torch.randn(1, 4000, generator=g).to(gpu))  # the workspace grows, outside any capture
    torch.cuda.synchronize()
    assert tuple(big.shape) == (1, 512, hc.frames(4000)) and bool(torch.isfinite(big).all())
    x_new = torch.randn(1, 800, generator=g).to(gpu)
    static.copy_(x_new)
    graph.replay()
    torch.cuda.synchronize()
    y_want = rvc_amd.HubertFrontHIP.from_state_dict(sd, gpu)(x_new)
    torch.cuda.synchronize()
    assert tuple(y_static.shape) == (1, 512, 2) and torch.equal(y_static, y_want), "the replay after the growth differs from an eager call"
    del graph


def test_workspace_sizes_are_those_of_the_planner_before_the_shared_carve(gpu):
    """``rvcmi_hubert_fe_workspace_bytes`` is ABI-visible.  The numbers are the offset planner's arithmetic worked by hand from the layer row
    counts (each part rounded up to 256 bytes: two fp16 activation buffers, the fp64 partial statistics, mean filter, scale, shift)."""
    from rvc_amd import _lib

    hip = _hip(gpu, 70)
    L = _lib.lib()
    assert L.rvcmi_hubert_fe_workspace_bytes(hip._h, 1, 400) == 125952
    assert L.rvcmi_hubert_fe_workspace_bytes(hip._h, 2, 16000) == 9837056
    assert L.rvcmi_hubert_fe_workspace_bytes_ragged(hip._h, 3, 4000) == 3694592


# ---------------------------------------------------------------- the module swap

def _hf_model(gpu, **cfg):
    from transformers import HubertConfig, HubertModel

    torch.manual_seed(3)
    return HubertModel(HubertConfig(**cfg)).eval().to(gpu)


class _Fp32GroupNorm(torch.nn.GroupNorm):
    def forward(self, x):
        return torch.nn.functional.group_norm(x.float(), self.num_groups, self.weight.float(), self.bias.float(), self.eps).type_as(x)


class _FairseqShaped(torch.nn.Module):
    """fairseq's ConvFeatureExtractionModel (extractor_mode "default") as far as its structure and state-dict keys go."""

    def __init__(self):
        super().__init__()
        nn = torch.nn
        self.conv_layers = nn.ModuleList()
        for i, (k, s) in enumerate(zip(hc.KERNELS, hc.STRIDES)):
            mods = [nn.Conv1d(512 if i else 1, 512, k, stride=s, bias=False), nn.Dropout(0.0)]
            if i == 0:
                mods.append(_Fp32GroupNorm(512, 512, affine=True))
            self.conv_layers.append(nn.Sequential(*mods, nn.GELU()))

    def forward(self, x):
        x = x.unsqueeze(1)
        for conv in self.conv_layers:
            x = conv(x)
        return x


def _errs_against_fp32(model32, model16, x):
    with torch.no_grad():
        want = model32(x.float()).last_hidden_state.double().cpu().numpy()
        got = model16(x.half()).last_hidden_state.double().cpu().numpy()
    return hc.err(got, want)


@pytest.mark.parametrize("layout", ["hf", "fairseq"])
def test_swap_and_restore(gpu, layout):
    """The swapped model against torch's fp32 model may be at most TWICE as far as torch's own ``.half()`` model is (what the reference runs)."""
    import copy

    import rvc_amd

    model32 = _hf_model(gpu, num_hidden_layers=2)
    if layout == "fairseq":
        fe = _FairseqShaped().eval().to(gpu)
        w = hc.weights(72)
        fe.load_state_dict(hc.state_dict(w, "fairseq"))
        model32.feature_extractor = fe
    model16 = copy.deepcopy(model32).half()
    x = _x(hc.Case(2, 16000, 73), gpu)
    ref_rms, ref_max = _errs_against_fp32(model32, model16, x)
    torch_fe = model16.feature_extractor
    keys = set(torch_fe.state_dict())
    assert rvc_amd.accelerate_hubert(model16) == 1 and isinstance(model16.feature_extractor, rvc_amd.HubertFrontHIP)
    assert rvc_amd.accelerate_hubert(model16) == 0  # already swapped
    rms, mx = _errs_against_fp32(model32, model16, x)
    print("%s: swapped vs fp32 rms %.3e max %.3e; torch half vs fp32 rms %.3e max %.3e" % (layout, rms, mx, ref_rms, ref_max))
    assert rms <= 2 * ref_rms and mx <= 2 * ref_max
    from rvc_amd import hubert

    # below the measured range the swapped module hands the input to torch's own module, at and above it to the kernels: counted with a hook on
    # torch's module (two calls of a MIOpen half convolution are not bit-equal to each other, so the outputs cannot tell)
    calls = []
    hook = torch_fe.register_forward_hook(lambda mod, args, out: calls.append(int(args[0].shape[1])))
    assert x.shape[1] >= hubert.MIN_SAMPLES
    with torch.no_grad():
        long_out = model16.feature_extractor(x[:, :hubert.MIN_SAMPLES])
        assert calls == [] and tuple(long_out.shape) == (2, 512, hc.frames(hubert.MIN_SAMPLES))
        short_out = model16.feature_extractor(x[:, :hubert.MIN_SAMPLES - 1])
        assert calls == [hubert.MIN_SAMPLES - 1] and tuple(short_out.shape) == (2, 512, hc.frames(hubert.MIN_SAMPLES - 1))
    hook.remove()
    assert rvc_amd.restore_hubert(model16) == 1 and model16.feature_extractor is torch_fe and set(torch_fe.state_dict()) == keys
    assert rvc_amd.restore_hubert(model16) == 0


def test_unsupported_cpu_and_training_models_are_left_alone(gpu):
    import rvc_amd

    small = dict(num_hidden_layers=1)
    for cfg in (dict(feat_extract_norm="layer"), dict(conv_bias=True), dict(conv_kernel=(10, 3, 3, 3, 3, 3, 2)), dict(feat_extract_activation="gelu_new"),
                dict(conv_dim=(256,) * 7)):
        m = _hf_model(gpu, **small, **cfg)
        fe = m.feature_extractor
        assert rvc_amd.accelerate_hubert(m) == 0 and m.feature_extractor is fe, cfg
    m = _hf_model("cpu", **small)
    fe = m.feature_extractor
    assert rvc_amd.accelerate_hubert(m) == 0 and m.feature_extractor is fe
    m = _hf_model(gpu, **small).train()
    fe = m.feature_extractor
    assert rvc_amd.accelerate_hubert(m) == 0 and m.feature_extractor is fe and m.training
    assert rvc_amd.accelerate_hubert(torch.nn.Linear(2, 2)) == 0 and rvc_amd.accelerate_hubert(object()) == 0


def test_switch_swaps_once_per_object_and_the_env_overrides_install(gpu, monkeypatch):
    import rvc_amd
    from rvc_amd import hubert

    class Proxy:  # tools/e2e_proxies.py HubertProxy: the model one attribute down
        def __init__(self):
            self.m = _hf_model(gpu, num_hidden_layers=1).half()

    monkeypatch.delenv("RVCMI_HUBERT_FE", raising=False)
    assert hubert.HUBERT_FE is False and not rvc_amd.hubert_on()  # the default is off
    p = Proxy()
    fe = p.m.feature_extractor
    assert hubert.accelerate_hubert_once(p) == 0 and p.m.feature_extractor is fe and not hasattr(p, "_rvcmi_hubert_fe")
    monkeypatch.setattr(hubert, "HUBERT_FE", True)      # what install(hubert_fe=True) sets
    assert rvc_amd.hubert_on()
    monkeypatch.setenv("RVCMI_HUBERT_FE", "0")           # the environment overrides it
    assert not rvc_amd.hubert_on() and hubert.accelerate_hubert_once(p) == 0 and p.m.feature_extractor is fe
    monkeypatch.setattr(hubert, "HUBERT_FE", False)
    monkeypatch.setenv("RVCMI_HUBERT_FE", "1")
    assert rvc_amd.hubert_on() and hubert.accelerate_hubert_once(p) == 1 and isinstance(p.m.feature_extractor, rvc_amd.HubertFrontHIP)
    hip = p.m.feature_extractor
    assert p._rvcmi_hubert_fe == 1 and hubert.accelerate_hubert_once(p) == 1 and p.m.feature_extractor is hip  # remembered, not redone
    assert rvc_amd.restore_hubert(p) == 1 and p.m.feature_extractor is fe and not hasattr(p, "_rvcmi_hubert_fe")
    import inspect

    assert inspect.signature(rvc_amd.install).parameters["hubert_fe"].default is False


def test_errors(gpu):
    import ctypes as C

    import rvc_amd
    from rvc_amd import _lib

    sd = hc.state_dict(hc.weights(74), "fairseq")
    hip = rvc_amd.HubertFrontHIP.from_state_dict(sd, gpu)
    assert hip(torch.zeros(1, 400, device=gpu)).shape == (1, 512, 1)
    for bad in (torch.zeros(1, 400), torch.zeros(1, 399, device=gpu), torch.zeros(0, 400, device=gpu), torch.zeros(400, device=gpu),
                torch.zeros(1, 400, device=gpu, dtype=torch.float64), torch.zeros(1, 1, device=gpu).expand(70000, 400)):
        with pytest.raises(rvc_amd.RvcmiError):
            hip(bad)
    with pytest.raises(rvc_amd.RvcmiError) as e:
        hip(torch.zeros(1, 399, device=gpu, dtype=torch.float16))
    assert e.value.code == _lib.ERR_INVALID
    lib = _lib.lib()
    assert [lib.rvcmi_hubert_fe_frames(n) for n in (399, 400, 719, 720, 1040, 16000, 192000)] == [0, 1, 1, 2, 3, 49, 599]
    assert lib.rvcmi_hubert_fe_workspace_bytes(hip._h, 1, 399) == 0 and lib.rvcmi_hubert_fe_workspace_bytes(hip._h, 0, 400) == 0
    assert lib.rvcmi_hubert_fe_workspace_bytes(hip._h, 65536, 400) == 0 and lib.rvcmi_hubert_fe_workspace_bytes(hip._h, 1, (1 << 30) + 1) == 0
    x = torch.zeros(1, 400, device=gpu)
    out = torch.zeros(1, 1, 512, device=gpu, dtype=torch.float16)
    for B, N in ((1, 399), (0, 400), (65536, 400), (1, (1 << 30) + 1)):  # refused while the arguments are checked: nothing is launched
        assert lib.rvcmi_hubert_fe_forward(hip._h, B, N, C.c_void_p(x.data_ptr()), 0, C.c_void_p(out.data_ptr()), None, None) == _lib.ERR_INVALID
    missing = {k: v for k, v in sd.items() if k != "conv_layers.3.0.weight"}
    with pytest.raises(rvc_amd.RvcmiError) as e:
        rvc_amd.HubertFrontHIP.from_state_dict(missing, gpu)
    assert e.value.code == -5
    for extra in ({"conv_layers.1.0.bias": torch.zeros(512)}, {"conv_layers.7.0.weight": torch.zeros(512, 512, 2)}, {"conv_layers.1.2.weight": torch.zeros(512)},
                  {"conv_layers.2.0.weight": torch.zeros(512, 512, 2)}):
        with pytest.raises(rvc_amd.RvcmiError) as e:
            rvc_amd.HubertFrontHIP.from_state_dict({**sd, **extra}, gpu)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.HubertFrontHIP.from_state_dict(sd, "cpu")
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.HubertFrontHIP.from_module(_hf_model(gpu, num_hidden_layers=1, feat_extract_norm="layer").feature_extractor)
    with pytest.raises(rvc_amd.RvcmiError):
        hip(x, workspace=torch.zeros(16, device=gpu, dtype=torch.uint8))
    other = rvc_amd.HubertFrontHIP.from_state_dict(sd, gpu)
    other._device = torch.device("cuda", 1)  # the check itself, against a handle that claims another device
    with pytest.raises(rvc_amd.RvcmiError):
        other(x)
