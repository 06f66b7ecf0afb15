"""GPU suite of HuBERT's transformer layers on csrc/hubert_enc.hip: one layer against the fp64 oracle of tests/hubert_enc_cases.py at the bars
derived there, the bit-exact properties (a multi-layer call = the chain of single-layer calls, masked keys, batch independence, determinism,
graph replay), the module swap in both conventions, and the errors."""
import ctypes as C

import numpy as np
import pytest
import torch

import hubert_enc_cases as hc

import rvc_amd
from rvc_amd import _lib
from rvc_amd import hubert as hb

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENC = {}


def encoder(cfg, seed, wgain=1.0, n_layers=1):
    key = (cfg, seed, wgain, n_layers)
    if key not in _ENC:
        ws = hc.weights(cfg, seed, wgain, n_layers)
        _ENC[key] = rvc_amd.HubertEncoderHIP.from_state_dicts([hc.state_dict(w) for w in ws], dict(hc.CONFIGS[cfg], eps=hc.EPS), DEV)
    return _ENC[key]


def dev_inputs(c, x=None):
    x = torch.from_numpy(np.array(hc.inputs(c) if x is None else x)).to(DEV)
    m = hc.key_mask(c)
    return (x.half() if c.half else x), (None if m is None else torch.from_numpy(m).to(DEV))


def check(got, b, name):
    e = hc.err(got, b["y"])
    print("%s: error %.3e %.3e  floor %.3e %.3e  bars %.3e %.3e" % (name, e[0], e[1], b["floor_rms"], b["floor_max"], b["bar_rms"], b["bar_max"]))
    assert e[0] <= b["bar_rms"] and e[1] <= b["bar_max"], name


@pytest.mark.parametrize("c", hc.TABLE, ids=hc.case_id)
def test_one_layer_against_the_oracle(c):
    x, m = dev_inputs(c)
    y = encoder(c.cfg, c.seed, c.wgain)(x, m)
    assert y.dtype == x.dtype and y.shape == x.shape
    check(y.float().cpu().numpy(), hc.bars(c), hc.case_id(c))


def test_workspace_sizes_are_those_of_the_planner_before_the_shared_carve():
    """``rvcmi_hubert_enc_workspace_bytes`` is ABI-visible.  The numbers are the offset planner's arithmetic worked by hand for M = B T rows:
    q / k / v (3 M d fp16), attention (M d fp16), the stream fp32 and fp16, the GELU output (M ffn fp16), two fp32 hand-over buffers, each
    part rounded up to 256 bytes."""
    base = encoder("base", 1)
    assert (base.workspace_bytes(1, 1), base.workspace_bytes(2, 77)) == (23040, 3548160)
    names = {"self_attn.q_proj": (64, 64), "self_attn.k_proj": (64, 64), "self_attn.v_proj": (64, 64), "self_attn.out_proj": (64, 64),
             "self_attn_layer_norm": (64,), "fc1": (64, 64), "fc2": (64, 64), "final_layer_norm": (64,)}
    sd = {}
    for n, shape in names.items():
        sd[n + ".weight"], sd[n + ".bias"] = torch.zeros(shape), torch.zeros(shape[0])
    tiny = rvc_amd.HubertEncoderHIP.from_state_dicts([sd], dict(d=64, heads=1, ffn=64, eps=hc.EPS), DEV)
    assert (tiny.workspace_bytes(1, 1), tiny.workspace_bytes(2, 77)) == (2048, 236544)


@pytest.mark.parametrize("c", hc.STAGE_CASES, ids=hc.case_id)
def test_gelu_output_against_the_oracle(c):
    """FFN-2's operand, read from the caller's workspace: where a wrong GELU would show (tests/hubert_enc_cases.py)."""
    enc = encoder(c.cfg, c.seed, c.wgain)
    x, m = dev_inputs(c)
    ws = torch.zeros(enc.workspace_bytes(c.B, c.T), dtype=torch.uint8, device=DEV)
    y = enc(x, m, workspace=ws)
    assert torch.equal(y, enc(x, m))  # the caller's workspace and the object's own give the same bits
    ffn, off = hc.CONFIGS[c.cfg]["ffn"], hc.ffn1_offset(c)
    h = ws[off:off + c.B * c.T * ffn * 2].view(torch.float16).view(c.B, c.T, ffn)
    check(h.float().cpu().numpy(), hc.bars_ffn1(c), "ffn1 " + hc.case_id(c))


@pytest.mark.parametrize("c", [hc.BATCHES[0], hc.BATCHES[1], hc.BASE[1]], ids=hc.case_id)
def test_two_layers_in_one_call_are_bit_equal_to_two_calls(c):
    enc = encoder(c.cfg, c.seed, c.wgain, 2)
    x, m = dev_inputs(c)
    both = enc(x, m, first=0, n=2)
    assert torch.equal(both, enc(x, m))  # n=None: every layer from ``first``
    one = enc(enc(x, m, first=0, n=1), m, first=1, n=1)
    assert torch.equal(both, one)
    check(both.float().cpu().numpy(), hc.bars(c, 2), "2 layers " + hc.case_id(c))
    assert torch.equal(both, enc(x, m, first=0, n=2))  # and from run to run


@pytest.mark.parametrize("c", [hc.BATCHES[0], hc.BATCHES[1]], ids=hc.case_id)
def test_values_at_masked_keys_do_not_reach_unmasked_rows(c):
    """Through the whole layer (no debug entry, no zeroed weights): everything behind the attention is row-wise, so an unmasked query row of
    the layer's output depends on the masked positions only through their keys and values -- which the mask removes."""
    enc = encoder(c.cfg, c.seed, c.wgain)
    x, m = dev_inputs(c)
    x2 = torch.where(m[:, :, None], torch.full_like(x, 7.5) + x, x)
    y, y2 = enc(x, m), enc(x2, m)
    keep = ~m
    assert torch.equal(y[keep], y2[keep]) and not torch.equal(y[m], y2[m])
    assert not torch.equal(enc(x2, None)[keep], y2[keep])  # (the mask does something)


def test_batch_items_are_independent():
    c = hc.BATCHES[1]
    enc = encoder(c.cfg, c.seed, c.wgain)
    x, m = dev_inputs(c)
    y = enc(x, m)
    for b in range(c.B):
        assert torch.equal(y[b:b + 1], enc(x[b:b + 1].contiguous(), m[b:b + 1].contiguous())), b


def test_graph_capture_after_a_larger_eager_call_replays_bit_equal():
    big, c = hc.SHAPES[9], hc.BATCHES[0]
    enc = encoder("small", c.seed, c.wgain, 2)
    xb, _ = dev_inputs(big)
    enc(xb)  # the larger shape: the object's workspace is allocated here, outside the capture
    x, m = dev_inputs(c)
    want = enc(x, m)
    xs = x.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ys = enc(xs, m)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ys, want)
    xs.copy_(x * 0.5)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(ys, enc(x * 0.5, m))


def _through_the_model(model, layers, run, ws, x_in_hook, mask_np, half):
    """The model on torch, swapped, restored: the swapped result against the oracle chained per layer from the first layer's own input."""
    seen = {}
    def pre(mod, args, kwargs):
        seen.setdefault("x", x_in_hook(args, kwargs))

    hook = layers[0].register_forward_pre_hook(pre, with_kwargs=True)
    with torch.no_grad():
        run()  # (torch's first call picks its convolution / GEMM algorithms and may differ from every later one)
        ref = run()
        repeats = torch.equal(run(), ref)
    hook.remove()
    originals = list(layers)
    assert rvc_amd.accelerate_hubert_layers(model) == len(originals) and all(isinstance(m, rvc_amd.HubertLayerHIP) for m in layers)
    assert len({id(m.encoder) for m in layers}) == 1 and not any(k.startswith("encoder.layers.0._original") for k in model.state_dict())
    with torch.no_grad():
        got = run()
    x0 = seen["x"].float().cpu().numpy()
    y64 = hc.chain(ws, x0, mask_np, half)
    check(got.float().cpu().numpy(), hc.bars_of(hc.chain(ws, x0, mask_np, half, arith="f32"), y64) | {"y": y64}, "model")
    assert rvc_amd.accelerate_hubert_layers(model) == 0  # already swapped
    assert rvc_amd.restore_hubert_layers(model) == len(originals) and all(a is b for a, b in zip(originals, layers))
    with torch.no_grad():
        assert not repeats or torch.equal(run(), ref)  # the same modules again (above); the same bits wherever torch repeats its own
    return got, ref


def test_module_swap_on_transformers_hubert_model():
    from transformers import HubertModel

    ws = hc.weights("small", 70, 1.0, 3)
    model = HubertModel(hc.hf_config("small", 3)).eval()
    for lyr, w in zip(model.encoder.layers, ws):
        lyr.load_state_dict(hc.hf_state_dict(w))
    model = model.to(DEV)
    wav = torch.from_numpy(np.random.default_rng(5).uniform(-0.5, 0.5, (2, 16000)).astype(np.float32)).to(DEV)
    run = lambda: model(wav).last_hidden_state
    assert all(rvc_amd.supported_layer(m) for m in model.encoder.layers)
    got, ref = _through_the_model(model, model.encoder.layers, run, ws, lambda a, k: (a[0] if a else k["hidden_states"]).detach().clone(), None, False)
    assert got.shape == ref.shape == (2, 49, 128)
    # output_attentions: the original layer answers
    assert rvc_amd.accelerate_hubert_layers(model) == 3
    with torch.no_grad():
        out = model(wav, output_attentions=True)
    assert len(out.attentions) == 3 and out.attentions[0].shape == (2, 2, 49, 49) and (out.last_hidden_state - ref).abs().max() < 1e-4
    # an additive mask [B, 1, T, T] becomes the key mask
    lyr = model.encoder.layers[0]
    x = torch.randn(2, 49, 128, device=DEV)
    km = torch.arange(49, device=DEV)[None, :] >= torch.tensor([49, 20], device=DEV)[:, None]
    add = torch.zeros(2, 1, 49, 49, device=DEV).masked_fill(km[:, None, None, :], torch.finfo(torch.float32).min)
    assert torch.equal(lyr(x, attention_mask=add)[0], lyr.encoder(x, km, first=0, n=1))
    assert torch.equal(lyr(x, attention_mask=~km[:, None, None, :].expand(2, 1, 49, 49))[0], lyr.encoder(x, km, first=0, n=1))
    assert rvc_amd.restore_hubert_layers(model) == 3


def test_module_swap_on_a_fairseq_shaped_model(monkeypatch):
    c = hc.Case("small", 3, 70, 71, True, 1.0, "noise", (70, 64, 9))
    ws = hc.weights("small", c.seed, 1.0, 3)
    model = hc.fs_model(ws, "small").half().to(DEV)
    x, m = dev_inputs(c)
    run = lambda: model(x, m)
    # the switch off: the conversion paths' helper leaves encoder.layers untouched
    monkeypatch.delenv("RVCMI_HUBERT_ENC", raising=False)
    before = list(model.encoder.layers)
    assert hb.accelerate_hubert_layers_once(model) == 0 and all(a is b for a, b in zip(before, model.encoder.layers))
    # T x B x C in, T x B x C out
    ws16 = tuple({k: hc.r16(a) for k, a in w.items()} for w in ws)  # what the .half() model holds: biases and LayerNorm affine on the fp16 grid too
    _through_the_model(model, model.encoder.layers, run, ws16, lambda a, k: a[0].detach().transpose(0, 1).clone(), hc.key_mask(c), True)
    # the switch on: once per model object
    monkeypatch.setenv("RVCMI_HUBERT_ENC", "1")
    assert hb.accelerate_hubert_layers_once(model) == 3 and hb.accelerate_hubert_layers_once(model) == 3 and model._rvcmi_hubert_enc == 3
    lyr = model.encoder.layers[1]
    xt = x.transpose(0, 1)
    with torch.no_grad():
        y, (attn, _) = lyr(xt, self_attn_padding_mask=m, need_weights=True)  # -> the original
        y0, (attn0, _) = lyr._original(xt, self_attn_padding_mask=m, need_weights=True)
        assert attn is not None and torch.equal(attn, attn0) and torch.equal(y, y0)
        y, extra = lyr(xt, self_attn_padding_mask=m, need_weights=False)
        assert extra == (None, None) and y.shape == xt.shape and not torch.equal(y, y0)
        sq = torch.zeros(70, 70, device=DEV, dtype=torch.float16)
        assert torch.equal(lyr(xt, self_attn_mask=sq, self_attn_padding_mask=m)[0], lyr._original(xt, self_attn_mask=sq, self_attn_padding_mask=m)[0])
    assert rvc_amd.restore_hubert_layers(model) == 3 and "_rvcmi_hubert_enc" not in model.__dict__


@pytest.mark.parametrize("bad", ["pre_norm", "tanh_gelu", "training"])
def test_swap_is_all_or_none(bad):
    g = hc.CONFIGS["small"]
    model = hc.fs_model(hc.weights("small", 72, 1.0, 3), "small")
    if bad == "pre_norm":
        model.encoder.layers[1].layer_norm_first = True
    elif bad == "tanh_gelu":
        model.encoder.layers[2].activation_fn = lambda v: torch.nn.functional.gelu(v, approximate="tanh")
    model = model.to(DEV)
    if bad == "training":
        model.encoder.layers[0].train()
    before = list(model.encoder.layers)
    assert [rvc_amd.supported_layer(m) for m in before].count(False) == 1
    assert rvc_amd.accelerate_hubert_layers(model) == 0 and all(a is b for a, b in zip(before, model.encoder.layers))
    # transformers' pre-norm layer has the attribute names of the post-norm one: it is told apart by what it computes
    from transformers.models.hubert.modeling_hubert import HubertEncoderLayerStableLayerNorm

    assert not rvc_amd.supported_layer(HubertEncoderLayerStableLayerNorm(hc.hf_config("small", 1)).eval().to(DEV))
    assert rvc_amd.supported_layer(hc.hf_layer(hc.weights("small", 72)[0], "small", torch.float32).to(DEV))
    del g


def test_errors_launch_nothing():
    sd = [hc.state_dict(hc.weights("small", 73)[0])]
    for cfg in (dict(d=128, heads=4, ffn=256), dict(d=128, heads=2, ffn=200), dict(d=128, heads=2, ffn=256, eps=0.0)):
        with pytest.raises(_lib.RvcmiError) as e:
            rvc_amd.HubertEncoderHIP.from_state_dicts(sd, cfg, DEV)
        assert e.value.code == _lib.ERR_INVALID
    extra = dict(sd[0], **{"self_attn.relative_attention_bias.weight": torch.zeros(4, 2)})
    with pytest.raises(_lib.RvcmiError) as e:
        rvc_amd.HubertEncoderHIP.from_state_dicts([extra], dict(hc.CONFIGS["small"]), DEV)
    assert e.value.code == _lib.ERR_INVALID
    enc = encoder("small", 73)
    x = torch.randn(1, 40, 128, device=DEV)
    out = torch.full_like(x, 123.0)
    ws = torch.zeros(enc.workspace_bytes(1, 40), dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    fwd = _lib.lib().rvcmi_hubert_enc_forward
    bad = [(enc._h, 0, 1, 1, 0, P(x), 0, None, P(out), P(ws), st),      # T = 0
           (enc._h, 0, 1, 0, 40, P(x), 0, None, P(out), P(ws), st),     # B = 0
           (enc._h, 0, 1, 1, 40, None, 0, None, P(out), P(ws), st),     # null input
           (enc._h, 0, 1, 1, 40, P(x), 0, None, None, P(ws), st),       # null output
           (enc._h, 0, 1, 1, 40, P(x), 0, None, P(out), None, st),      # null workspace
           (None, 0, 1, 1, 40, P(x), 0, None, P(out), P(ws), st),       # null handle
           (enc._h, 1, 1, 1, 40, P(x), 0, None, P(out), P(ws), st),     # a layer the handle does not have
           (enc._h, 0, 2, 1, 40, P(x), 0, None, P(out), P(ws), st)]
    for args in bad:
        assert fwd(*args) == _lib.ERR_INVALID, args[1:5]
    assert enc.workspace_bytes(1, 0) == 0 and enc.workspace_bytes(0, 5) == 0 and enc.workspace_bytes(65536, 1) == 0
    with pytest.raises(_lib.RvcmiError) as e:
        enc(x, workspace=ws[:ws.numel() - 256])  # a short workspace
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.RvcmiError) as e:
        enc(x[:, :0])
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.RvcmiError):
        enc(x.cpu())
    torch.cuda.synchronize()
    assert bool((out == 123.0).all()) and not ws.any()
