"""Ragged batched HuBERT: ``rvcmi_hubert_fe_forward_ragged`` / ``HubertFrontHIP.forward_ragged``, ``extract_features_batch`` and the grouped path of
``Pipeline.convert_files``.  Every comparison is against the DENSE entry on the lone item or against fp64, none against the ragged entry itself.

  * valid rows bit-equal to the dense entry on the item alone, exact zeros behind them, with a garbage tail (NaN / 6e4) behind every item's
    samples, canaries behind the output and the workspace untouched -- fp16 and fp32 input, caller's and own workspace;
  * a second call, a captured graph, the refusals;
  * the whole model (tests/hubert_batch_cases.py ``FairseqShaped``) batched against its lone calls, both measured against fp64; the naive
    sample mask fails the same bar;
  * ``convert_files`` with the switch on against the switch off.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import hubert_batch_cases as bc  # noqa: E402
import hubert_cases as hc  # noqa: E402
from test_gpu_dropin import rvc_tree  # noqa: E402,F401  (skeleton checkout)

pytestmark = pytest.mark.gpu

SEED = 81
CANARY = 0x5A


@functools.lru_cache(maxsize=None)
def _hip(gpu):
    import rvc_amd

    return rvc_amd.HubertFrontHIP.from_state_dict(hc.state_dict(hc.weights(SEED), "fairseq"), gpu)


def _ids(g):
    return "-".join(map(str, g))


def _padded(lens, half, gpu):
    """-> (x [B, N_max] with a garbage tail behind every item, the items alone)"""
    dt = torch.float16 if half else torch.float32
    items = [torch.from_numpy(w).to(gpu, dt) for w in bc.waves(lens, SEED)]
    x = torch.full((len(lens), max(lens)), 6e4 if half else float("nan"), device=gpu, dtype=dt)
    for i, w in enumerate(items):
        x[i, :lens[i]] = w
    return x, items


@functools.lru_cache(maxsize=None)
def _lone(lens, half, gpu):
    """The dense entry on every item alone, channels last [L_i, 512] (computed once per group and dtype)."""
    _, items = _padded(lens, half, gpu)
    return tuple(_hip(gpu)(w.view(1, -1)).transpose(1, 2)[0].clone() for w in items)


def _raw_ragged(hip, x, lens, out, ws, lens_host=True, lens_dev=True, B=None, N=None):
    """The C entry itself on caller-held buffers -> the return code"""
    from rvc_amd import _lib

    host = (C.c_int * len(lens))(*lens)
    dev = torch.tensor(lens, dtype=torch.int32).to(x.device)
    rc = _lib.lib().rvcmi_hubert_fe_forward_ragged(hip._h, len(lens) if B is None else B, x.shape[1] if N is None else N, host if lens_host else None,
                                                   C.c_void_p(dev.data_ptr()) if lens_dev else None, C.c_void_p(x.data_ptr()), 1 if x.dtype == torch.float16 else 0,
                                                   C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()) if ws is not None else None,
                                                   C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream))
    torch.cuda.synchronize()
    return rc


def _check_rows(rows, lens, lone):
    """rows [B, L_max, 512] against the lone dense calls"""
    for i, n in enumerate(lens):
        L = hc.frames(n)
        assert tuple(lone[i].shape) == (L, 512)
        assert torch.equal(rows[i, :L], lone[i].to(rows.dtype)), "item %d (%d samples): valid rows differ from the dense entry on the item alone" % (i, n)
        assert not bool(rows[i, L:].any()) and bool(torch.isfinite(rows[i, L:]).all()), "item %d: rows behind its end are not exactly zero" % i


@pytest.mark.parametrize("own_ws", [False, True], ids=["caller-ws", "own-ws"])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("lens", bc.GROUPS, ids=_ids)
def test_valid_rows_are_bit_equal_to_the_lone_dense_call_and_the_rest_is_zero(gpu, lens, half, own_ws):
    hip = _hip(gpu)
    x, _ = _padded(lens, half, gpu)
    lone = _lone(lens, half, gpu)
    B, L = len(lens), hc.frames(max(lens))
    if own_ws:
        y = hip.forward_ragged(x, lens)
        assert y.dtype == x.dtype and tuple(y.shape) == (B, 512, L) and y.transpose(1, 2).is_contiguous()
        _check_rows(y.transpose(1, 2), lens, lone)
        return
    need = hip.workspace_bytes_ragged(B, max(lens))
    assert need == hip.workspace_bytes(B, max(lens)) > 0
    ws = torch.full((need + 4096,), CANARY, device=gpu, dtype=torch.uint8)
    out = torch.full((B * L + 4, 512), 123.0, device=gpu, dtype=torch.float16)  # (every valid and every zero row must be WRITTEN)
    assert _raw_ragged(hip, x, lens, out, ws) == 0
    _check_rows(out[:B * L].view(B, L, 512), lens, lone)
    assert bool((out[B * L:] == 123.0).all()) and bool((ws[need:] == CANARY).all())
    y = hip.forward_ragged(x, lens, workspace=ws)
    _check_rows(y.transpose(1, 2), lens, lone)
    assert bool((ws[need:] == CANARY).all())


def test_a_second_call_is_bit_equal(gpu):
    lens = bc.GROUPS[1]
    hip = _hip(gpu)
    x, _ = _padded(lens, False, gpu)
    a = hip.forward_ragged(x, lens).clone()
    assert torch.equal(a, hip.forward_ragged(x, lens))


def test_ragged_context_routes_the_plain_forward_and_clears(gpu):
    import rvc_amd

    lens = bc.GROUPS[0]
    hip = _hip(gpu)
    x, _ = _padded(lens, False, gpu)
    with hip.ragged(lens):
        y = hip(x)
        with pytest.raises(rvc_amd.RvcmiError):
            hip(x[:2])
        with pytest.raises(rvc_amd.RvcmiError):
            hip(x[:, :5000])
    _check_rows(y.transpose(1, 2), lens, _lone(lens, False, gpu))
    with pytest.raises(ZeroDivisionError):
        with hip.ragged(lens):
            1 / 0
    assert hip.__dict__.get("_ragged") is None
    xd = torch.zeros(2, 5040, device=gpu)
    assert torch.equal(hip(xd)[0], hip(xd[:1])[0])  # dense again


def test_a_captured_group_replays_bit_equal_to_a_fresh_handles_eager_call(gpu):
    """The capture is made after a LARGER eager call has replaced the handle's own workspace (and after one eager call at the group, which puts
    its lengths on the device: an upload cannot be captured)."""
    import rvc_amd

    hip = rvc_amd.HubertFrontHIP.from_state_dict(hc.state_dict(hc.weights(SEED), "fairseq"), gpu)
    small, big = bc.GROUPS[0], bc.GROUPS[1]
    xs, _ = _padded(small, False, gpu)
    xb, _ = _padded(big, False, gpu)
    hip.forward_ragged(xs, small)
    hip.forward_ragged(xb, big)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = hip.forward_ragged(xs, small)
    y.zero_()
    graph.replay()
    torch.cuda.synchronize()
    fresh = rvc_amd.HubertFrontHIP.from_state_dict(hc.state_dict(hc.weights(SEED), "hf"), gpu)
    assert torch.equal(y, fresh.forward_ragged(xs, small))
    _check_rows(y.transpose(1, 2), small, _lone(small, False, gpu))


def test_refusals_launch_nothing(gpu):
    import rvc_amd
    from rvc_amd import _lib

    hip = _hip(gpu)
    lens = (5040, 400, 1040)
    x, _ = _padded(lens, False, gpu)
    out = torch.full((3 * 15, 512), 123.0, device=gpu, dtype=torch.float16)
    bad = [dict(lens=(5040, 399, 1040)), dict(lens=(5040, 5041, 1040)), dict(lens=(5039, 400, 1040)), dict(lens=lens, lens_host=False),
           dict(lens=lens, lens_dev=False), dict(lens=lens, B=0), dict(lens=lens, B=65536), dict(lens=lens, N=(1 << 30) + 1), dict(lens=lens, N=399)]
    for kw in bad:
        assert _raw_ragged(hip, x, kw.pop("lens"), out, None, **kw) == _lib.ERR_INVALID, kw
        assert bool((out == 123.0).all())
    lib = _lib.lib()
    assert lib.rvcmi_hubert_fe_workspace_bytes_ragged(hip._h, 0, 5040) == 0 and lib.rvcmi_hubert_fe_workspace_bytes_ragged(hip._h, 1, 399) == 0
    assert lib.rvcmi_hubert_fe_workspace_bytes_ragged(hip._h, 65536, 5040) == 0 and lib.rvcmi_hubert_fe_workspace_bytes_ragged(hip._h, 1, (1 << 30) + 1) == 0
    for args in ((x, (5040, 400)), (x, (5040, 399, 1040)), (x, (5000, 400, 1040)), (x.double(), lens), (x.cpu(), lens), (x[0], lens)):
        with pytest.raises(rvc_amd.RvcmiError):
            hip.forward_ragged(*args)
    with pytest.raises(rvc_amd.RvcmiError):
        hip.forward_ragged(x, lens, workspace=torch.zeros(16, device=gpu, dtype=torch.uint8))


# ---------------------------------------------------------------- the whole model

@pytest.mark.parametrize("lens", bc.MODEL_GROUPS, ids=_ids)
def test_whole_model_batched_is_as_close_to_fp64_as_the_lone_calls(gpu, lens):
    """e_batch <= 2 e_single + 1e-6 rms(ref64) per item (hubert_batch_cases.within_bar).  Measured on an MI355X (profiles/hubert_batch_parity.json):
    both legs at 2 - 5e-7 of rms(ref64) = 1.00; e_batch / e_single is 1.00 on the 128- and 129-frame items, 1.6 - 1.7 on the items of
    (5040, 400, 1040) and 2.9 on the one-frame item next to the long ones (5.2e-7 against a lone call that rounds to 1.8e-7), which the additive
    term passes and the factor 2 alone would not."""
    for e in bc.whole_model_errors(gpu, lens):
        print("%s item %6d (%3d frames): e_batch %.3e  e_single %.3e  (ratio %.2f)  rms(ref64) %.3e" % (
            _ids(lens), e["len"], e["frames"], e["e_batch"], e["e_single"], e["e_batch"] / max(e["e_single"], 1e-300), e["ref_rms"]))
        assert bc.within_bar(e), e


def test_the_naive_sample_mask_fails_the_same_bar(gpu):
    """... on the 400 and the 1040 item, which it leaves one unmasked frame too many: the bar bites."""
    errs = bc.whole_model_errors(gpu, (5040, 400, 1040), naive=True)
    for e in errs:
        print("naive mask, item %5d: e_batch %.3e  e_single %.3e  rms(ref64) %.3e" % (e["len"], e["e_batch"], e["e_single"], e["ref_rms"]))
    assert bc.within_bar(errs[0]) and not bc.within_bar(errs[1]) and not bc.within_bar(errs[2])


# ---------------------------------------------------------------- the pipeline

def _pipe(gpu, tmp_path):
    from test_gpu_prep import _webui_pipe

    d, seed, pl, pipe, net_g, tail = _webui_pipe(gpu, tmp_path)
    for key, val in (("RB_STREAM", 0), ("NO_RB_SPLIT", 1)):
        net_g.dec.set_option(key, val)
    for key, val in (("FR_NJ", 1), ("FR_FFN_SPLIT", 1), ("FR_WN_SPLIT", 1)):
        net_g._rvcmi_front.set_option(key, val)
    return d, seed, pipe, net_g, tail


def test_convert_files_with_the_switch_on_agrees_with_the_switch_off(rvc_tree, gpu, tmp_path, monkeypatch):  # noqa: F811
    """Three inputs of different length through the skeleton ``Pipeline.convert_files`` and the fairseq-shaped model (768 wide, so that the
    index and the synthesizer behind it run as they are): the same segments in the same order, the same ``p_len`` and shapes, and the HuBERT
    features handed to ``blend_segments`` within the whole-model bar -- each leg against the fp64 encoder on the segment's own extractor rows.
    A model without ``forward_padding_mask`` takes the per-segment calls whatever the switch says: bit-equal outputs."""
    import rvc_amd
    import rvc_amd.pipeline as rp
    from oracle import synth
    from rvc_amd import hubert

    d, seed, pipe, net_g, tail = _pipe(gpu, tmp_path)
    monkeypatch.delenv("RVCMI_DEVICE_PREP", raising=False)
    audios = [synth.make_audio16k(n, seed + 1 + i) for i, n in enumerate((16000 * 2 + 77, 20000, 50000))]
    model = bc.make_model(gpu, hidden_size=768, num_attention_heads=12)
    ref = bc.reference_of(model)
    got, waves, batch_calls = [], [], []
    real_blend, real_wave, real_batch = rp.blend_segments, rp._hubert_wave, hubert.extract_features_batch
    monkeypatch.setattr(rp, "blend_segments", lambda raw, *a, **k: (got.append([(f.clone(), p) for f, _, _, p in raw]), real_blend(raw, *a, **k))[1])
    monkeypatch.setattr(rp, "_hubert_wave", lambda self, a0: (lambda w: (waves.append(w.clone()), w)[1])(real_wave(self, a0)))
    monkeypatch.setattr(hubert, "extract_features_batch", lambda m, ws, layer: (batch_calls.append(len(ws)), real_batch(m, ws, layer))[1])

    def convert(hub, batch):
        del got[:], waves[:], batch_calls[:]
        monkeypatch.setenv("RVCMI_HUBERT_FE", "1")
        monkeypatch.setenv("RVCMI_HUBERT_BATCH", "1" if batch else "0")
        torch.manual_seed(5)
        res = pipe.convert_files(hub, net_g, int(d["sid"]), [a.copy() for a in audios], [0, 0, 0], *tail)
        assert len(got) == 1
        return res, list(got[0]), list(waves)

    off, raw_off, waves_off = convert(model, False)
    assert batch_calls == [] and isinstance(model.feature_extractor, rvc_amd.HubertFrontHIP)
    on, raw_on, waves_on = convert(model, True)
    assert batch_calls and sum(batch_calls) >= 2 and all(n >= hubert.HUBERT_BATCH_MIN_ITEMS for n in batch_calls)
    assert len(raw_on) == len(raw_off) == len(waves_off) > len(audios)  # (the 50 000-sample input is cut)
    assert len(on) == len(off) == 3 and all(a.shape == b.shape and np.isfinite(a).all() for a, b in zip(on, off))
    fe = model.feature_extractor
    for i, ((f_on, p_on), (f_off, p_off)) in enumerate(zip(raw_on, raw_off)):
        w = waves_off[i]
        assert torch.equal(w, waves_on[i]) and w.shape[0] >= hubert.MIN_SAMPLES
        assert p_on == p_off and f_on.shape == f_off.shape == (1, hc.frames(w.shape[0]), 768) and f_on.dtype == f_off.dtype
        with torch.no_grad():
            want = ref.encode(fe(w.to(gpu).view(1, -1)).transpose(1, 2).double().cpu(), None, 12).numpy()
        e = {"e_batch": bc.rms(f_on.double().cpu().numpy() - want), "e_single": bc.rms(f_off.double().cpu().numpy() - want), "ref_rms": bc.rms(want)}
        print("segment %d (%d samples): e_batch %.3e  e_single %.3e  rms(ref64) %.3e" % (i, w.shape[0], e["e_batch"], e["e_single"], e["ref_rms"]))
        assert bc.within_bar(e), (i, e)
    rvc_amd.restore_hubert(model)
    # a torch model that ignores padding_mask: swapped like the other, but never batched (its outputs are not compared bit for bit: nothing
    # pins torch's own convolutions to the same bits from one call to the next) ...
    blind = bc.make_model(gpu, with_padding_mask=False, hidden_size=768, num_attention_heads=12)
    b_on, raw_b_on, _ = convert(blind, True)
    assert batch_calls == [] and isinstance(blind.feature_extractor, rvc_amd.HubertFrontHIP) and not hubert.batch_capable(blind)
    assert [(tuple(f.shape), p) for f, p in raw_b_on] == [(tuple(f.shape), p) for f, p in raw_off]
    rvc_amd.restore_hubert(blind)
    # ... and the skeleton's seeded stand-in, which has no forward_padding_mask either: bit-equal with the switch on and off
    fake = synth.FakeHubert(768, seed)
    f_off, raw_f_off, _ = convert(fake, False)
    f_on, raw_f_on, _ = convert(fake, True)
    assert batch_calls == [] and fake.calls == 2 * len(raw_f_off)
    assert len(raw_f_on) == len(raw_f_off) and all(torch.equal(a[0], b[0]) and a[1] == b[1] for a, b in zip(raw_f_on, raw_f_off))
    assert all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(f_on, f_off))
