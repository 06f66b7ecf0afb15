"""CPU suite of the HuBERT encoder-layer kernels' yardstick (tests/hubert_enc_cases.py): the fp64 oracle is transformers' own layer when its
rounding is off, the kernels' documented liberties stay within half of each bar, the named wrong layers stand clear of the bars, and the
binding, the switch and the structural recognition behave without a GPU."""
import numpy as np
import pytest
import torch

import hubert_enc_cases as hc

import rvc_amd
from rvc_amd import _lib
from rvc_amd import hubert as hb


@pytest.mark.parametrize("c", [hc.SHAPES[9], hc.BATCHES[1], hc.BATCHES[2]], ids=hc.case_id)
def test_oracle_without_rounding_is_transformers_layer_in_fp64(c):
    w, x, m = hc.weights(c.cfg, c.seed)[0], hc.inputs(c).copy(), hc.key_mask(c)
    got = hc.layer(w, x, m, half=False, round_operands=False)
    add = None
    if m is not None:
        add = torch.zeros(c.B, 1, c.T, c.T, dtype=torch.float64).masked_fill(torch.from_numpy(m)[:, None, None, :], torch.finfo(torch.float64).min)
    with torch.no_grad():
        want = hc.hf_layer(w, c.cfg)(torch.from_numpy(x).double(), attention_mask=add)[0].numpy()
    assert np.abs(got - want).max() < 1e-11
    # ... and the fairseq-shaped stand-in is the same function in the other convention
    fs = hc.fs_model((w,), c.cfg).double()
    with torch.no_grad():
        want = fs(torch.from_numpy(x).double(), None if m is None else torch.from_numpy(m)).numpy()
    assert np.abs(got - want).max() < 1e-11


def test_perturbations_stay_inside_half_the_bars():
    rows, worst = [], [0.0, 0.0]
    for c in hc.TABLE + tuple(("ffn1", c) for c in hc.STAGE_CASES):
        stage, c = c if isinstance(c, tuple) and c[0] == "ffn1" else (None, c)
        b = hc.bars_ffn1(c) if stage else hc.bars(c)
        w, x, m = hc.weights(c.cfg, c.seed, c.wgain)[0], hc.inputs(c), hc.key_mask(c)
        for seed in (1, 2):
            e = hc.err(hc.layer(w, x, m, c.half, arith="f32", perturb=dict(hc.PERTURB, seed=seed), stage=stage), b["y"])
            r = [e[0] / b["floor_rms"] if b["floor_rms"] else float("nan"), e[1] / b["floor_max"] if b["floor_max"] else float("nan")]
            print("%-5s %-44s seed %d  floor %.3e %.3e  perturbed %.3e %.3e  ratio %.2f %.2f  bars %.3e %.3e" % (
                stage or "", hc.case_id(c), seed, b["floor_rms"], b["floor_max"], e[0], e[1], r[0], r[1], b["bar_rms"], b["bar_max"]))
            worst = [max(worst[i], r[i]) if r[i] == r[i] else worst[i] for i in range(2)]
            rows.append((hc.case_id(c), e, b))
    print("worst ratio of perturbed error to floor: rms %.2f, max %.2f" % tuple(worst))
    for name, e, b in rows:
        assert e[0] <= 0.5 * b["bar_rms"] and e[1] <= 0.5 * b["bar_max"], name
    # the factor is twice the worst ratio, rounded up to the next half
    assert hc.FACTOR == np.ceil(2.0 * max(worst) * 2.0) / 2.0


WRONG = (("scale_before_bias", hc.BASE[0]), ("scale_before_bias", hc.SHAPES[10]), ("tanh_gelu", hc.STAGE_CASES[0]), ("pre_norm", hc.SHAPES[10]),
         ("mask_ignored", hc.BATCHES[0]), ("mask_ignored", hc.BATCHES[1]), ("mask_ignored", hc.BATCHES[2]), ("no_max", hc.LARGE_SCORES),
         ("unbiased_var", hc.SHAPES[10]))
CLEAR = 1.25


@pytest.mark.parametrize("variant,c", WRONG, ids=lambda v: v if isinstance(v, str) else hc.case_id(v))
def test_wrong_layers_stand_clear_of_the_bars(variant, c):
    stage = "ffn1" if variant == "tanh_gelu" else None  # (a wrong GELU is held to account at the GELU output: hubert_enc_cases' docstring)
    b = hc.bars_ffn1(c) if stage else hc.bars(c)
    y = hc.layer(hc.weights(c.cfg, c.seed, c.wgain)[0], hc.inputs(c), hc.key_mask(c), c.half, variant=variant, stage=stage)
    e = hc.err(y, b["y"])
    print("%s on %s: error %.3e %.3e against bars %.3e %.3e" % (variant, hc.case_id(c), e[0], e[1], b["bar_rms"], b["bar_max"]))
    assert e[0] > CLEAR * b["bar_rms"] or e[1] > CLEAR * b["bar_max"]


def test_large_score_case_overflows_an_unstable_softmax():
    c = hc.LARGE_SCORES
    w, x = hc.weights(c.cfg, c.seed, c.wgain)[0], hc.inputs(c)
    assert np.isfinite(hc.layer(w, x, None, c.half, arith="f32")).all()
    assert not np.isfinite(hc.layer(w, x, None, c.half, arith="f32", variant="no_max")).all()  # exp(score) leaves fp16's range


def test_binding_switch_and_recognition_without_a_gpu(monkeypatch):
    names = {s[0] for s in _lib.SYMBOLS}
    assert {"rvcmi_hubert_enc_create", "rvcmi_hubert_enc_destroy", "rvcmi_hubert_enc_workspace_bytes", "rvcmi_hubert_enc_forward"} <= names
    assert "hubert_enc.hip" in _lib.SOURCES
    for n in ("HubertEncoderHIP", "HubertLayerHIP", "accelerate_hubert_layers", "restore_hubert_layers", "supported_layer"):
        assert hasattr(rvc_amd, n) and n in rvc_amd.__all__
    monkeypatch.delenv("RVCMI_HUBERT_ENC", raising=False)
    assert hb.HUBERT_ENC is False and not hb.hubert_enc_on()
    monkeypatch.setenv("RVCMI_HUBERT_ENC", "1")
    assert hb.hubert_enc_on() and not hb.hubert_on()  # independent of RVCMI_HUBERT_FE
    monkeypatch.setenv("RVCMI_HUBERT_ENC", "0")
    monkeypatch.setattr(hb, "HUBERT_ENC", True)
    assert not hb.hubert_enc_on()
    # a CPU model: nothing is swapped, nothing raises; with the switch off the once-helper does not even look
    m = hc.fs_model(hc.weights("small", 1, 1.0, 2), "small")
    before = list(m.encoder.layers)
    assert not hb.supported_layer(before[0]) and hb.accelerate_hubert_layers(m) == 0 and hb.accelerate_hubert_layers_once(m) == 0
    assert all(a is b for a, b in zip(before, m.encoder.layers)) and "_rvcmi_hubert_enc" not in m.__dict__
    assert sorted(hb.layer_state_dict(before[0])) == sorted(hb._LAYER_TENSORS)
    hf = hc.hf_layer(hc.weights("small", 1)[0], "small", torch.float32)
    sd = hb.layer_state_dict(hf)
    assert sorted(sd) == sorted(hb._LAYER_TENSORS) and torch.equal(sd["fc1.weight"], hf.feed_forward.intermediate_dense.weight)
    with pytest.raises(_lib.RvcmiError):
        hb.HubertEncoderHIP.from_state_dicts([hc.state_dict(hc.weights("small", 1)[0])], dict(hc.CONFIGS["small"], eps=hc.EPS), "cpu")
    h = _lib.C.c_void_p()
    assert _lib.lib().rvcmi_hubert_enc_create(None, 0, 1, 128, 2, 256, 1e-5, 0, _lib.C.byref(h)) == _lib.ERR_INVALID
    assert _lib.lib().rvcmi_hubert_enc_workspace_bytes(None, 1, 1) == 0
    assert _lib.lib().rvcmi_hubert_enc_forward(None, 0, 1, 1, 1, None, 1, None, None, None, None) == _lib.ERR_INVALID
