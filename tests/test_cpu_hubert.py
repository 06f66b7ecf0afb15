"""The checker of csrc/hubert_fe.hip checked (no GPU): the fp64 oracle of tests/hubert_cases.py is transformers' ``HubertFeatureEncoder``,
and the bars derived from it are sharp enough to tell the kernel's documented design from the networks that look like it.

  * With the fp16 rounding off, the oracle is ``HubertFeatureEncoder`` in fp64 (1e-12 relative to the largest output) and reproduces the
    committed goldens (tests/golden/hubert_fe_*.npz, written by tools/make_golden_hubert.py from that module).
  * The kernel's documented liberties -- erff within 4 ulp, the normalisation scale within 1 ulp, another summation order -- move the fp32
    evaluation by at most HALF the bars' factors over the floor: the factors are twice the largest movement.
  * The reference's own fp32 path (the module in float32) is inside the bars on every case.
  * The named wrong variants stand clear of the bars, each on the case and at the place that exposes it: tanh-GELU (measured 7.7x the RMS bar),
    the unbiased variance (70x) and statistics taken from the fp16-rounded conv output (3x) at layer 0, where six more layers of fp16
    rounding have not buried them yet; eps dropped, statistics shared across the batch and reversed taps (> 400x) in the final output.
    Whoever widens the bars fails here.
  * The structural recognition of ``rvc_amd.hubert.supported`` and the key renaming, which need no GPU.
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

EXACT = (hc.Case(1, 400, 80, False), hc.Case(2, 1040, 81, False), hc.Case(1, 5040, 82, False, 2.5), hc.Case(2, 5040, 83, False, 1.0, "dc"),
         hc.Case(1, 5040, 84, False, 1.0, "small"))


def _hf(c, dtype):
    fe = hc.hf_module(hc.weights(c.seed, c.wgain), dtype)
    with torch.no_grad():
        return fe(torch.from_numpy(hc.inputs(c).copy()).to(dtype)).double().numpy()


@pytest.mark.parametrize("c", EXACT, ids=hc.case_id)
def test_the_oracle_is_transformers_feature_encoder(c):
    ref = _hf(c, torch.float64)
    y = hc.extractor(hc.weights(c.seed, c.wgain), hc.inputs(c), c.half, round_operands=False)
    assert y.shape == ref.shape == (c.B, 512, hc.frames(c.N))
    mx = hc.err(y, ref)[1]
    print("%s: oracle (no rounding) vs HubertFeatureEncoder fp64: %.2e max-abs, max|y| %.2e" % (hc.case_id(c), mx, np.abs(ref).max()))
    assert mx <= 1e-12 * max(np.abs(ref).max(), 1e-3)


@pytest.mark.parametrize("name", sorted(hc.GOLDEN))
def test_the_oracle_reproduces_the_goldens(name):
    c = hc.GOLDEN[name]
    d = np.load(os.path.join(hc.GOLDEN_DIR, name + ".npz"), allow_pickle=False)
    assert np.array_equal(d["x"], hc.inputs(c))  # the seeded input is the committed one
    y = hc.extractor(hc.weights(c.seed, c.wgain), d["x"], False, round_operands=False)
    assert y.shape == d["y"].shape and hc.err(y, d["y"])[1] <= 1e-12 * np.abs(d["y"]).max()


def test_frame_counts():
    assert [hc.frames(n) for n in (399, 400, 719, 720, 1040, 16000, 192000)] == [0, 1, 1, 2, 3, 49, 599]
    for c in hc.TABLE:
        assert hc.bars(c)["y"].shape == (c.B, 512, hc.frames(c.N))
    rows = [192000]
    for k, s in zip(hc.KERNELS, hc.STRIDES):
        rows.append((rows[-1] - k) // s + 1)
    assert rows[1:] == [38399, 19199, 9599, 4799, 2399, 1199, 599]
    assert {hc.frames(c.N) for c in hc.TILE_EDGES[:3]} == {hc.M_TILE - 1, hc.M_TILE, hc.M_TILE + 1}
    assert {((c.N - 10) // 5 + 1 - 3) // 2 + 1 for c in hc.TILE_EDGES[3:]} == {hc.M_TILE - 1, hc.M_TILE, hc.M_TILE + 1}


@pytest.mark.parametrize("c", hc.TABLE, ids=hc.case_id)
def test_perturbations_stay_inside_half_the_bars(c):
    """erff +-4 ulp, the normalisation scale +-1 ulp, the K loop in another order: the fp32 evaluation so perturbed is within half of each bar
    (bar_rms = 2.5 floor + 1.2 ulp16(rms y), bar_max = 2.5 floor + ulp16(max |y|)) of the fp64 oracle."""
    b = hc.bars(c)
    assert b["bar_rms"] == 2.5 * b["floor_rms"] + 1.2 * hc.ulp16(np.sqrt(np.mean(b["y"] ** 2))) and b["bar_max"] == 2.5 * b["floor_max"] + hc.ulp16(np.abs(b["y"]).max())
    w, x = hc.weights(c.seed, c.wgain), hc.inputs(c)
    for seed in (1, 2):
        y = hc.extractor(w, x, c.half, arith="f32", perturb={"erf": 4, "rsqrt": 1, "reorder": True, "seed": seed})
        rms, mx = hc.err(y, b["y"])
        print("%s seed %d: %.3e rms = %.2f x floor, %.3e max = %.2f x floor" % (hc.case_id(c), seed, rms, rms / max(b["floor_rms"], 1e-300), mx,
                                                                              mx / max(b["floor_max"], 1e-300)))
        assert rms <= b["bar_rms"] / 2 and mx <= b["bar_max"] / 2
        if c in hc.LAYER0:
            b0 = hc.bars0(c)
            y0 = hc.extractor(w, x, c.half, arith="f32", perturb={"erf": 4, "rsqrt": 1, "reorder": True, "seed": seed}, layers=1)[0, hc.layer0_kept_rows(c.N)[0]:]
            rms, mx = hc.err(y0, b0["y"])
            print("    layer 0: %.3e rms = %.2f x floor, %.3e max = %.2f x floor" % (rms, rms / max(b0["floor_rms"], 1e-300), mx, mx / max(b0["floor_max"], 1e-300)))
            assert rms <= b0["bar_rms"] / 2 and mx <= b0["bar_max"] / 2


@pytest.mark.parametrize("c", hc.TABLE, ids=hc.case_id)
def test_the_references_fp32_path_is_inside_the_bars(c):
    """transformers' module in float32 on the CPU, fed what the kernel is fed (fp16-rounded weights and input; it does not round between
    layers, so it is compared with the oracle that does not either, at the bars of the one that does)."""
    w = hc.weights(c.seed, c.wgain)
    w16 = {"conv": tuple(hc.r16(a) for a in w["conv"]), "gamma": w["gamma"], "beta": w["beta"]}
    fe = hc.hf_module(w16, torch.float32)
    with torch.no_grad():
        y = fe(torch.from_numpy(hc.inputs(c).copy())).double().numpy()
    want = hc.extractor(w16, hc.inputs(c), c.half, round_operands=False)
    b = hc.bars(c)
    rms, mx = hc.err(y, want)
    print("%s: torch fp32 vs fp64 oracle (no stream rounding) rms %.3e (bar %.3e) max %.3e (bar %.3e)" % (hc.case_id(c), rms, b["bar_rms"], mx, b["bar_max"]))
    assert np.isfinite(y).all() and rms <= b["bar_rms"] and mx <= b["bar_max"]


# variant -> (the case that exposes it, where: the final output or layer 0 alone, the least multiple of the RMS bar it must reach)
WRONG = {
    "tanh_gelu": (hc.Case(1, 16000, 14), "layer0", 5),
    "unbiased_var": (hc.Case(1, 1040, 13), "layer0", 10),
    "stats_from_fp16": (hc.Case(1, 5040, 56, True, 1.0, "dc"), "layer0", 2),
    "no_eps": (hc.Case(1, 5040, 54, True, 1.0, "small"), "out", 10),
    "stats_across_batch": (hc.Case(3, 5040, 41), "out", 10),
    "taps_reversed": (hc.Case(1, 1040, 13), "out", 10),
}


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_the_bars_separate_the_design_from_its_lookalikes(variant):
    c, where, factor = WRONG[variant]
    assert c in hc.TABLE and (where == "out" or c in hc.LAYER0)  # a case the GPU test runs, at the place it looks
    if where == "out":
        b = hc.bars(c)
        y = hc.extractor(hc.weights(c.seed, c.wgain), hc.inputs(c), c.half, variant=variant)
    else:
        b = hc.bars0(c)
        y = hc.extractor(hc.weights(c.seed, c.wgain), hc.inputs(c), c.half, variant=variant, layers=1)[0, hc.layer0_kept_rows(c.N)[0]:]
    rms = hc.err(y, b["y"])[0]
    print("%s on %s: %.2e RMS = %.1f x bar_rms (floor %.2e)" % (variant, hc.case_id(c), rms, rms / b["bar_rms"], b["floor_rms"]))
    assert rms >= factor * b["bar_rms"], "%s is only %.2f x the RMS bar of %s" % (variant, rms / b["bar_rms"], hc.case_id(c))


def test_a_frame_too_many_or_too_few_changes_the_shape():
    c = hc.Case(1, 1040, 13)
    for variant, L in (("frame_more", 4), ("frame_less", 2)):
        y = hc.extractor(hc.weights(c.seed), hc.inputs(c), c.half, variant=variant)
        assert y.shape == (1, 512, L) != hc.bars(c)["y"].shape


def test_the_zero_and_dc_cases_are_what_they_claim():
    z = next(c for c in hc.TABLE if c.kind == "zero")
    assert not hc.inputs(z).any() and np.isfinite(hc.bars(z)["y"]).all()
    dc = next(c for c in hc.TABLE if c.kind == "dc" and not c.half)
    x = hc.inputs(dc)[0].astype(np.float64)
    assert abs(x.mean() - 0.5) < 1e-3 and x.std() < 1e-3  # mean^2 / variance > 2.5e5: E[y^2] - mean^2 in fp32 would keep no digit of the variance


# ---------------------------------------------------------------- recognition (rvc_amd.hubert), no GPU

def test_recognition_is_by_structure():
    from transformers import HubertConfig
    from transformers.models.hubert.modeling_hubert import HubertFeatureEncoder

    from rvc_amd import hubert

    assert hubert.supported(HubertFeatureEncoder(HubertConfig()).eval())
    for cfg in (dict(feat_extract_norm="layer"), dict(conv_bias=True), dict(conv_kernel=(10, 3, 3, 3, 3, 3, 2)), dict(conv_stride=(5, 2, 2, 2, 2, 2, 1)),
                dict(feat_extract_activation="gelu_new"), dict(feat_extract_activation="relu"), dict(conv_dim=(256,) * 7)):
        assert not hubert.supported(HubertFeatureEncoder(HubertConfig(**cfg)).eval()), cfg
    fe = HubertFeatureEncoder(HubertConfig()).eval()
    fe.conv_layers[0].layer_norm.eps = 1e-6
    assert not hubert.supported(fe)
    assert not hubert.supported(torch.nn.Linear(2, 2)) and not hubert.supported(None)
    nn = torch.nn
    fs = nn.Module()  # fairseq's shape: Sequential(conv, dropout, [norm], GELU) per layer
    fs.conv_layers = nn.ModuleList(nn.Sequential(*([nn.Conv1d(512 if i else 1, 512, k, stride=s, bias=False), nn.Dropout(0.1)]
                                                   + ([nn.GroupNorm(512, 512)] if i == 0 else []) + [nn.GELU()]))
                                   for i, (k, s) in enumerate(zip(hc.KERNELS, hc.STRIDES)))
    assert hubert.supported(fs)
    fs.conv_layers[3][-1] = nn.GELU(approximate="tanh")
    assert not hubert.supported(fs)


def test_both_key_layouts_are_renamed_to_one():
    from rvc_amd import hubert

    w = hc.weights(5)
    a = hubert.canonical_keys({"feature_extractor." + k: v for k, v in hc.state_dict(w, "hf").items()})
    b = hubert.canonical_keys(hc.state_dict(w, "fairseq"))
    assert sorted(a) == sorted(b) == sorted(["conv_layers.%d.0.weight" % i for i in range(7)] + ["conv_layers.0.2.weight", "conv_layers.0.2.bias"])
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert hubert.frames(399) == 0 and hubert.frames(400) == 1 and hubert.frames(16000) == 49
    assert hubert.HUBERT_FE is False  # the default is off
