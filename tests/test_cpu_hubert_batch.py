"""The host side of the batched HuBERT path (hubert.py: ``frame_mask``, ``sample_mask``, ``plan_groups``, ``batch_capable``) and the reason the
extractor needs the lengths: no GPU.

  * ``sample_mask`` pushed through fairseq's rule (restated in tests/hubert_batch_cases.py) is exactly ``frame_mask``; the plain mask is not;
  * ``plan_groups``: a partition, the waste bound per group, deterministic, short items alone, ``max_waste = 0`` groups equal lengths only;
  * models that must stay on the per-item loop are recognised;
  * layer 0 of a zero-padded dense batch is further from the item's own layer 0 than the bars of tests/hubert_cases.py allow: GroupNorm
    statistics taken over N_max cannot pass, whatever is done behind them.
"""
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

MASK_GROUPS = ((400, 1040, 5040), (16000, 31999, 48000), (21000, 400, 10250, 10649), (16000, 16000, 16000), (720, 5050))


@pytest.mark.parametrize("lens", MASK_GROUPS, ids=lambda g: "-".join(map(str, g)))
def test_sample_mask_through_fairseqs_rule_is_the_frame_mask(lens):
    from rvc_amd import hubert

    N = max(lens)
    L = hubert.frames(N)
    fm, sm = hubert.frame_mask(lens, N), hubert.sample_mask(lens, N)
    assert fm.dtype == sm.dtype == torch.bool and tuple(fm.shape) == (len(lens), L) and tuple(sm.shape) == (len(lens), N)
    want = torch.tensor([[t >= hc.frames(n) for t in range(L)] for n in lens])
    assert torch.equal(fm, want)
    assert torch.equal(bc.fairseq_frame_mask(sm, L), fm)
    c = N // L
    for i in range(len(lens)):  # [t c, (t + 1) c) for every padded t and nothing else
        blocks = sm[i, :L * c].view(L, c)
        assert bool((blocks.all(1) | ~blocks.any(1)).all()) and torch.equal(blocks.all(1), fm[i]) and not bool(sm[i, L * c:].any())
    if len(set(lens)) == 1:
        assert not bool(sm.any()) and not bool(fm.any())
    if lens == (720, 5050):
        assert N % L != 0  # the tail fairseq drops
    assert torch.equal(hubert.frame_mask(torch.tensor(lens), N), fm)


def test_the_naive_mask_leaves_a_frame_unmasked():
    """The trap: True from sample N_i on gives, for the 400 and the 1040 item in a batch padded to 5040, one frame more than the item has."""
    from rvc_amd import hubert

    lens = (400, 1040, 5040)
    fm = hubert.frame_mask(lens, 5040)
    naive = bc.fairseq_frame_mask(bc.naive_sample_mask(lens, 5040), 15)
    assert [int((~fm[i]).sum()) for i in range(3)] == [1, 3, 15]
    assert [int((~naive[i]).sum()) for i in range(3)] == [2, 4, 15]
    assert not torch.equal(naive[0], fm[0]) and not torch.equal(naive[1], fm[1]) and torch.equal(naive[2], fm[2])


def _check_plan(lens, groups, w, hubert):
    assert sorted(i for g in groups for i in g) == list(range(len(lens)))
    for g in groups:
        ls = [lens[i] for i in g]
        assert len(g) * max(ls) <= (1 + w) * sum(ls) + 1e-9
        if min(ls) < hubert.MIN_SAMPLES:
            assert len(g) == 1
        if w == 0:
            assert len(set(ls)) == 1


def test_plan_groups():
    from rvc_amd import hubert

    rng = np.random.default_rng(7)
    lens = [int(n) for n in rng.integers(16000, 200000, 40)] + [48000] * 5 + [400, 8000, 15999, 16000]
    for w in (0.0, 0.05, 0.25, 1.0):
        groups = hubert.plan_groups(lens, w)
        _check_plan(lens, groups, w, hubert)
        assert groups == hubert.plan_groups(list(lens), w) == hubert.plan_groups(torch.tensor(lens), w)
    assert any(len(g) > 1 for g in hubert.plan_groups(lens, 0.25))
    assert sorted(hubert.plan_groups(lens, 0.0), key=len)[-1] == [40, 41, 42, 43, 44]  # the five equal lengths, and nothing else with them
    for g in hubert.plan_groups(lens, 1.0):
        assert all(lens[i] >= hubert.MIN_SAMPLES for i in g) or len(g) == 1
    assert hubert.plan_groups([], 0.25) == []
    assert hubert.plan_groups([48000] * 4, 0.0, max_samples=2 * 48000) == [[0, 1], [2, 3]]
    assert hubert.plan_groups(lens) == hubert.plan_groups(lens, hubert.HUBERT_BATCH_MAX_WASTE)
    with pytest.raises(ValueError):
        hubert.plan_groups(lens, -0.1)


def test_switch_and_constants(monkeypatch):
    import inspect

    import rvc_amd
    from rvc_amd import hubert

    monkeypatch.delenv("RVCMI_HUBERT_FE", raising=False)
    monkeypatch.delenv("RVCMI_HUBERT_BATCH", raising=False)
    assert hubert.HUBERT_BATCH is False and hubert.HUBERT_BATCH_MIN_ITEMS == 2 and not rvc_amd.hubert_batch_on()
    assert inspect.signature(rvc_amd.install).parameters["hubert_batch"].default is False
    monkeypatch.setenv("RVCMI_HUBERT_BATCH", "1")
    assert not rvc_amd.hubert_batch_on()  # only together with the extractor's switch
    monkeypatch.setenv("RVCMI_HUBERT_FE", "1")
    assert rvc_amd.hubert_batch_on()
    monkeypatch.setenv("RVCMI_HUBERT_BATCH", "0")
    monkeypatch.setattr(hubert, "HUBERT_BATCH", True)
    assert not rvc_amd.hubert_batch_on()
    monkeypatch.delenv("RVCMI_HUBERT_BATCH")
    assert rvc_amd.hubert_batch_on()


def test_models_that_stay_on_the_per_item_loop_are_recognised():
    import rvc_amd

    m = bc.make_model("cpu")
    assert callable(m.forward_padding_mask) and not rvc_amd.batch_capable(m)  # torch's extractor, and on the CPU

    class Proxy:  # tools/e2e_proxies.py HubertProxy: extract_features that ignores padding_mask, no forward_padding_mask
        def __init__(self):
            self.m = m

        def extract_features(self, source, padding_mask, output_layer):
            return (source,)

    assert not rvc_amd.batch_capable(Proxy()) and not rvc_amd.batch_capable(bc.make_model("cpu", with_padding_mask=False))
    assert not rvc_amd.batch_capable(object()) and not rvc_amd.batch_capable(torch.nn.Linear(2, 2))
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.extract_features_batch(m, [torch.zeros(16000)], 12)


def test_statistics_over_the_padded_length_cannot_pass_layer_0():
    """fp64, the oracle of tests/hubert_cases.py: the ragged extractor IS that oracle per item, zero-padded.  The dense oracle on the padded
    batch takes layer 0's mean and variance over N_max; for the short items that is further from their own layer 0 than ``bars0``'s bars."""
    lens, seed = (5040, 400, 1040), 80
    w = hc.weights(seed)
    xs = [hc.r16(x) for x in bc.waves(lens, seed)]
    pad = np.zeros((len(lens), max(lens)), dtype=np.float32)
    for i, x in enumerate(xs):
        pad[i, :lens[i]] = x
    dense = hc.extractor(w, pad, True, layers=1)
    for i, n in enumerate(lens):
        own64 = hc.extractor(w, xs[i][None], True, layers=1)[0]
        own32 = hc.extractor(w, xs[i][None], True, arith="f32", layers=1)[0]
        b = hc.bars_of(own32, own64, layer0=True)
        r, mx = hc.err(dense[i, :own64.shape[0]], own64)
        print("item %d (%d samples): dense-batch layer 0 vs its own: rms %.3e (bar %.3e)  max %.3e (bar %.3e)" % (i, n, r, b["bar_rms"], mx, b["bar_max"]))
        if n == max(lens):
            assert r <= b["bar_rms"] and mx <= b["bar_max"]  # the full-length item has no padding: the same function
        else:
            assert r > b["bar_rms"] and mx > b["bar_max"]
