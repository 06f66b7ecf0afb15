"""CPU side of the RMVPE U-Net work (csrc/unet.hip, rvc_amd/unet.py): the tests' own functional evaluator against the REAL reference's
output, the conditions that make the seeded weights a meaningful parity case, the recogniser, the ABI symbols, the default-off switch; the
fp16-operand fp64 oracle (oracle/unet_oracle.py): its identities, the floors and caps of tests/unet_cases.py with both sides asserted, the
named wrong variants, the workspace offsets of the skip tensors."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import unet_cases as uc  # noqa: E402


def _golden(name):
    return np.load(os.path.join(uc.GOLDEN, name))


def test_key_list_is_the_reference_networks():
    keys = uc.golden_keys()
    assert len(keys) == 731 and keys == uc.key_list(**uc.FULL)
    import rvc_amd.unet as ru

    assert list(ru.expected_keys(**uc.FULL).items()) == keys
    assert ru.geometry(dict(keys)) == dict(uc.FULL, head=3)


def test_functional_evaluator_reproduces_the_real_reference():
    """fp32 on the CPU, to fp32 rounding: allclose at rtol 1e-4 relative to the output's RMS."""
    for name, keys in (("rmvpe_unet_T32.npz", uc.golden_keys()), ("rmvpe_unet_small_T24.npz", None)):
        z = _golden(name)
        if keys is None:
            keys = uc.key_list(int(z["levels"]), int(z["blocks"]), int(z["inters"]), int(z["base"]))
        sd = uc.seeded_weights(keys, int(z["seed"]))
        mel = torch.from_numpy(z["mel"])
        assert torch.equal(mel, uc.seeded_mel(1, mel.shape[-1], int(z["mel_seed"])))
        with torch.no_grad():
            out = uc.forward(sd, mel)
        ref = torch.from_numpy(z["out"])
        rms = float(ref.pow(2).mean().sqrt())
        assert out.shape == ref.shape == (1, mel.shape[-1], 384) and rms > 0.5
        assert float((out - ref).abs().max()) <= 1e-4 * rms, name


def test_seeded_weights_keep_every_branch_visible_and_inside_fp16():
    """Neither is a tolerance: with torch's default BatchNorm gains the branches vanish against the shortcut path (a wrong convolution would
    pass a parity test), with large gains the 56 residual units overflow fp16."""
    z = _golden("rmvpe_unet_T32.npz")
    sd = uc.seeded_weights(uc.golden_keys(), int(z["seed"]))
    stats = []
    with torch.no_grad():
        uc.forward(sd, torch.from_numpy(z["mel"]), stats=stats)
    assert len(stats) == 56
    for s in stats:
        assert s["branch_rms"] >= 0.1 * s["shortcut_rms"], s
        assert s["max_abs"] < 1000, s


def test_standin_is_recognised_and_the_rest_is_refused():
    import rvc_amd
    import rvc_amd.unet as ru

    keys = uc.golden_keys()
    model = uc.StandIn(keys)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    assert ru.geometry(shapes) == dict(uc.FULL, head=3) and ru._pooling_ok(model.unet)
    assert rvc_amd.accelerate_rmvpe_unet(model) == 0 and isinstance(model.unet, uc._UNet)  # a CPU model is left alone
    # one shape altered
    for victim in ("unet.encoder.layers.2.conv.1.conv.3.weight", "unet.decoder.layers.0.conv1.0.weight", "cnn.bias", "unet.encoder.bn.running_var"):
        bad = dict(shapes)
        bad[victim] = bad[victim][:-1] + (bad[victim][-1] + 1,)
        assert ru.geometry(bad) is None, victim
    # a key missing, a key too many
    assert ru.geometry({k: s for k, s in shapes.items() if k != "unet.intermediate.layers.3.conv.3.conv.4.bias"}) is None
    assert ru.geometry(dict(shapes, **{"unet.extra.weight": (3,)})) is None
    assert ru.geometry({"fc.0.gru.weight_ih_l0": (768, 384)}) is None
    # a channel count that is not a multiple of 16
    assert ru.geometry(dict(uc.key_list(2, 1, 1, 24))) is None and ru.geometry(dict(uc.key_list(2, 1, 1, 32))) is not None
    # pooling other than (2, 2): not in the state dict, read from the modules
    assert not ru._pooling_ok(uc.StandIn(uc.key_list(2, 1, 1, 16), pool=(1, 2)).unet)
    assert not ru._pooling_ok(torch.nn.Sequential(torch.nn.ConvTranspose2d(4, 4, 3, stride=(1, 2), padding=1, output_padding=(0, 1))))
    assert ru._pooling_ok(torch.nn.Sequential(torch.nn.ConvTranspose2d(4, 4, 3, stride=2, padding=1, output_padding=1), torch.nn.AvgPool2d(2)))
    # a tree of REAL torch modules, as the reference's network is one: every nn.Conv2d has an `output_padding` too, only the transposed
    # ones are held to stride (2, 2)
    real = uc.StandIn(keys, real_modules=True)
    kinds = [type(m) for m in real.unet.modules()]
    assert kinds.count(torch.nn.Conv2d) == 123 and kinds.count(torch.nn.ConvTranspose2d) == 5 and kinds.count(torch.nn.AvgPool2d) == 1
    assert [(k, tuple(v.shape)) for k, v in real.state_dict().items()] == keys
    assert ru.geometry({k: tuple(v.shape) for k, v in real.state_dict().items()}) == dict(uc.FULL, head=3) and ru._pooling_ok(real.unet)
    assert not ru._pooling_ok(uc.StandIn(uc.key_list(2, 1, 1, 16), pool=(1, 2), real_modules=True).unet)
    assert ru._pooling_ok(torch.nn.Sequential(torch.nn.Conv2d(4, 4, 3, padding=1), torch.nn.ConvTranspose2d(4, 4, 3, stride=2, padding=1, output_padding=1)))
    # a CPU device is no place for the HIP module
    try:
        rvc_amd.UNetHIP.from_state_dict(uc.seeded_weights(uc.key_list(2, 1, 1, 16), 0), "cpu")
    except rvc_amd.RvcmiError:
        pass
    else:
        raise AssertionError("UNetHIP on the CPU did not raise")


def test_abi_symbols_bind_and_the_version_stays():
    from rvc_amd import _lib

    names = [s[0] for s in _lib.SYMBOLS]
    for n in ("rvcmi_unet_create", "rvcmi_unet_workspace_bytes", "rvcmi_unet_forward", "rvcmi_unet_destroy"):
        assert n in names and getattr(_lib.lib(), n) is not None
    assert _lib.lib().rvcmi_version() == _lib.RVCMI_VERSION == 2
    assert "unet.hip" in _lib.SOURCES
    header = open(os.path.join(os.path.dirname(HERE), "include", "rvcmi.h")).read()
    for n in names:
        assert n + "(" in header, n


def test_switch_is_off_by_default_and_the_helper_swaps_what_it_swapped(monkeypatch):
    import rvc_amd
    import rvc_amd.unet as ru
    from rvc_amd.gru import accelerate_f0_rmvpe

    monkeypatch.delenv("RVCMI_RMVPE_UNET", raising=False)
    monkeypatch.delenv("RVCMI_RMVPE_GRU", raising=False)
    assert ru.RMVPE_UNET is False and not ru.unet_on()
    assert {"UNetHIP", "accelerate_rmvpe_unet", "restore_rmvpe_unet"} <= set(rvc_amd.__all__)

    class Net(uc.StandIn):
        def __init__(self):
            super().__init__(uc.key_list(2, 1, 1, 16))
            self.gru = torch.nn.GRU(384, 256, batch_first=True, bidirectional=True)

    # what the helper asks for: recorded, because on a CPU model neither swap would change anything
    import rvc_amd.gru as rg

    calls = []
    monkeypatch.setattr(rg, "accelerate_rmvpe", lambda net: calls.append(("gru", net)) or 0)
    monkeypatch.setattr(ru, "accelerate_rmvpe_unet", lambda net: calls.append(("unet", net)) or 0)
    r = types.SimpleNamespace(model=Net())
    before = dict(r.model.named_modules())
    assert accelerate_f0_rmvpe(r) == 0 and r._rvcmi_gru == 0 and not hasattr(r, "_rvcmi_unet")
    assert calls == [("gru", r.model)] and dict(r.model.named_modules()) == before  # switch off: the GRU swap alone, as before the switch existed
    accelerate_f0_rmvpe(r)
    assert len(calls) == 1
    monkeypatch.setenv("RVCMI_RMVPE_UNET", "1")
    assert ru.unet_on()
    accelerate_f0_rmvpe(r)  # the switch may come on later: the U-Net swap is asked for once, the GRU swap not again
    accelerate_f0_rmvpe(r)
    assert calls == [("gru", r.model), ("unet", r.model)] and r._rvcmi_unet == 0
    monkeypatch.setenv("RVCMI_RMVPE_GRU", "0")
    del calls[:]
    r2 = types.SimpleNamespace(model=Net())
    accelerate_f0_rmvpe(r2)
    assert calls == [("unet", r2.model)]
    monkeypatch.undo()
    monkeypatch.delenv("RVCMI_RMVPE_GRU", raising=False)
    monkeypatch.setenv("RVCMI_RMVPE_UNET", "1")
    r3 = types.SimpleNamespace(model=Net())
    assert accelerate_f0_rmvpe(r3) == 0 and r3._rvcmi_unet == 0 and isinstance(r3.model.unet, uc._UNet)  # the real functions: a CPU model is left alone
    monkeypatch.setenv("RVCMI_RMVPE_UNET", "0")
    monkeypatch.setattr(ru, "RMVPE_UNET", True)
    assert not ru.unet_on()  # the environment's 0 overrides install(rmvpe_unet=True)
    monkeypatch.delenv("RVCMI_RMVPE_UNET")
    assert ru.unet_on()


# ---------------------------------------------------------------- the fp16-operand fp64 oracle (oracle/unet_oracle.py) and the bars derived from it

def _uo():
    from oracle import unet_oracle as uo

    return uo


def test_oracle_without_rounding_is_the_functional_evaluator():
    """fp64, to ~1e-12 of the output's RMS; also with the K dimension summed term by term (which restates the transposed convolution as the
    kernel's four output phases); and the committed goldens of the REAL reference at the tolerance the evaluator is held to."""
    uo = _uo()
    for c in (uc.WHOLE[0], uc.WHOLE[2], uc.WHOLE[3]):
        sd, mel = uc.case_inputs(c)
        sd64 = uc.to(sd, dtype=torch.float64)
        with torch.no_grad():
            ref = uc.forward(sd64, mel.double())
            a = uo.forward(sd64, mel.double(), rounded=False)
            b = uo.forward(sd64, mel.double(), rounded=False, perturb=dict(seed=3, split=True))
        rms = float(ref.pow(2).mean().sqrt())
        assert a["out"].dtype == torch.float64 and len(a["skips"]) == c[0][0]
        assert float((a["out"] - ref).abs().max()) <= 1e-12 * rms and float((b["out"] - ref).abs().max()) <= 1e-12 * rms, uc.case_id(c)
    for name, keys in (("rmvpe_unet_T32.npz", uc.golden_keys()), ("rmvpe_unet_small_T24.npz", None)):
        z = _golden(name)
        if keys is None:
            keys = uc.key_list(int(z["levels"]), int(z["blocks"]), int(z["inters"]), int(z["base"]))
        sd64 = uc.to(uc.seeded_weights(keys, int(z["seed"])), dtype=torch.float64)
        with torch.no_grad():
            out = uo.forward(sd64, torch.from_numpy(z["mel"]).double(), rounded=False)["out"]
        ref = torch.from_numpy(z["out"]).double()
        assert float((out - ref).abs().max()) <= 1e-4 * float(ref.pow(2).mean().sqrt()), name


def test_oracle_rounds_once_and_restates_the_forwards_k_split():
    uo = _uo()
    # a double just above the midpoint of two fp16 values, by less than half a float ulp: through float it would round to even (down)
    v = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30], dtype=torch.float64)
    assert float(uo.r16(v)) == 1.0 + 2.0 ** -10
    # conv() of csrc/unet.hip at the sweep's size: level 0 (8192 pixels, 16 channels: 64 blocks) splits a 3x3 layer in two and leaves a 1x1
    # layer whole; the deepest 3x3 layers (8 pixels, 512 channels: 8 blocks) split in 32; 128 blocks and more: none
    assert uo.forward_ksplit(uo.K_3X3, 16, 16, 8192) == 2 and uo.forward_ksplit(uo.K_1X1, 32, 16, 8192) == 1
    assert uo.forward_ksplit(uo.K_3X3, 512, 512, 8) == 32 and uo.forward_ksplit(uo.K_UP, 512, 256, 8) == 16
    assert uo.forward_ksplit(uo.K_3X3, 16, 16, 128 * 128) == 1 and uo.forward_ksplit(uo.K_HEAD, 16, 3, 64) == 1
    # the trace: every primitive once, operands on the fp16 grid, the next primitive's operand = this one's result rounded ONCE
    trace = uc.sweep_trace()
    kinds = [r["kind"] for r in trace]
    assert len(trace) == 134 and [kinds.count(k) for k in range(7)] == [111, 10, 5, 5, 1, 1, 1]
    assert sum(r["x1"] is not None for r in trace) == 10 and sum(r["res"] is not None for r in trace) == 56
    for r in trace:
        for k in ("x0", "x1", "res"):
            if r[k] is not None and r["kind"] not in (uo.K_FIRST3, uo.K_FIRST1):
                assert torch.equal(r[k], r[k].half().float()), (r["name"], k)
    by = {r["name"]: r for r in trace}
    p = "unet.encoder.layers.1.conv.0"
    assert torch.equal(by[p + ".conv.3"]["x0"], uo.r16(by[p + ".conv.0"]["y"]).float())
    assert torch.equal(by[p + ".conv.3"]["res"], uo.r16(by[p + ".shortcut"]["y"]).float())
    assert tuple(by["cnn"]["y"].shape) == (2, 3, 32, 128) and tuple(by["unet.encoder.layers.4.pool"]["y"].shape) == (2, 256, 1, 4)


def test_skip_offsets_are_those_of_the_workspace_carve():
    offs, end = uc.skip_offsets(1, 32, uc.FULL)
    assert [o for o, _ in offs] == [524288, 655360, 720896, 753664, 770048] and end == 778240  # (of the pinned 1368064 bytes)
    assert [s for _, s in offs] == [(1, 32, 128, 16), (1, 16, 64, 32), (1, 8, 32, 64), (1, 4, 16, 128), (1, 2, 8, 256)]
    offs, end = uc.skip_offsets(1, 6, dict(levels=1, base=48))  # 6 * 128 * 48 * 2 = 73728 = 288 * 256
    assert offs == [(4 * 73728, (1, 6, 128, 48))] and end == 5 * 73728
    offs, end = uc.skip_offsets(1, 2, dict(levels=1, base=16))  # a part that is rounded up: none at these geometries (128 mel bins * 2 bytes = 256)
    assert end == 5 * 8192


_APPLIES = {"res_before_relu": lambda r: r["res"] is not None, "double_round": lambda r: r["res"] is not None, "scale_folded": lambda r: r["bn"],
            "bias_dropped": lambda r: r["name"].endswith(".shortcut"), "concat_swapped": lambda r: r["x1"] is not None,
            "up_flip": lambda r: r["kind"] == 2, "pad_leak": lambda r: r["kind"] == 4, "pool_pairwise": lambda r: r["kind"] == 3}


def _stored(uo, r, y):
    return y.double() if r["kind"] == uo.K_HEAD else uo.r16(y.double()) if y.dtype == torch.float64 else y.half().double()


def test_every_primitive_floor_and_wrong_variants_teacher_forced():
    """Both sides of the per-primitive conditions, for every primitive of the sweep cases.  The fp32 evaluations (torch's summation order, and
    the kernel's chunked / split order permuted) stay within a QUARTER of the flip cap and inside the elementwise bound with no violation --
    also at HALF of GAMMA; the doubly rounded epilogue and the folded scale exceed TWICE the cap on every layer where they apply; every other
    named wrong variant leaves the elementwise bound or the cap on every layer where it applies.  Widening GAMMA or the cap fails here."""
    uo = _uo()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    for c in uc.SWEEP_CPU:
        trace = uc.sweep_trace(c)
        by = {r["name"]: r for r in trace}
        floor = {"f32": [0.0, 0.0], "permuted": [0.0, 0.0]}
        least = {}
        for r in trace:
            for tag, kw in (("f32", {}), ("permuted", dict(perturb=dict(seed=5, split=True)))):
                y32 = uo.eval_prim(r, "f32", **kw)
                ck = uc.prim_check(_stored(uo, r, y32), r, gamma=uc.GAMMA / 2)
                raw = float(((y32.double() - r["y"]).abs() / r["A"].clamp_min(1e-300)).max())
                floor[tag] = [max(floor[tag][0], ck["flips"]), max(floor[tag][1], raw)]
                assert ck["violations"] == 0 and ck["flips"] <= uc.FLIP_CAP / 4, (r["name"], tag, ck)
            for wr, applies in _APPLIES.items():
                if not applies(r):
                    continue
                ck = uc.prim_check(_stored(uo, r, uo.eval_prim(r, "f64", wrong=wr)), r)
                least[wr] = min(least.get(wr, 1.0), ck["flips"])
                if wr in ("double_round", "scale_folded"):
                    assert ck["flips"] > 2 * uc.FLIP_CAP, (r["name"], wr, ck)
                else:
                    assert ck["violations"] > 0 or ck["flips"] > uc.FLIP_CAP, (r["name"], wr, ck)
            if r["name"].endswith(".shortcut"):  # the unrounded shortcut shows in the unit's second convolution, which adds it
                r2 = dict(by[r["name"][:-len(".shortcut")] + ".conv.3"], res=r["y"])
                ck = uc.prim_check(_stored(uo, r2, uo.eval_prim(r2, "f64")), r2)
                least["shortcut_unrounded"] = min(least.get("shortcut_unrounded", 1.0), ck["flips"])
                assert ck["flips"] > 2 * uc.FLIP_CAP, (r2["name"], "shortcut_unrounded", ck)
        print("unet sweep %s: largest flip share / largest |y32 - y| / A: %s; smallest flip share of the wrong variants: %s" % (
            uc.case_id(c), {k: "%.2e / %.2e" % tuple(v) for k, v in floor.items()}, {k: "%.2e" % v for k, v in least.items()}))
        assert sorted(least) == sorted(uo.WRONG)
        assert max(v[1] for v in floor.values()) <= uc.GAMMA / 2  # (measured: 3.8e-7 A, a fifth of GAMMA)


GROSS = ("res_before_relu", "bias_dropped", "concat_swapped", "up_flip", "pad_leak")
# what the whole-network bars do NOT catch reliably -- the per-primitive sweep alone does: at the full network's output each of these sits at
# 1.0 - 1.4 times the floor, inside the bars; the first skip tensor sees the first three at 3 - 8 times its floor, a little over its bar and with
# no margin to speak of, and the pairwise pool (which first acts behind it) nowhere
SWEEP_ONLY = ("double_round", "scale_folded", "shortcut_unrounded", "pool_pairwise")


def test_whole_network_bars_hold_the_perturbed_evaluations_and_refuse_the_gross_variants():
    uo = _uo()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    top = [0.0, 0.0]
    for c in uc.WHOLE:
        sd, mel = uc.case_inputs(c)
        bars = uc.whole_case(c)
        for k, b in bars.items():
            assert b["floor_rms"] > 0 and b["floor_max"] > 0, (uc.case_id(c), k)  # (no zero floor to measure an additive term on: unet_cases.py)
        for seed in (1, 2):
            with torch.no_grad():
                p = uc.stages(uo.forward(sd, mel, arith="f32", perturb=dict(seed=seed, split=True)))
            for k, b in bars.items():
                rms, mx = uc.err(p[k], b["y"])
                top = [max(top[0], rms / b["floor_rms"]), max(top[1], mx / b["floor_max"])]
                print("unet %s %s seed %d: perturbed / floor rms %.2f max %.2f" % (uc.case_id(c), k, seed, rms / b["floor_rms"], mx / b["floor_max"]))
                assert rms <= 0.5 * b["bar_rms"] and mx <= 0.5 * b["bar_max"], (uc.case_id(c), k, seed)
        if c == uc.WHOLE[1]:
            continue  # (the full geometry's variants are shown at B = 1)
        for wr in GROSS + SWEEP_ONLY:
            with torch.no_grad():
                p = uc.stages(uo.forward(sd, mel, wrong=wr))
            over = {k: max(uc.err(p[k], b["y"])[0] / b["bar_rms"], uc.err(p[k], b["y"])[1] / b["bar_max"]) for k, b in bars.items()}
            print("unet %s wrong %s: error / bar %s" % (uc.case_id(c), wr, {k: "%.2f" % v for k, v in over.items()}))
            if wr in GROSS:
                assert max(over.values()) > 2, (uc.case_id(c), wr, over)
            else:
                assert over["out"] < 1, (uc.case_id(c), wr, over)
    print("largest perturbed / floor ratios: rms %.2f max %.2f -> f = %.1f, %.1f" % (top[0], top[1], uc.F_RMS, uc.F_MAX))
    assert 2 * top[0] <= uc.F_RMS and 2 * top[1] <= uc.F_MAX
