"""CPU side of the RMVPE U-Net work (csrc/unet.hip, rvc_amd/unet.py): the tests' own functional evaluator against the REAL reference's
output, the conditions that make the seeded weights a meaningful parity case, the recogniser, the ABI symbols, the default-off switch."""
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
