"""TorchGateHIP's host side (rvc_amd/gate.py): the smoothing filter against the reference's own (tests/golden/gui_torchgate.npz,
tools/make_golden_gate.py), the constructor's errors, no CPU fallback, and install(patch_gui=True) / uninstall()."""
import sys
import types

import numpy as np
import pytest
import torch

from conftest import load_golden

RATES = (48000, 44100, 40000, 32000, 22050)


@pytest.mark.parametrize("sr", RATES)
def test_smoothing_filter_is_the_references(sr):
    """Built on the host exactly as torchgate.py:75-127 builds it: equal bit for bit, in fp32 and under an fp64 default dtype."""
    import rvc_amd

    d = load_golden("gui_torchgate")
    tg = rvc_amd.TorchGateHIP(sr=sr, n_fft=4 * (sr // 100), prop_decrease=0.9)
    f = tg.smoothing_filter
    assert f.dtype == torch.float32 and tuple(f.shape) == (1, 1) + d["filter%d_32" % sr].shape
    assert np.array_equal(f[0, 0].numpy(), d["filter%d_32" % sr])
    assert f.shape[-2:] == ((19, 11) if sr == 22050 else (21, 11))
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        f64 = rvc_amd.TorchGateHIP(sr=sr, n_fft=4 * (sr // 100), prop_decrease=0.9).smoothing_filter
    finally:
        torch.set_default_dtype(prev)
    assert f64.dtype == torch.float64 and np.array_equal(f64[0, 0].numpy(), d["filter%d_64" % sr])


def test_constructor_matches_the_reference_signature_and_errors():
    import inspect

    import rvc_amd

    params = inspect.signature(rvc_amd.TorchGateHIP.__init__).parameters
    assert list(params)[1:] == ["sr", "nonstationary", "n_std_thresh_stationary", "n_thresh_nonstationary", "temp_coeff_nonstationary",
                                "n_movemean_nonstationary", "prop_decrease", "n_fft", "win_length", "hop_length", "freq_mask_smooth_hz",
                                "time_mask_smooth_ms"]
    assert [params[k].default for k in list(params)[2:]] == [False, 1.5, 1.3, 0.1, 20, 1.0, 1024, None, None, 500, 50]
    tg = rvc_amd.TorchGateHIP(sr=48000)
    assert (tg.n_fft, tg.win_length, tg.hop_length, tg.prop_decrease) == (1024, 1024, 256, 1.0)
    assert list(tg.state_dict()) == ["smoothing_filter"]
    for bad in (-0.1, 1.5):
        with pytest.raises(AssertionError):
            rvc_amd.TorchGateHIP(sr=48000, prop_decrease=bad)
    with pytest.raises(ValueError, match="time_mask_smooth_ms"):
        rvc_amd.TorchGateHIP(sr=48000, n_fft=1920, time_mask_smooth_ms=5)
    # the reference means to raise this ValueError; its message formats the missing self._n_fft (AttributeError instead)
    with pytest.raises(ValueError, match="freq_mask_smooth_hz"):
        rvc_amd.TorchGateHIP(sr=48000, n_fft=1920, freq_mask_smooth_hz=20)
    assert rvc_amd.TorchGateHIP(sr=48000, freq_mask_smooth_hz=None, time_mask_smooth_ms=None).smoothing_filter is None


def test_cpu_tensor_raises():
    import rvc_amd

    tg = rvc_amd.TorchGateHIP(sr=48000, n_fft=1920, prop_decrease=0.9)
    with pytest.raises(rvc_amd.RvcmiError):
        tg(torch.zeros(1, 4800), torch.zeros(1, 9600))
    with pytest.raises(rvc_amd.RvcmiError):
        tg(torch.zeros(4800))
    w = torch.zeros(1920, dtype=torch.float64)
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.glue.spectral_gate(torch.zeros(1, 4800), None, 1920, 480, w)


def test_realtime_stream_keywords_default_to_the_vc_block():
    import inspect

    import rvc_amd

    params = inspect.signature(rvc_amd.RealtimeStream.__init__).parameters
    assert params["I_noise_reduce"].default is False and params["O_noise_reduce"].default is False
    assert params["function"].default == "vc"
    with pytest.raises(ValueError, match="samplerate"):
        rvc_amd.RealtimeStream(None, function="im")


def test_install_patch_gui_rebinds_torchgate(monkeypatch):
    """install(patch_gui=True) rebinds TorchGate where gui.py imports it (infer.modules.gui) and where it is defined
    (infer.modules.gui.torchgate); uninstall() restores both; the default install() leaves them alone."""
    import os

    import rvc_amd

    skel = os.path.join(os.path.dirname(os.path.abspath(__file__)), "skeleton")
    for m in [m for m in sys.modules if m.split(".")[0] in ("rvc", "infer")]:
        monkeypatch.delitem(sys.modules, m)
    monkeypatch.syspath_prepend(skel)
    import infer.modules  # noqa: F401  (the skeleton package the stand-ins hang under)

    class TorchGate(torch.nn.Module):
        pass

    gui = types.ModuleType("infer.modules.gui")
    tgm = types.ModuleType("infer.modules.gui.torchgate")
    gui.TorchGate = tgm.TorchGate = TorchGate
    monkeypatch.setitem(sys.modules, "infer.modules.gui", gui)
    monkeypatch.setitem(sys.modules, "infer.modules.gui.torchgate", tgm)
    try:
        rvc_amd.install()
        assert gui.TorchGate is TorchGate and tgm.TorchGate is TorchGate
        rvc_amd.uninstall()
        rvc_amd.install(patch_gui=True)
        assert gui.TorchGate is rvc_amd.TorchGateHIP and tgm.TorchGate is rvc_amd.TorchGateHIP
        rvc_amd.uninstall()
        assert gui.TorchGate is TorchGate and tgm.TorchGate is TorchGate
    finally:
        rvc_amd.uninstall()
        for m in [m for m in sys.modules if m.split(".")[0] in ("rvc", "infer")]:
            del sys.modules[m]
