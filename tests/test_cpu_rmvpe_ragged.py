"""The host side of the ragged batched RMVPE f0 without a GPU: the new entry points in the header, the binding and the built library, the
packing helper, and the refusals that must come before any device call."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import rmvpe_cases as rc  # noqa: E402

NEW = {"rvcmi_unet_workspace_bytes_ragged": (C.c_size_t, 3), "rvcmi_unet_forward_ragged": (C.c_int, 8), "rvcmi_gru_forward_ragged": (C.c_int, 8)}


def test_new_symbols_are_declared_bound_and_built():
    from rvc_amd import _lib

    header = open(os.path.join(ROOT, "include", "rvcmi.h")).read()
    table = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    L = _lib.lib()
    for name, (res, nargs) in NEW.items():
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header)
        assert decl is not None, name + " is not declared in include/rvcmi.h"
        assert len(decl.group(1).split(",")) == nargs == len(table[name][1]) and table[name][0] is res, name
        f = getattr(L, name)
        assert f.restype is res and list(f.argtypes) == table[name][1]
    # the offsets are pointers on both sides; the dense siblings keep their signatures
    assert table["rvcmi_unet_forward"][1] == [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4
    assert table["rvcmi_gru_forward"][1] == [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 4


def test_packing_helper():
    from rvc_amd import RvcmiError
    from rvc_amd.rmvpe import ragged_layout

    frames = [n // rc.HOP + 1 for n in (5120, 513, 5037)]
    assert frames == [33, 4, 32]
    assert ragged_layout(frames) == ([0, 64, 96, 128], 128)
    assert ragged_layout([n // rc.HOP + 1 for n in (48077, 5120)]) == ([0, 320, 384], 384)
    assert ragged_layout([1]) == ([0, 32], 32) and ragged_layout([32, 33]) == ([0, 32, 96], 96)
    off, R = ragged_layout([1001] * 64)
    assert R == 64 * 1024 and off[1] == 1024 and all(b - a == 1024 for a, b in zip(off, off[1:]))
    for bad in ([], [0], [33, -1], [1 << 22, 1]):
        with pytest.raises(RvcmiError):
            ragged_layout(bad)


def test_bad_arguments_raise_before_any_device_call():
    """An object without a handle or weights: anything that reached the device layer would fail with an AttributeError, not an RvcmiError."""
    from rvc_amd import RMVPEHIP, RvcmiError, _lib

    hip = object.__new__(RMVPEHIP)
    hip.device, hip.n_fft, hip.hop_length, hip.is_half = torch.device("cuda", 0), 1024, 160, True
    w = torch.zeros(5120)
    for bad in ([], (), None, w, [w], [w.numpy()], [torch.zeros(2, 5120)]):
        with pytest.raises(RvcmiError):
            hip.salience_batch(bad)
        with pytest.raises(RvcmiError):
            hip.f0_batch(bad, [32])
    # the C entry points refuse a null handle / null offsets without touching a device
    L = _lib.lib()
    off = (C.c_int * 3)(0, 32, 64)
    assert L.rvcmi_unet_workspace_bytes_ragged(None, 2, off) == 0
    assert L.rvcmi_unet_forward_ragged(None, 2, off, None, None, None, None, None) == _lib.ERR_INVALID
    assert L.rvcmi_gru_forward_ragged(None, 2, off, None, None, None, None, None) == _lib.ERR_INVALID


def test_batch_switch(monkeypatch):
    """The group path is a switch inside the opt-in: off unless ``RVCMI_RMVPE_BATCH=1`` (or ``rmvpe.RMVPE_BATCH``), never on without the estimator."""
    from rvc_amd import rmvpe as rm

    monkeypatch.delenv("RVCMI_RMVPE_BATCH", raising=False)
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "1")
    assert rm.rmvpe_batch_on() == bool(rm.RMVPE_BATCH) and rm.RMVPE_BATCH_MIN_FILES >= 2
    monkeypatch.setenv("RVCMI_RMVPE_BATCH", "1")
    assert rm.rmvpe_batch_on()
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "0")
    assert not rm.rmvpe_batch_on()
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "1")
    monkeypatch.setenv("RVCMI_RMVPE_BATCH", "0")
    assert not rm.rmvpe_batch_on()
    monkeypatch.setattr(rm, "RMVPE_BATCH", True)
    assert not rm.rmvpe_batch_on()
    monkeypatch.delenv("RVCMI_RMVPE_BATCH")
    assert rm.rmvpe_batch_on()
