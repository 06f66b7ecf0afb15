"""The deep U-Net of the RMVPE f0 network and its head on the HIP kernels of ``csrc/unet.hip`` -- like ``gru.py`` BEYOND the scope table
(SURVEY.md section 8).  Together with ``GRUHIP`` it leaves only the mel front end and the final ``Linear`` + sigmoid of RMVPE on PyTorch-ROCm;
``rmvpe.py`` (``RMVPEHIP``, its own opt-in switch) puts those two on ``csrc/rmvpe.hip`` as well.

``UNetHIP`` stands in for ``E2E.unet`` (rvc/f0/deepunet.py ``DeepUnet``) AND ``E2E.cnn`` (rvc/f0/e2e.py:29) at once: its forward returns the
head's result, so ``accelerate_rmvpe_unet(model)`` replaces ``model.unet`` by it and ``model.cnn`` by an identity, and the unmodified
``E2E.forward`` (``self.cnn(self.unet(mel)).transpose(1, 2).flatten(-2)``) runs on.

    net = rmvpe.model                          # rvc/f0/rmvpe.py: the E2E network
    rvc_amd.accelerate_rmvpe_unet(net)         # net.unet -> UNetHIP, net.cnn -> Identity (same weights)
    rvc_amd.restore_rmvpe_unet(net)            # ... and back

Opt-in (``RVCMI_RMVPE_UNET=1`` or ``rvc_amd.install(rmvpe_unet=True)``; default off): parity rests on seeded weights, not on a real
``rmvpe.pt``.  Operands and stored activations are fp16 (like the reference's own ``is_half`` RMVPE), accumulation and the
BatchNorm / ReLU / residual epilogues fp32.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import Dict, Optional, Tuple

import torch

from . import _lib

N_MELS = 128
RMVPE_UNET = False  # install(rmvpe_unet=True) sets it; RVCMI_RMVPE_UNET=1 / =0 overrides it per call


unet_on = _lib.Switch("RVCMI_RMVPE_UNET", globals(), "RMVPE_UNET").on


def _unit_keys(p: str, cin: int, cout: int, out: Dict[str, Tuple[int, ...]]) -> None:
    for conv, bn, ci in (("conv.0", "conv.1", cin), ("conv.3", "conv.4", cout)):
        out["%s.%s.weight" % (p, conv)] = (cout, ci, 3, 3)
        _bn_keys("%s.%s" % (p, bn), cout, out)
    if cin != cout:
        out[p + ".shortcut.weight"] = (cout, cin, 1, 1)
        out[p + ".shortcut.bias"] = (cout,)


def _bn_keys(p: str, c: int, out: Dict[str, Tuple[int, ...]]) -> None:
    for k in ("weight", "bias", "running_mean", "running_var"):
        out["%s.%s" % (p, k)] = (c,)
    out[p + ".num_batches_tracked"] = ()


def expected_keys(levels: int, blocks: int, inters: int, base: int, head: int = 3) -> Dict[str, Tuple[int, ...]]:
    """The ``unet.*`` / ``cnn.*`` state-dict keys, with shapes, of ``E2E(blocks, _, (2, 2), levels, inters, 1, base)`` (rvc/f0/e2e.py,
    deepunet.py), in the state dict's order."""
    out: Dict[str, Tuple[int, ...]] = {}
    _bn_keys("unet.encoder.bn", 1, out)
    cin, cout = 1, base
    for l in range(levels):
        for u in range(blocks):
            _unit_keys("unet.encoder.layers.%d.conv.%d" % (l, u), cout if u else cin, cout, out)
        cin, cout = cout, cout * 2
    for i in range(inters):
        for u in range(blocks):
            _unit_keys("unet.intermediate.layers.%d.conv.%d" % (i, u), cout if (i or u) else cin, cout, out)
    cin = cout
    for i in range(levels):
        cout = cin // 2
        out["unet.decoder.layers.%d.conv1.0.weight" % i] = (cin, cout, 3, 3)
        _bn_keys("unet.decoder.layers.%d.conv1.1" % i, cout, out)
        for u in range(blocks):
            _unit_keys("unet.decoder.layers.%d.conv2.%d" % (i, u), cout if u else 2 * cout, cout, out)
        cin = cout
    out["cnn.weight"] = (head, base, 3, 3)
    out["cnn.bias"] = (head,)
    return out


def geometry(shapes: Dict[str, Tuple[int, ...]]) -> Optional[dict]:
    """``{"levels", "blocks", "inters", "base", "head"}`` when the ``unet.`` / ``cnn.`` entries of ``shapes`` (state-dict key -> shape) are
    EXACTLY those of a network ``csrc/unet.hip`` serves (one input channel, channel counts that are multiples of 16), else None."""
    mine = {k: tuple(int(s) for s in v) for k, v in shapes.items() if k.startswith("unet.") or k.startswith("cnn.")}
    w0 = mine.get("unet.encoder.layers.0.conv.0.conv.0.weight")
    wh = mine.get("cnn.weight")
    if w0 is None or wh is None or len(w0) != 4 or len(wh) != 4:
        return None

    def count(pat):
        idx = {int(m.group(1)) for m in (re.match(pat, k) for k in mine) if m}
        return len(idx) if idx == set(range(len(idx))) else -1

    g = dict(levels=count(r"unet\.encoder\.layers\.(\d+)\.conv\.0\.conv\.0\.weight$"),
             blocks=count(r"unet\.encoder\.layers\.0\.conv\.(\d+)\.conv\.0\.weight$"),
             inters=count(r"unet\.intermediate\.layers\.(\d+)\.conv\.0\.conv\.0\.weight$"), base=w0[0], head=wh[0])
    if not (1 <= g["levels"] <= 7 and g["blocks"] >= 1 and g["inters"] >= 1 and g["base"] >= 16 and g["base"] % 16 == 0 and 1 <= g["head"] <= 16):
        return None
    return g if expected_keys(**g) == mine else None


def _pooling_ok(model: torch.nn.Module) -> bool:
    """The state dict does not say how the network pools: every parameter-free leaf module with a ``kernel_size`` must pool (2, 2) (containers that merely remember one, possibly None, do not count), and every
    transposed convolution must be (3x3, stride 2, padding 1, output_padding 1)."""
    def pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    for m in model.modules():
        if getattr(m, "transposed", False) and hasattr(m, "weight"):  # (every torch convolution has `output_padding`; only these are transposed)
            if (pair(m.stride), pair(m.padding), pair(m.output_padding), pair(getattr(m, "dilation", 1))) != ((2, 2), (1, 1), (1, 1), (1, 1)):
                return False
        elif getattr(m, "kernel_size", None) is not None and not hasattr(m, "weight") and not list(m.children()):  # a pooling leaf
            stride = m.stride if getattr(m, "stride", None) is not None else m.kernel_size
            if pair(m.kernel_size) != (2, 2) or pair(stride) != (2, 2) or pair(getattr(m, "padding", 0)) != (0, 0):
                return False
    return True


class UNetHIP(torch.nn.Module):
    """``[B, 1, T, 128]`` (any float dtype, on the handle's GPU) -> ``[B, head, T, 128]`` in the input dtype: a permuted view of a contiguous
    ``[B, T, head, 128]`` buffer, so the ``.transpose(1, 2).flatten(-2)`` of rvc/f0/e2e.py:46 gives a contiguous ``[B, T, head * 128]``
    without a copy."""

    def __init__(self, state_dict, device):
        super().__init__()
        dev = _lib.cuda_device(device, "UNetHIP")
        arr = _lib.pack_tensors((k, v.detach().float().cpu().contiguous()) for k, v in state_dict.items()
                                if k.startswith(("unet.", "cnn.")) and torch.is_tensor(v) and v.is_floating_point() and 1 <= v.dim() <= 4)
        if not len(arr):
            raise _lib.RvcmiError("UNetHIP: no 'unet.' / 'cnn.' weights in the state dict", code=_lib.ERR_INVALID)
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rvcmi_unet_create(arr, len(arr), dev.index, C.byref(h)))
        self._h = _lib.Handle("rvcmi_unet_destroy", h)
        self._device = dev
        self.head_channels = int(_lib.lib().rvcmi_unet_head_channels(h))
        self.geometry = geometry({k: tuple(v.shape) for k, v in state_dict.items() if torch.is_tensor(v)})

    @classmethod
    def from_state_dict(cls, sd, device) -> "UNetHIP":
        return cls(sd, device)

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(_lib.lib().rvcmi_unet_workspace_bytes(self._h, int(B), int(T)))

    def forward(self, mel: torch.Tensor) -> torch.Tensor:
        _lib.require_on(mel, self._device, "UNetHIP")
        if mel.dim() != 4 or mel.shape[1] != 1 or mel.shape[3] != N_MELS or not mel.is_floating_point():
            raise _lib.RvcmiError("UNetHIP: expected a float [B, 1, T, %d], got %s %s" % (N_MELS, mel.dtype, tuple(mel.shape)), code=_lib.ERR_INVALID)
        B, T = int(mel.shape[0]), int(mel.shape[2])
        nbytes = self.workspace_bytes(B, T) if B and T else 0
        if not nbytes:
            msg = _lib.lib().rvcmi_last_error()
            raise _lib.RvcmiError("UNetHIP: B = %d, T = %d not served (%s)" % (B, T, msg.decode(errors="replace") if msg else "?"), code=_lib.ERR_INVALID)
        x = mel.detach().to(torch.float32).contiguous()
        out = torch.empty(B, T, self.head_channels, N_MELS, device=mel.device, dtype=torch.float32)
        ws = torch.empty(nbytes, device=mel.device, dtype=torch.uint8)  # torch's caching allocator: no hipMalloc inside a capture
        with torch.cuda.device(mel.device):
            _lib.check(_lib.lib().rvcmi_unet_forward(self._h, B, T, _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), _lib.stream_ptr(mel.device)))
        return out.to(mel.dtype).permute(0, 2, 1, 3)


def accelerate_rmvpe_unet(model) -> int:
    """Replace ``model.unet`` by a ``UNetHIP`` with the same weights and ``model.cnn`` by an identity, in place, when ``model`` is on a GPU and
    the ``unet.`` / ``cnn.`` keys and shapes of its state dict are those of a network the kernels serve (recognised by keys, not by class).
    -> 1, or 0 with the model untouched.  The originals stay on the HIP module (unregistered) for ``restore_rmvpe_unet``."""
    if not isinstance(model, torch.nn.Module) or not isinstance(getattr(model, "unet", None), torch.nn.Module) \
            or not isinstance(getattr(model, "cnn", None), torch.nn.Module) or isinstance(model.unet, UNetHIP):
        return 0
    sd = model.state_dict()
    if geometry({k: tuple(v.shape) for k, v in sd.items()}) is None or not _pooling_ok(model.unet):
        return 0
    devs = {v.device for k, v in sd.items() if k.startswith("unet.") or k.startswith("cnn.")}
    if len(devs) != 1 or next(iter(devs)).type != "cuda":
        return 0
    try:
        hip = UNetHIP(sd, next(iter(devs)))
    except _lib.RvcmiError as e:
        if e.code == _lib.ERR_INVALID:  # a configuration the kernels do not serve: torch's modules stay
            return 0
        raise
    object.__setattr__(hip, "_originals", (model.unet, model.cnn))  # (not registered: their weights must not reappear in state_dict())
    model.unet = hip
    model.cnn = torch.nn.Identity()
    return 1


def restore_rmvpe_unet(model) -> int:
    """Undo ``accelerate_rmvpe_unet``.  -> 1 when the torch modules were put back."""
    hip = getattr(model, "unet", None)
    orig = getattr(hip, "_originals", None) if isinstance(hip, UNetHIP) else None
    if orig is None:
        return 0
    model.unet, model.cnn = orig
    return 1
