"""HuBERT's convolutional feature extractor on the HIP kernels of ``csrc/hubert_fe.hip`` -- like ``unet.py`` BEYOND the scope table
(SURVEY.md section 8).  The transformer behind it, its LayerNorm and ``post_extract_proj`` stay on PyTorch-ROCm / hipBLASLt.

``HubertFrontHIP`` stands in for the ``feature_extractor`` of a HuBERT-base content encoder: fairseq's ``ConvFeatureExtractionModel``
(``extractor_mode="default"``) and transformers' ``HubertFeatureEncoder`` (``feat_extract_norm="group"``) are the same function behind
the same attribute, ``[B, N]`` samples -> ``[B, 512, L]``, ``L = (N - 400) // 320 + 1``.

    n = rvc_amd.accelerate_hubert(model)       # model.feature_extractor -> HubertFrontHIP (same weights); -> number of swaps
    rvc_amd.restore_hubert(model)              # ... and back

Opt-in (``RVCMI_HUBERT_FE=1`` or ``rvc_amd.install(hubert_fe=True)``; default off): parity rests on seeded weights, not on a real
``hubert_base.pt``.  Operands and stored activations are fp16 (like the reference's own ``.half()`` HuBERT), accumulation
and the GELU epilogues fp32, the GroupNorm statistics fp64.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, Optional

import torch

from . import _lib

CHANNELS = 512
KERNELS = (10, 3, 3, 3, 3, 2, 2)
STRIDES = (5, 2, 2, 2, 2, 2, 2)
GN_EPS = 1e-5
HUBERT_FE = False  # install(hubert_fe=True) sets it; RVCMI_HUBERT_FE=1 / =0 overrides it per call
# A swapped extractor hands inputs shorter than this to torch's module.  tools/hubert_fe_time.py (profiles/hubert_fe_time.json) found the HIP
# extractor's range of times below torch's, not overlapping it, at every length it measured; the shortest of those is 1 s, and below it nothing
# is measured, so shorter inputs stay where they were.
MIN_SAMPLES = 16000


def hubert_on() -> bool:
    env = os.environ.get("RVCMI_HUBERT_FE")
    return env == "1" if env in ("0", "1") else bool(HUBERT_FE)


def frames(n: int) -> int:
    """Output frames of an ``n``-sample input (0: too short)."""
    return (int(n) - 400) // 320 + 1 if n >= 400 else 0


_HF_CONV = re.compile(r"conv_layers\.(\d+)\.conv\.(weight|bias)$")
_HF_NORM = re.compile(r"conv_layers\.(\d+)\.layer_norm\.(weight|bias)$")


def canonical_keys(sd) -> Dict[str, torch.Tensor]:
    """The ``conv_layers.*`` tensors of a state dict under fairseq's names (``conv_layers.<i>.0.weight``, ``conv_layers.0.2.weight``):
    transformers' ``conv_layers.<i>.conv.*`` / ``conv_layers.<i>.layer_norm.*`` are renamed, fairseq's pass through, whatever stands in
    front of ``conv_layers.`` is dropped.  Nothing is filtered: a tensor the kernels have no use for makes the C side refuse the lot."""
    out = {}
    for k, v in sd.items():
        at = k.find("conv_layers.")
        if at < 0 or not torch.is_tensor(v):
            continue
        k = k[at:]
        m = _HF_CONV.match(k)
        if m:
            k = "conv_layers.%s.0.%s" % m.groups()
        else:
            m = _HF_NORM.match(k)
            if m:
                k = "conv_layers.%s.2.%s" % m.groups()
        out[k] = v
    return out


def _exact_gelu(act) -> bool:
    probe = torch.tensor([-3.0, -1.0, -0.3, 0.5, 2.0], dtype=torch.float64)
    try:
        with torch.no_grad():
            got = act(probe.clone())
    except Exception:  # noqa  (not a pointwise activation)
        return False
    # (the tanh approximation differs from erf's by up to 2e-4 on these points)
    return torch.is_tensor(got) and got.shape == probe.shape and bool((got.double() - torch.nn.functional.gelu(probe)).abs().max() < 1e-9)


def supported(fe) -> bool:
    """Whether ``fe`` has the STRUCTURE the kernels serve (never its class name): seven ``conv_layers``, each with one bias-free ``Conv1d`` of
    the channels, kernel and stride above (no padding, dilation or groups), a ``GroupNorm(512, 512, eps=1e-5, affine)`` in layer 0 and no
    norm anywhere else, one activation per layer that is the exact GELU, and besides these nothing but dropout."""
    nn = torch.nn
    layers = getattr(fe, "conv_layers", None)
    try:
        layers = list(layers) if layers is not None else None
    except TypeError:
        return False
    if not isinstance(fe, nn.Module) or layers is None or len(layers) != len(KERNELS):
        return False
    for i, layer in enumerate(layers):
        if not isinstance(layer, nn.Module):
            return False
        leaves = [m for m in layer.modules() if not list(m.children())]
        convs = [m for m in leaves if isinstance(m, nn.modules.conv._ConvNd)]
        norms = [m for m in leaves if isinstance(m, (nn.GroupNorm, nn.LayerNorm, nn.modules.batchnorm._NormBase))]
        acts = [m for m in leaves if m not in convs and m not in norms and not isinstance(m, nn.modules.dropout._DropoutNd)]
        if len(convs) != 1 or len(acts) != 1 or len(norms) != (1 if i == 0 else 0):
            return False
        c = convs[0]
        if not isinstance(c, nn.Conv1d) or c.bias is not None or (c.in_channels, c.out_channels) != (CHANNELS if i else 1, CHANNELS) \
                or tuple(c.kernel_size) != (KERNELS[i],) or tuple(c.stride) != (STRIDES[i],) or c.padding not in ((0,), 0, "valid") \
                or tuple(c.dilation) != (1,) or c.groups != 1:
            return False
        if i == 0:
            g = norms[0]
            if not isinstance(g, nn.GroupNorm) or g.num_groups != CHANNELS or g.num_channels != CHANNELS or g.eps != GN_EPS or g.weight is None or g.bias is None:
                return False
        if not _exact_gelu(acts[0]):
            return False
    return True


class HubertFrontHIP(torch.nn.Module):
    """``[B, N]`` (fp16 or fp32, on the handle's GPU) -> ``[B, 512, L]`` in the input dtype: a transposed view of a contiguous ``[B, L, 512]``
    buffer, so the ``.transpose(1, 2)`` that follows the extractor in both HuBERT implementations gives a contiguous tensor without a copy."""

    def __init__(self, state_dict, device):
        super().__init__()
        dev = torch.device(device)
        if dev.type != "cuda":
            raise _lib.RvcmiError("HubertFrontHIP needs a GPU device (got %s); there is no CPU fallback" % dev)
        dev = torch.device("cuda", _lib.device_index(dev))
        keep = [(k, v.detach().float().cpu().contiguous()) for k, v in canonical_keys(state_dict).items() if v.is_floating_point() and 1 <= v.dim() <= 4]
        if not keep:
            raise _lib.RvcmiError("HubertFrontHIP: no 'conv_layers.' weights in the state dict", code=_lib.ERR_INVALID)
        arr = (_lib.Tensor * len(keep))()
        for i, (k, v) in enumerate(keep):
            arr[i].name = k.encode()
            arr[i].data = v.data_ptr()
            arr[i].ndim = v.dim()
            for j, s in enumerate(v.shape):
                arr[i].shape[j] = int(s)
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rvcmi_hubert_fe_create(arr, len(keep), dev.index, C.byref(h)))
        self._h = h
        self._device = dev

    @classmethod
    def from_state_dict(cls, sd, device) -> "HubertFrontHIP":
        return cls(sd, device)

    @classmethod
    def from_module(cls, fe) -> "HubertFrontHIP":
        """From a torch feature extractor on a GPU, fairseq's or transformers' (recognised by ``supported``)."""
        if not supported(fe):
            raise _lib.RvcmiError("HubertFrontHIP: not the feature extractor the kernels serve (HuBERT-base, GroupNorm on layer 0 only, exact "
                                  "GELU, no conv bias)", code=_lib.ERR_INVALID)
        devs = {p.device for p in fe.parameters()}
        if len(devs) != 1:
            raise _lib.RvcmiError("HubertFrontHIP: the module's parameters are on %d devices" % len(devs), code=_lib.ERR_INVALID)
        return cls(fe.state_dict(), next(iter(devs)))

    def __del__(self):
        h = self.__dict__.pop("_h", None)  # (not through nn.Module.__setattr__: it may be gone at interpreter shutdown)
        if h:
            try:
                _lib.lib().rvcmi_hubert_fe_destroy(h)
            except Exception:  # noqa  (interpreter shutdown)
                pass

    def workspace_bytes(self, B: int, N: int) -> int:
        return int(_lib.lib().rvcmi_hubert_fe_workspace_bytes(self._h, int(B), int(N)))

    def forward(self, x: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``workspace``: a uint8 tensor of ``workspace_bytes(B, N)`` bytes to run in (nothing is allocated by the handle then); default: the
        handle's own, which grows on the first call of a larger shape -- such a call must not be inside a stream capture."""
        if not torch.is_tensor(x) or x.device.type != "cuda":
            raise _lib.RvcmiError("HubertFrontHIP input must live on the GPU (got %s); there is no CPU fallback" % getattr(x, "device", type(x)))
        if x.device != self._device:
            raise _lib.RvcmiError("HubertFrontHIP: the input is on %s, the weights on %s" % (x.device, self._device))
        if x.dim() != 2 or x.dtype not in (torch.float16, torch.float32):
            raise _lib.RvcmiError("HubertFrontHIP: expected an fp16 or fp32 [B, N], got %s %s" % (x.dtype, tuple(x.shape)), code=_lib.ERR_INVALID)
        B, N = int(x.shape[0]), int(x.shape[1])
        orig = self.__dict__.get("_original")
        if orig is not None and N < MIN_SAMPLES:
            return orig(x)
        L = frames(N)
        x = x.detach().contiguous()
        out = torch.empty(B, max(L, 0), CHANNELS, device=x.device, dtype=torch.float16)
        ws = 0
        if workspace is not None:
            if workspace.device != x.device or workspace.dtype != torch.uint8 or workspace.numel() < self.workspace_bytes(B, N):
                raise _lib.RvcmiError("HubertFrontHIP: the workspace must be %d uint8 on %s" % (self.workspace_bytes(B, N), x.device), code=_lib.ERR_INVALID)
            ws = workspace.data_ptr()
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().rvcmi_hubert_fe_forward(self._h, B, N, C.c_void_p(x.data_ptr()), 1 if x.dtype == torch.float16 else 0,
                                                          C.c_void_p(out.data_ptr()), C.c_void_p(ws), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
        return out.to(x.dtype).transpose(1, 2)


def debug_conv(x16: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Test hook: one of layers 1 - 6 without its activation.  ``x16`` fp16 ``[B, L_in, 512]`` on a GPU, ``w`` ``[512, 512, taps]`` (torch's
    layout) -> fp32 ``[B, L_out, 512]``."""
    B, L_in, taps = int(x16.shape[0]), int(x16.shape[1]), int(w.shape[2])
    x16 = x16.contiguous()
    wh = w.detach().float().cpu().contiguous()
    out = torch.empty(B, max((L_in - taps) // 2 + 1, 0), CHANNELS, device=x16.device, dtype=torch.float32)
    with torch.cuda.device(x16.device):
        _lib.check(_lib.lib().rvcmi_hubert_fe_debug_conv(taps, B, L_in, C.c_void_p(wh.data_ptr()), C.c_void_p(x16.data_ptr()), C.c_void_p(out.data_ptr()),
                                                         _lib.device_index(x16.device), C.c_void_p(torch.cuda.current_stream(x16.device).cuda_stream)))
    return out


def _holders(model):
    """``model`` when it has a ``feature_extractor`` itself, else the objects one attribute down that do (``HubertProxy.m``)."""
    if isinstance(getattr(model, "feature_extractor", None), torch.nn.Module):
        return [model]
    subs = list(model.children()) if isinstance(model, torch.nn.Module) else []
    subs += [v for v in getattr(model, "__dict__", {}).values() if isinstance(v, torch.nn.Module)]
    out = []
    for m in subs:
        if isinstance(getattr(m, "feature_extractor", None), torch.nn.Module) and not any(m is o for o in out):
            out.append(m)
    return out


def accelerate_hubert(model) -> int:
    """Replace the ``feature_extractor`` of ``model`` (or of the module it holds one attribute down) by a ``HubertFrontHIP`` with the same
    weights, in place.  -> the number of swaps; 0, with nothing modified, for an extractor the kernels do not serve (``supported``), a CPU
    model or one in training mode.  The original stays on the HIP module (unregistered) for ``restore_hubert``."""
    n = 0
    for holder in _holders(model):
        fe = holder.feature_extractor
        if isinstance(fe, HubertFrontHIP) or fe.training or not supported(fe):
            continue
        devs = {p.device for p in fe.parameters()}
        if len(devs) != 1 or next(iter(devs)).type != "cuda":
            continue
        try:
            hip = HubertFrontHIP(fe.state_dict(), next(iter(devs)))
        except _lib.RvcmiError as e:
            if e.code == _lib.ERR_INVALID:  # a configuration the kernels do not serve: torch's module stays
                continue
            raise
        hip.eval()
        object.__setattr__(hip, "_original", fe)  # (not registered: its weights must not appear twice in state_dict())
        holder.feature_extractor = hip
        n += 1
    return n


def restore_hubert(model) -> int:
    """Undo ``accelerate_hubert``.  -> the number of torch modules put back."""
    n = 0
    for holder in _holders(model):
        hip = holder.feature_extractor
        orig = hip.__dict__.get("_original") if isinstance(hip, HubertFrontHIP) else None
        if orig is not None:
            holder.feature_extractor = orig
            n += 1
    getattr(model, "__dict__", {}).pop("_rvcmi_hubert_fe", None)  # (the count accelerate_hubert_once remembered)
    return n


def accelerate_hubert_once(model) -> int:
    """What the conversion paths call in front of ``model.extract_features``: with the switch on, ``accelerate_hubert(model)`` once per
    model object (the count is remembered on it as ``_rvcmi_hubert_fe``); with it off, nothing."""
    if not hubert_on():
        return 0
    n = getattr(model, "_rvcmi_hubert_fe", None)
    if n is None:
        n = accelerate_hubert(model)
        try:
            object.__setattr__(model, "_rvcmi_hubert_fe", n)
        except Exception:  # noqa  (an object without a __dict__: the swap is looked for again next time, and found done)
            pass
    return n
