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

Several inputs in ONE pass (opt-in on top of the above: ``RVCMI_HUBERT_BATCH=1`` or ``rvc_amd.install(hubert_batch=True)``):
``HubertFrontHIP.forward_ragged`` runs a zero-padded ``[B, N_max]`` batch whose items keep their own lengths -- layer 0's GroupNorm averages
over the item's own frames, not over the padding -- and ``extract_features_batch`` hands such a batch to a fairseq-shaped model together
with a sample mask (``sample_mask``) from which fairseq's ``forward_padding_mask`` derives exactly the frames behind each item's end.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import contextlib
from typing import Dict, List, Optional, Sequence

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
HUBERT_BATCH = False  # install(hubert_batch=True) sets it; RVCMI_HUBERT_BATCH=1 / =0 overrides it per call.  Effective only with the switch above.
# tools/hubert_batch_time.py (profiles/hubert_batch_time.json) found the batched call's range of times below the per-item loop's, not overlapping it, at
# 2, 8 and 64 items of 12 s and on a mixed group of 3 - 12 s, for the extractor alone and for a fairseq-shaped HuBERT-base.  The switch stays off all the
# same: that model is a stand-in with random weights, and the effect on a whole conversion is unmeasured.
HUBERT_BATCH_MIN_ITEMS = 2    # with the switch on, a planned group of at least this many segments takes the batched call (2 x 12 s: 6.93 -> 5.06 ms)
# A group's padded samples B * N_max may exceed the sum of its lengths by this fraction.  Measured on the mixed group planned at 0 / 0.1 / 0.25 / 0.5 / 1.0:
# 37.5 / 22.8 / 13.9 / 11.4 / 10.8 ms against the loop's 40 - 42 -- fewer, larger groups won at every step.  At 1.0 the one group's actual waste was 0.57,
# so a waste above that is unmeasured, and the bound stays at the largest setting that keeps every group inside what was.
HUBERT_BATCH_MAX_WASTE = 0.5
HUBERT_BATCH_MAX_SAMPLES = 64 * 12 * 16000  # B * N_max of one group (the extractor's workspace takes ~310 bytes per sample): the largest shape the timing tool runs


def hubert_on() -> bool:
    env = os.environ.get("RVCMI_HUBERT_FE")
    return env == "1" if env in ("0", "1") else bool(HUBERT_FE)


def hubert_batch_on() -> bool:
    env = os.environ.get("RVCMI_HUBERT_BATCH")
    return hubert_on() and (env == "1" if env in ("0", "1") else bool(HUBERT_BATCH))


def frames(n: int) -> int:
    """Output frames of an ``n``-sample input (0: too short)."""
    return (int(n) - 400) // 320 + 1 if n >= 400 else 0


def _lens_list(lens) -> List[int]:
    if torch.is_tensor(lens):
        lens = lens.tolist()
    return [int(n) for n in lens]


def frame_mask(lens, N_max: int) -> torch.Tensor:
    """bool ``[B, frames(N_max)]`` (on the host), True where ``t >= frames(lens[i])``: the frames item ``i``'s own call never computes."""
    lens = _lens_list(lens)
    t = torch.arange(frames(N_max)).unsqueeze(0)
    return t >= torch.tensor([frames(n) for n in lens], dtype=torch.long).unsqueeze(1)


def sample_mask(lens, N_max: int) -> torch.Tensor:
    """bool ``[B, N_max]`` (on the host) from which fairseq's ``forward_padding_mask`` -- drop the ``N_max % L_max`` tail,
    ``view(B, L_max, -1).all(-1)`` -- derives exactly ``frame_mask(lens, N_max)``: samples ``[t c, (t + 1) c)``, ``c = N_max // L_max``, are set
    for every padded frame ``t`` and nothing else.  (The plain mask, True from sample ``lens[i]`` on, leaves one frame too many unmasked
    whenever ``lens[i]`` is not a multiple of ``c``: that rule is only approximate.)"""
    fm = frame_mask(lens, N_max)
    B, L = fm.shape
    if L < 1:
        raise _lib.RvcmiError("sample_mask: N_max = %d is shorter than one frame (400 samples)" % N_max, code=_lib.ERR_INVALID)
    c = int(N_max) // L
    out = torch.zeros(B, int(N_max), dtype=torch.bool)
    out[:, :L * c] = fm.unsqueeze(2).expand(B, L, c).reshape(B, L * c)
    return out


def plan_groups(lens, max_waste: Optional[float] = None, max_samples: Optional[int] = None) -> List[List[int]]:
    """Host only.  Which inputs share a padded batch: the indices sorted by length (ties by index), consecutive runs packed while
    ``B * N_max <= (1 + max_waste) * sum(lens)`` holds for the run (and ``B * N_max <= max_samples``).  -> lists of indices, every input in
    exactly one; inputs under ``MIN_SAMPLES`` (below it nothing is measured) come back alone.  The same input gives the same plan."""
    lens = _lens_list(lens)
    w = HUBERT_BATCH_MAX_WASTE if max_waste is None else float(max_waste)
    cap = HUBERT_BATCH_MAX_SAMPLES if max_samples is None else int(max_samples)
    if w < 0:
        raise ValueError("max_waste must be >= 0")
    order = sorted(range(len(lens)), key=lambda i: (lens[i], i))
    groups, cur, total = [], [], 0
    for i in order:
        n = lens[i]
        if n < MIN_SAMPLES:
            groups.append([i])
            continue
        # (ascending: n is the run's N_max once i has joined it)
        if cur and (len(cur) + 1) * n <= (1.0 + w) * (total + n) and (len(cur) + 1) * n <= cap:
            cur.append(i)
            total += n
        else:
            if cur:
                groups.append(cur)
            cur, total = [i], n
    if cur:
        groups.append(cur)
    return groups


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

    def workspace_bytes_ragged(self, B: int, N_max: int) -> int:
        return int(_lib.lib().rvcmi_hubert_fe_workspace_bytes_ragged(self._h, int(B), int(N_max)))

    _LENS_KEPT = 64

    def _lens_dev(self, lens: tuple) -> torch.Tensor:
        """The lengths on the device.  The last ``_LENS_KEPT`` tuples are kept (a group converted again uploads nothing); one used inside a stream
        capture is kept for the handle's life, since the graph's kernels read it on every replay."""
        kept = self.__dict__.setdefault("_lens_kept", {})
        held = self.__dict__.setdefault("_lens_held", {})
        t = held.get(lens)
        if t is None:
            t = kept.pop(lens, None)
        capturing = torch.cuda.is_current_stream_capturing()
        if t is None:
            if capturing:
                raise _lib.RvcmiError("HubertFrontHIP.forward_ragged: these lengths are not on the device yet, and an upload cannot be captured; "
                                      "call once with them before the capture (as for the handle's own workspace)")
            t = torch.tensor(lens, dtype=torch.int32).to(self._device)
        if capturing:
            held[lens] = t
        elif lens not in held:
            kept[lens] = t  # (re-inserted: most recently used last)
            while len(kept) > self._LENS_KEPT:
                kept.pop(next(iter(kept)))
        return t

    def forward_ragged(self, x: torch.Tensor, lens, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``x`` ``[B, N_max]``: item ``i`` is its first ``lens[i]`` samples (host ints; at least 400 each, the longest ``N_max``); whatever
        lies behind them is not read.  -> the same transposed view as ``forward``, ``[B, 512, frames(N_max)]``: item ``i``'s first
        ``frames(lens[i])`` frames are bit-equal to ``forward`` of that item alone, the frames behind them exactly zero.  ``workspace``: as in
        ``forward`` (``workspace_bytes_ragged(B, N_max)`` bytes).  Inside a stream capture the lengths must have been used once before."""
        if not torch.is_tensor(x) or x.device.type != "cuda":
            raise _lib.RvcmiError("HubertFrontHIP input must live on the GPU (got %s); there is no CPU fallback" % getattr(x, "device", type(x)))
        if x.device != self._device:
            raise _lib.RvcmiError("HubertFrontHIP: the input is on %s, the weights on %s" % (x.device, self._device))
        if x.dim() != 2 or x.dtype not in (torch.float16, torch.float32):
            raise _lib.RvcmiError("HubertFrontHIP: expected an fp16 or fp32 [B, N_max], got %s %s" % (x.dtype, tuple(x.shape)), code=_lib.ERR_INVALID)
        lens = tuple(_lens_list(lens))
        B, N = int(x.shape[0]), int(x.shape[1])
        if len(lens) != B or B < 1 or min(lens) < 400 or max(lens) != N:
            raise _lib.RvcmiError("HubertFrontHIP.forward_ragged: lens %s do not fit an input of shape %s (one length per item, each >= 400, the "
                                  "longest equal to N_max)" % (list(lens[:8]), tuple(x.shape)), code=_lib.ERR_INVALID)
        x = x.detach().contiguous()
        out = torch.empty(B, frames(N), CHANNELS, device=x.device, dtype=torch.float16)
        ws = 0
        if workspace is not None:
            need = self.workspace_bytes_ragged(B, N)
            if workspace.device != x.device or workspace.dtype != torch.uint8 or workspace.numel() < need or need == 0:
                raise _lib.RvcmiError("HubertFrontHIP: the workspace must be %d uint8 on %s" % (need, x.device), code=_lib.ERR_INVALID)
            ws = workspace.data_ptr()
        host = (C.c_int * B)(*lens)
        dev = self._lens_dev(lens)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().rvcmi_hubert_fe_forward_ragged(self._h, B, N, host, C.c_void_p(dev.data_ptr()), C.c_void_p(x.data_ptr()),
                                                                 1 if x.dtype == torch.float16 else 0, C.c_void_p(out.data_ptr()), C.c_void_p(ws),
                                                                 C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
        return out.to(x.dtype).transpose(1, 2)

    @contextlib.contextmanager
    def ragged(self, lens):
        """Inside the block the plain ``forward(x)`` -- what a model calls on its ``feature_extractor`` -- is ``forward_ragged(x, lens)``: how
        the lengths reach an extractor the model calls itself.  An ``x`` that does not fit ``lens`` raises.  Cleared on exit, exceptions too."""
        lens = tuple(_lens_list(lens))
        if self.__dict__.get("_ragged") is not None:
            raise _lib.RvcmiError("HubertFrontHIP.ragged: already inside a ragged block")
        object.__setattr__(self, "_ragged", lens)
        try:
            yield self
        finally:
            object.__setattr__(self, "_ragged", None)

    def forward(self, x: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``workspace``: a uint8 tensor of ``workspace_bytes(B, N)`` bytes to run in (nothing is allocated by the handle then); default: the
        handle's own, which grows on the first call of a larger shape -- such a call must not be inside a stream capture."""
        lens = self.__dict__.get("_ragged")
        if lens is not None:
            return self.forward_ragged(x, lens, workspace)
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


def batch_capable(model) -> bool:
    """Whether ``extract_features_batch`` may run ``model``, by structure (like ``supported``): its ``feature_extractor`` is a swapped
    ``HubertFrontHIP``, it is on the GPU and in eval mode, and it has fairseq's ``forward_padding_mask`` -- the method through which a
    sample mask becomes the frame mask the encoder honours.  A model without it (one that ignores ``padding_mask``) would attend to the padding."""
    fe = getattr(model, "feature_extractor", None)
    if not isinstance(model, torch.nn.Module) or not isinstance(fe, HubertFrontHIP) or fe.__dict__.get("_original") is None:
        return False
    if model.training or not callable(getattr(model, "forward_padding_mask", None)) or not callable(getattr(model, "extract_features", None)):
        return False
    devs = {p.device for p in model.parameters()}
    return len(devs) == 1 and next(iter(devs)) == fe._device


def extract_features_batch(model, wavs: Sequence[torch.Tensor], output_layer) -> List[torch.Tensor]:
    """``model.extract_features`` for SEVERAL waveforms (1-D, one dtype, fp16 or fp32; each at least 400 samples) in one call: zero-padded to the
    longest, the extractor told the lengths (``HubertFrontHIP.ragged``), the model handed ``sample_mask`` -- so a padded frame is zeroed in front
    of ``pos_conv`` and masked as an attention key, and no item sees another's or its own padding.  -> one ``[1, L_i, d]`` tensor per input,
    ``L_i = frames(len(wavs[i]))``.  The extractor's rows are bit-equal to the lone calls'; the transformer's GEMMs see another M, so the result
    equals the lone call's to operand rounding."""
    if not batch_capable(model):
        raise _lib.RvcmiError("extract_features_batch: the model is not batch_capable (swapped HubertFrontHIP extractor, GPU, eval mode, "
                              "forward_padding_mask)", code=_lib.ERR_INVALID)
    fe = model.feature_extractor
    wavs = [torch.as_tensor(w) for w in wavs]
    if not wavs or any(w.dim() != 1 for w in wavs) or len({w.dtype for w in wavs}) != 1:
        raise _lib.RvcmiError("extract_features_batch: expected 1-D waveforms of one dtype", code=_lib.ERR_INVALID)
    lens = [int(w.shape[0]) for w in wavs]
    N = max(lens)
    x = torch.zeros(len(wavs), N, dtype=wavs[0].dtype, device=fe._device)
    for i, w in enumerate(wavs):
        x[i, :lens[i]] = w.to(fe._device)
    mask = sample_mask(lens, N).to(fe._device)
    with torch.no_grad(), fe.ragged(lens):
        logits = model.extract_features(source=x, padding_mask=mask, output_layer=output_layer)
    y = logits[0]
    if y.dim() != 3 or int(y.shape[0]) != len(wavs) or int(y.shape[1]) != frames(N):
        raise _lib.RvcmiError("extract_features_batch: the model returned %s for %d items of %d frames" % (tuple(y.shape), len(wavs), frames(N)))
    return [y[i:i + 1, :frames(n)].contiguous() for i, n in enumerate(lens)]


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
