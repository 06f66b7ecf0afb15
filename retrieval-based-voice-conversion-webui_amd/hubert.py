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

The transformer's LAYERS on ``csrc/hubert_enc.hip`` (a switch of its own, ``RVCMI_HUBERT_ENC=1`` or ``rvc_amd.install(hubert_enc=True)``; default off;
DESIGN.md 7.9): ``accelerate_hubert_layers(model)`` swaps every post-norm layer of ``model.encoder.layers`` for a ``HubertLayerHIP`` on one
``HubertEncoderHIP`` -- all layers or none -- and ``restore_hubert_layers`` puts torch's back.  ``pos_conv``, the feature projection, the encoder's own
LayerNorm, ``final_proj`` and the loop over the layers stay on torch.  Measured slower than torch's layers at every shape today
(profiles/hubert_enc_time.json): the switch is for whoever wants the kernels' rounding, not for speed.
"""
from __future__ import annotations

import ctypes as C
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


_FE = _lib.Switch("RVCMI_HUBERT_FE", globals(), "HUBERT_FE")
_BATCH = _lib.Switch("RVCMI_HUBERT_BATCH", globals(), "HUBERT_BATCH", base=_FE)
hubert_on, hubert_batch_on = _FE.on, _BATCH.on


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
        dev = _lib.cuda_device(device, "HubertFrontHIP")
        arr = _lib.pack_tensors((k, v.detach().float().cpu().contiguous()) for k, v in canonical_keys(state_dict).items()
                                if v.is_floating_point() and 1 <= v.dim() <= 4)
        if not len(arr):
            raise _lib.RvcmiError("HubertFrontHIP: no 'conv_layers.' weights in the state dict", code=_lib.ERR_INVALID)
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rvcmi_hubert_fe_create(arr, len(arr), dev.index, C.byref(h)))
        self._h = _lib.Handle("rvcmi_hubert_fe_destroy", h)
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
        _lib.require_on(x, self._device, "HubertFrontHIP")
        if x.dim() != 2 or x.dtype not in (torch.float16, torch.float32):
            raise _lib.RvcmiError("HubertFrontHIP: expected an fp16 or fp32 [B, N_max], got %s %s" % (x.dtype, tuple(x.shape)), code=_lib.ERR_INVALID)
        lens = tuple(_lens_list(lens))
        B, N = int(x.shape[0]), int(x.shape[1])
        if len(lens) != B or B < 1 or min(lens) < 400 or max(lens) != N:
            raise _lib.RvcmiError("HubertFrontHIP.forward_ragged: lens %s do not fit an input of shape %s (one length per item, each >= 400, the "
                                  "longest equal to N_max)" % (list(lens[:8]), tuple(x.shape)), code=_lib.ERR_INVALID)
        x = x.detach().contiguous()
        out = torch.empty(B, frames(N), CHANNELS, device=x.device, dtype=torch.float16)
        ws = None if workspace is None else _lib.workspace_ptr(workspace, self.workspace_bytes_ragged(B, N), x.device, "HubertFrontHIP")
        host = (C.c_int * B)(*lens)
        dev = self._lens_dev(lens)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().rvcmi_hubert_fe_forward_ragged(self._h, B, N, host, _lib.ptr(dev), _lib.ptr(x), 1 if x.dtype == torch.float16 else 0,
                                                                 _lib.ptr(out), ws, _lib.stream_ptr(x.device)))
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
        _lib.require_on(x, self._device, "HubertFrontHIP")
        if x.dim() != 2 or x.dtype not in (torch.float16, torch.float32):
            raise _lib.RvcmiError("HubertFrontHIP: expected an fp16 or fp32 [B, N], got %s %s" % (x.dtype, tuple(x.shape)), code=_lib.ERR_INVALID)
        B, N = int(x.shape[0]), int(x.shape[1])
        orig = self.__dict__.get("_original")
        if orig is not None and N < MIN_SAMPLES:
            return orig(x)
        L = frames(N)
        x = x.detach().contiguous()
        out = torch.empty(B, max(L, 0), CHANNELS, device=x.device, dtype=torch.float16)
        ws = None if workspace is None else _lib.workspace_ptr(workspace, self.workspace_bytes(B, N), x.device, "HubertFrontHIP")
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().rvcmi_hubert_fe_forward(self._h, B, N, _lib.ptr(x), 1 if x.dtype == torch.float16 else 0, _lib.ptr(out), ws,
                                                          _lib.stream_ptr(x.device)))
        return out.to(x.dtype).transpose(1, 2)


def debug_conv(x16: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Test hook: one of layers 1 - 6 without its activation.  ``x16`` fp16 ``[B, L_in, 512]`` on a GPU, ``w`` ``[512, 512, taps]`` (torch's
    layout) -> fp32 ``[B, L_out, 512]``."""
    B, L_in, taps = int(x16.shape[0]), int(x16.shape[1]), int(w.shape[2])
    x16 = x16.contiguous()
    wh = w.detach().float().cpu().contiguous()
    out = torch.empty(B, max((L_in - taps) // 2 + 1, 0), CHANNELS, device=x16.device, dtype=torch.float32)
    with torch.cuda.device(x16.device):
        _lib.check(_lib.lib().rvcmi_hubert_fe_debug_conv(taps, B, L_in, _lib.ptr(wh), _lib.ptr(x16), _lib.ptr(out), _lib.device_index(x16.device),
                                                         _lib.stream_ptr(x16.device)))
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
    return _lib.once(model, "_rvcmi_hubert_fe", lambda: accelerate_hubert(model)) if hubert_on() else 0


# ---- the transformer's layers on csrc/hubert_enc.hip (opt-in: RVCMI_HUBERT_ENC=1 or rvc_amd.install(hubert_enc=True); default off) ----
# Only the repeated block x = LN(x + Attn(x)); x = LN(x + FFN(x)) is served.  LayerNorm + post_extract_proj, pos_conv, the encoder's own LayerNorm,
# final_proj and the loop over the layers stay on torch: the integration point is the single layer module, so output_layer = 9 / 12 and the ragged
# batched path (a padding mask) need no plumbing of their own.
HUBERT_ENC = False  # install(hubert_enc=True) sets it; RVCMI_HUBERT_ENC=1 / =0 overrides it per call.  Independent of HUBERT_FE.
HEAD_DIM = 64
_LAYER_TENSORS = tuple("%s.%s" % (m, p) for m in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "self_attn_layer_norm",
                                                  "fc1", "fc2", "final_layer_norm") for p in ("weight", "bias"))


hubert_enc_on = _lib.Switch("RVCMI_HUBERT_ENC", globals(), "HUBERT_ENC").on


def _layer_parts(m):
    """-> (convention, {canonical name: module}, activation, attention module) of a layer under either convention's attribute names, else None."""
    sub = lambda o, *names: [getattr(o, n, None) for n in names]
    att = getattr(m, "self_attn", None)
    if att is not None:
        conv, ln1, fc1, fc2, ln2, act = "fairseq", *sub(m, "self_attn_layer_norm", "fc1", "fc2", "final_layer_norm", "activation_fn")
    else:
        att, ff = getattr(m, "attention", None), getattr(m, "feed_forward", None)
        conv, ln1, ln2 = "transformers", *sub(m, "layer_norm", "final_layer_norm")
        fc1, fc2, act = sub(ff, "intermediate_dense", "output_dense", "intermediate_act_fn")
    q, k, v, o = sub(att, "q_proj", "k_proj", "v_proj", "out_proj")
    parts = {"self_attn.q_proj": q, "self_attn.k_proj": k, "self_attn.v_proj": v, "self_attn.out_proj": o, "self_attn_layer_norm": ln1, "fc1": fc1,
             "fc2": fc2, "final_layer_norm": ln2}
    if any(p is None for p in parts.values()) or act is None:
        return None
    return conv, parts, act, att


def _layer_cfg(m) -> Optional[dict]:
    """The geometry of a layer the kernels serve (``supported_layer``), else None."""
    nn = torch.nn
    if not isinstance(m, nn.Module) or isinstance(m, HubertLayerHIP) or m.training:  # (eval mode: every dropout is the identity)
        return None
    got = _layer_parts(m)
    if got is None:
        return None
    conv, parts, act, att = got
    lin = [parts[n] for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "fc1", "fc2")]
    lns = [parts["self_attn_layer_norm"], parts["final_layer_norm"]]
    if not all(isinstance(l, nn.Linear) and l.bias is not None for l in lin) or not all(isinstance(l, nn.LayerNorm) for l in lns):
        return None
    d, ffn, heads = lin[0].in_features, lin[4].out_features, getattr(att, "num_heads", None)
    if any((l.in_features, l.out_features) != (d, d) for l in lin[:4]) or (lin[4].in_features, lin[5].in_features, lin[5].out_features) != (d, ffn, d):
        return None
    if any(tuple(l.normalized_shape) != (d,) or l.weight is None or l.bias is None for l in lns) or lns[0].eps != lns[1].eps:
        return None
    if not isinstance(heads, int) or heads * HEAD_DIM != d or d % 64 or d > 1024 or ffn % 64 or ffn > 4096 or not _exact_gelu(act):
        return None
    ps = list(m.parameters())
    if len(ps) != len(_LAYER_TENSORS) or len({p.device for p in ps}) != 1 or ps[0].device.type != "cuda" or len({p.dtype for p in ps}) != 1:
        return None  # (a further parameter -- a relative-position table, say -- is a layer the kernels do not compute)
    if conv == "fairseq":
        if getattr(m, "layer_norm_first", None) is not False:
            return None
    else:
        # transformers' pre-norm layer has the same attribute names: compare the module with the post-norm formula on its own submodules
        try:
            with torch.no_grad():
                x = torch.linspace(-1.0, 1.0, 3 * d, device=ps[0].device, dtype=torch.float32).view(1, 3, d).to(ps[0].dtype).sin()
                h = parts["self_attn_layer_norm"](x + att(x, attention_mask=None, output_attentions=False)[0])
                want = parts["final_layer_norm"](h + m.feed_forward(h))
                ok = bool((m(x)[0].float() - want.float()).abs().max() <= 1e-3 * (1.0 + want.float().abs().max()))
        except Exception:  # noqa  (not a layer of this shape)
            return None
        if not ok:
            return None
    return dict(convention=conv, d=int(d), heads=int(heads), ffn=int(ffn), eps=float(lns[0].eps), device=ps[0].device)


def supported_layer(m) -> bool:
    """Whether ``m`` has the STRUCTURE of the layer the kernels serve (never its class name): either convention's attribute names
    (``self_attn.{q,k,v,out}_proj``, ``self_attn_layer_norm``, ``fc1``, ``fc2``, ``final_layer_norm``; or ``attention.*``, ``layer_norm``,
    ``feed_forward.intermediate_dense / output_dense``, ``final_layer_norm``), post-norm, the exact GELU, eval mode (no dropout effect), biases
    everywhere, head dim 64, ``d <= 1024`` and ``ffn <= 4096`` in multiples of 64, and no further parameter, all on one GPU."""
    return _layer_cfg(m) is not None


def layer_state_dict(m) -> Dict[str, torch.Tensor]:
    """The sixteen tensors of a layer under fairseq's names (``_LAYER_TENSORS``), whichever convention ``m`` follows."""
    got = _layer_parts(m)
    if got is None:
        raise _lib.RvcmiError("layer_state_dict: not a transformer layer of either convention", code=_lib.ERR_INVALID)
    return {"%s.%s" % (n, p): getattr(mod, p) for n, mod in got[1].items() for p in ("weight", "bias")}


class HubertEncoderHIP:
    """Some or all layers of a post-norm HuBERT transformer on the HIP kernels.  ``forward(x[B, T, d])`` -> the same shape and dtype (fp16 or
    fp32), every layer's output rounded once to that dtype, so ``forward(first=0, n=2)`` is bit-equal to two calls of one layer."""

    def __init__(self, state_dicts, cfg, device):
        dev = _lib.cuda_device(device, "HubertEncoderHIP")
        arr = _lib.pack_tensors(("layers.%d.%s" % (i, k), v.detach().float().cpu().contiguous()) for i, sd in enumerate(state_dicts) for k, v in sd.items()
                                if torch.is_tensor(v) and v.is_floating_point() and 1 <= v.dim() <= 4)
        if not len(arr):
            raise _lib.RvcmiError("HubertEncoderHIP: no layer weights", code=_lib.ERR_INVALID)
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rvcmi_hubert_enc_create(arr, len(arr), len(state_dicts), int(cfg["d"]), int(cfg["heads"]), int(cfg["ffn"]),
                                                          float(cfg.get("eps", 1e-5)), dev.index, C.byref(h)))
        self._h = _lib.Handle("rvcmi_hubert_enc_destroy", h)
        self._device = dev
        self.n_layers, self.d = len(state_dicts), int(cfg["d"])
        self._ws = None
        self._retired = []  # earlier, smaller workspaces: a captured graph may still point at one

    @classmethod
    def from_state_dicts(cls, state_dicts, cfg, device) -> "HubertEncoderHIP":
        """``state_dicts``: one dict per layer under fairseq's names (``layer_state_dict``); ``cfg``: ``d``, ``heads``, ``ffn``, ``eps``."""
        return cls(list(state_dicts), cfg, device)

    @classmethod
    def from_layers(cls, modules, device=None) -> "HubertEncoderHIP":
        """From torch layer modules on a GPU, fairseq's or transformers' (each recognised by ``supported_layer``, all of one geometry)."""
        cfgs = [_layer_cfg(m) for m in modules]
        if not cfgs or any(c is None for c in cfgs):
            raise _lib.RvcmiError("HubertEncoderHIP: not the layers the kernels serve (post-norm, exact GELU, head dim 64, eval mode, on a GPU)",
                                  code=_lib.ERR_INVALID)
        key = lambda c: (c["d"], c["heads"], c["ffn"], c["eps"], c["device"])
        if len({key(c) for c in cfgs}) != 1:
            raise _lib.RvcmiError("HubertEncoderHIP: the layers differ in geometry or device", code=_lib.ERR_INVALID)
        return cls([layer_state_dict(m) for m in modules], cfgs[0], cfgs[0]["device"] if device is None else device)

    def workspace_bytes(self, B: int, T: int) -> int:
        return int(_lib.lib().rvcmi_hubert_enc_workspace_bytes(self._h, int(B), int(T)))

    def _own_workspace(self, need: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.RvcmiError("HubertEncoderHIP: the first call of a larger shape allocates its workspace and must not be inside a stream "
                                      "capture; call once before the capture or pass workspace=")
            if self._ws is not None:
                self._retired.append(self._ws)
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self._device)
        return self._ws

    def forward(self, x: torch.Tensor, key_mask: Optional[torch.Tensor] = None, first: int = 0, n: Optional[int] = None,
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Layers ``first .. first + n - 1`` (default: all from ``first``).  ``key_mask``: bool / uint8 ``[B, T]`` on the GPU, nonzero = a padded
        key no query attends to (padded QUERY rows are computed like any other, as torch does).  ``workspace``: a uint8 tensor of
        ``workspace_bytes(B, T)`` bytes; default: the object's own, which grows on the first call of a larger shape (not inside a capture)."""
        _lib.require_on(x, self._device, "HubertEncoderHIP")
        if x.dim() != 3 or x.dtype not in (torch.float16, torch.float32) or int(x.shape[2]) != self.d:
            raise _lib.RvcmiError("HubertEncoderHIP: expected an fp16 or fp32 [B, T, %d], got %s %s" % (self.d, x.dtype, tuple(x.shape)), code=_lib.ERR_INVALID)
        B, T = int(x.shape[0]), int(x.shape[1])
        n = self.n_layers - int(first) if n is None else int(n)
        x = x.detach().contiguous()
        km = None
        if key_mask is not None:
            if key_mask.device != x.device or tuple(key_mask.shape) != (B, T):
                raise _lib.RvcmiError("HubertEncoderHIP: the key mask must be [B, T] = %s on %s" % ((B, T), x.device), code=_lib.ERR_INVALID)
            key_mask = (key_mask if key_mask.dtype in (torch.uint8, torch.bool) else key_mask != 0).contiguous()
            key_mask = key_mask.view(torch.uint8) if key_mask.dtype == torch.bool else key_mask
            km = key_mask
        need = self.workspace_bytes(B, T)
        ws = _lib.ptr(self._own_workspace(need)) if workspace is None else _lib.workspace_ptr(workspace, need, x.device, "HubertEncoderHIP")
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().rvcmi_hubert_enc_forward(self._h, int(first), n, B, T, _lib.ptr(x), 1 if x.dtype == torch.float16 else 0, _lib.ptr(km),
                                                           _lib.ptr(out), ws, _lib.stream_ptr(x.device)))
        return out

    __call__ = forward


class HubertLayerHIP(torch.nn.Module):
    """The drop-in for ONE layer: layer ``index`` of ``encoder``, answering in the convention of the module it replaced (``_original``, kept
    unregistered).  fairseq: ``layer(x[T, B, C], self_attn_mask=None, self_attn_padding_mask=None, need_weights=False, att_args=None) ->
    (x, (None, None))``.  transformers: ``layer(hidden_states[B, T, C], attention_mask=None, output_attentions=False) -> (hidden_states,)``.
    What the kernels do not compute -- an attention mask over (query, key) pairs, attention weights -- goes to the original module."""

    def __init__(self, encoder: HubertEncoderHIP, index: int, convention: str):
        super().__init__()
        if convention not in ("fairseq", "transformers"):
            raise ValueError("convention: 'fairseq' or 'transformers'")
        object.__setattr__(self, "encoder", encoder)
        self.index = int(index)
        self.convention = convention

    def forward(self, *args, **kw):
        return self._fairseq(*args, **kw) if self.convention == "fairseq" else self._transformers(*args, **kw)

    def _fairseq(self, x, self_attn_mask=None, self_attn_padding_mask=None, need_weights=False, att_args=None):
        if self_attn_mask is not None or need_weights:
            return self.__dict__["_original"](x, self_attn_mask=self_attn_mask, self_attn_padding_mask=self_attn_padding_mask, need_weights=need_weights,
                                              att_args=att_args)
        y = self.encoder.forward(x.transpose(0, 1), self_attn_padding_mask, first=self.index, n=1)
        return y.transpose(0, 1), (None, None)

    def _transformers(self, hidden_states, attention_mask=None, output_attentions=False, **kw):
        if output_attentions or kw:
            return self.__dict__["_original"](hidden_states, attention_mask=attention_mask, output_attentions=output_attentions, **kw)
        km = None
        if attention_mask is not None:  # [B, 1, 1 or T, T]: additive (negative = masked) or boolean (True = attend); a device op, no sync
            row = attention_mask[:, 0, 0, :]
            km = ~row if row.dtype == torch.bool else row < 0
        return (self.encoder.forward(hidden_states, km, first=self.index, n=1),)


def _layer_lists(model):
    """The ``ModuleList``s of transformer layers: ``model.encoder.layers``, else the same one attribute down (as ``_holders`` looks)."""
    def of(m):
        layers = getattr(getattr(m, "encoder", None), "layers", None)
        return layers if isinstance(layers, torch.nn.ModuleList) and len(layers) else None
    if of(model) is not None:
        return [of(model)]
    subs = list(model.children()) if isinstance(model, torch.nn.Module) else []
    subs += [v for v in getattr(model, "__dict__", {}).values() if isinstance(v, torch.nn.Module)]
    out = []
    for m in subs:
        if of(m) is not None and not any(of(m) is o for o in out):
            out.append(of(m))
    return out


def accelerate_hubert_layers(model) -> int:
    """Replace every layer of ``model.encoder.layers`` (or of the module one attribute down) by a ``HubertLayerHIP`` on ONE ``HubertEncoderHIP``
    with the same weights, in place.  ALL OR NONE: if any layer is not ``supported_layer`` (or they differ in geometry), nothing is modified
    and 0 is returned.  -> the number of layers swapped.  The originals stay on the HIP modules (unregistered) for ``restore_hubert_layers``."""
    n = 0
    for layers in _layer_lists(model):
        mods = list(layers)
        try:
            enc = HubertEncoderHIP.from_layers(mods)
        except _lib.RvcmiError as e:
            if e.code == _lib.ERR_INVALID:  # layers the kernels do not serve: torch's modules stay
                continue
            raise
        for i, m in enumerate(mods):
            hip = HubertLayerHIP(enc, i, _layer_parts(m)[0])
            hip.eval()
            object.__setattr__(hip, "_original", m)  # (not registered: its weights must not appear twice in state_dict())
            layers[i] = hip
            n += 1
    return n


def restore_hubert_layers(model) -> int:
    """Undo ``accelerate_hubert_layers``.  -> the number of torch modules put back."""
    n = 0
    for layers in _layer_lists(model):
        for i, m in enumerate(list(layers)):
            orig = m.__dict__.get("_original") if isinstance(m, HubertLayerHIP) else None
            if orig is not None:
                layers[i] = orig
                n += 1
    getattr(model, "__dict__", {}).pop("_rvcmi_hubert_enc", None)
    return n


def accelerate_hubert_layers_once(model) -> int:
    """What the conversion paths call next to ``accelerate_hubert_once``: with the switch on, ``accelerate_hubert_layers(model)`` once per
    model object (the count is remembered on it as ``_rvcmi_hubert_enc``); with it off, nothing."""
    return _lib.once(model, "_rvcmi_hubert_enc", lambda: accelerate_hubert_layers(model)) if hubert_enc_on() else 0
