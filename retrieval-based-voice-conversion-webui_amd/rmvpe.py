"""The whole RMVPE f0 estimator (rvc/f0/rmvpe.py) on this project's kernels -- like ``gru.py`` and ``unet.py`` BEYOND the scope table
(SURVEY.md section 8), and the piece that closes the chain: the log-mel front end and the ``Linear`` + sigmoid head of ``csrc/rmvpe.hip``
around ``UNetHIP`` and ``GRUHIP``, decoded by ``glue.rmvpe_f0``.

    hip = rvc_amd.RMVPEHIP.from_reference(rmvpe)     # an rvc.f0.rmvpe.RMVPE-like object; None when it is not one the kernels serve
    pitch, pitchf = hip.f0(wav16k, p_len, f0_up_key) # what Generator.calculate(..., "rmvpe") + post_process return, on the device
    pairs = hip.f0_batch(wavs, p_lens, f0_up_key)    # the same for waveforms of ANY lengths in one pass (a ragged batch): one (pitch, pitchf) each

Between the input cast ``wav.float()`` and the result torch allocates buffers and makes the one fp32 -> fp16 cast in front of the GRU;
everything else is enqueue-only HIP, so the chain captures into a hipGraph once its first call of a size has happened eagerly.

Opt-in (``RVCMI_RMVPE_HIP=1`` or ``rvc_amd.install(rmvpe_hip=True)``; default off): with the switch on, ``pipeline._rmvpe_on_device`` runs
this object instead of the reference's ``mel_extractor`` + ``_mel2hidden``, and the realtime entry keeps a fractional key (formant slider)
on the device.  The reference object is read, never changed.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from . import glue
from . import unet as _unet
from .gru import GRUHIP
from .gru import supports as _gru_supports

N_MELS, N_FFT, N_CLASS = 128, 1024, 360
CACHE_ROWS = 512   # workspaces of calls with B * T_pad <= this stay with the object (the realtime windows: a captured graph points at them, so
                   # they are never dropped); longer inputs take theirs from torch's caching allocator per call
RMVPE_HIP = False  # install(rmvpe_hip=True) sets it; RVCMI_RMVPE_HIP=1 / =0 overrides it per call


RMVPE_BATCH = False        # the group path of pipeline.convert_files (ONE f0_batch call per group); RVCMI_RMVPE_BATCH=1 / =0 overrides it per call.
                           # Off until tools/rmvpe_batch_time.py has been run: profiles/rmvpe_batch_time.json decides the default and the threshold
RMVPE_BATCH_MIN_FILES = 2  # ... and with it on, a group takes that path from this many files to estimate


_HIP = _lib.Switch("RVCMI_RMVPE_HIP", globals(), "RMVPE_HIP")
rmvpe_on, rmvpe_batch_on = _HIP.on, _lib.Switch("RVCMI_RMVPE_BATCH", globals(), "RMVPE_BATCH", base=_HIP).on


def ragged_layout(frames: Sequence[int]) -> Tuple[List[int], int]:
    """Frame counts ``T_i`` of a ragged batch -> (row offsets, R): every sequence padded to ``Tp_i = 32 * ceil(T_i / 32)`` as the reference pads a
    single one (rvc/f0/rmvpe.py:141-144) and PACKED along the frame axis -- sequence i owns rows ``[offsets[i], offsets[i] + Tp_i)``,
    ``R = offsets[-1] = sum(Tp_i)``; no row is spent on padding to the longest."""
    frames = [int(t) for t in frames]
    if not frames:
        raise _lib.RvcmiError("RMVPEHIP: an empty batch", code=_lib.ERR_INVALID)
    off = [0]
    for t in frames:
        if t < 1:
            raise _lib.RvcmiError("RMVPEHIP: a sequence of %d frames" % t, code=_lib.ERR_INVALID)
        off.append(off[-1] + 32 * ((t - 1) // 32 + 1))
    if off[-1] > 1 << 22:
        raise _lib.RvcmiError("RMVPEHIP: %d packed frames in one batch (at most 2^22)" % off[-1], code=_lib.ERR_INVALID)
    return off, off[-1]


def _network_parts(model):
    """-> (UNetHIP or state dict, GRUHIP or nn.GRU, nn.Linear, device) of an ``E2E``-like network (rvc/f0/e2e.py: U-Net, 3-channel head, one
    bidirectional GRU, Linear(512, 360), sigmoid), recognised by its state-dict keys and module types; None for anything else."""
    if not isinstance(model, torch.nn.Module) or isinstance(model, torch.jit.ScriptModule):
        return None
    named = list(model.named_modules())
    grus = [(n, m) for n, m in named if isinstance(m, (torch.nn.GRU, GRUHIP))]
    lins = [(n, m) for n, m in named if isinstance(m, torch.nn.Linear)]
    if len(grus) != 1 or len(lins) != 1:
        return None
    (gname, gru), (lname, lin) = grus[0], lins[0]
    if isinstance(gru, torch.nn.GRU) and not _gru_supports(gru):
        return None
    if gru.input_size != 3 * N_MELS or (lin.in_features, lin.out_features) != (2 * gru.hidden_size, N_CLASS) or lin.bias is None:
        return None
    sd = model.state_dict()
    rest = {k for k in sd if not (k.startswith("unet.") or k.startswith("cnn."))}
    want = {lname + ".weight", lname + ".bias"}
    if isinstance(gru, torch.nn.GRU):
        want |= {"%s.%s" % (gname, p) for p, _ in gru.named_parameters()}
    if rest != want:
        return None
    un = getattr(model, "unet", None)
    if isinstance(un, _unet.UNetHIP):  # already swapped by accelerate_rmvpe_unet: the same handle serves
        net = un
        geo = un.geometry
    else:
        geo = _unet.geometry({k: tuple(v.shape) for k, v in sd.items()})
        if geo is None or not isinstance(un, torch.nn.Module) or not _unet._pooling_ok(un):
            return None
        net = sd
    if geo is None or geo["head"] != 3:
        return None
    devs = {v.device for v in sd.values()} | ({gru._device} if isinstance(gru, GRUHIP) else set()) | ({un._device} if isinstance(un, _unet.UNetHIP) else set())
    if len(devs) != 1 or next(iter(devs)).type != "cuda":
        return None
    dev = next(iter(devs))
    return net, gru, lin, torch.device("cuda", _lib.device_index(dev))


class RMVPEHIP:
    """waveform at 16 kHz -> log-mel -> U-Net -> GRU -> salience -> (pitch, pitchf), every stage a HIP kernel of this project."""

    def __init__(self, n_fft: int, hop_length: int, win_length: int, clamp: float, mel_basis: torch.Tensor, is_half: bool, net, gru, linear, device):
        dev = _lib.cuda_device(device, "RMVPEHIP")
        basis = mel_basis.detach().float().cpu().contiguous()
        if basis.dim() != 2 or basis.shape[1] != int(n_fft) // 2 + 1:
            raise _lib.RvcmiError("RMVPEHIP: mel_basis %s does not belong to n_fft %d" % (tuple(basis.shape), n_fft), code=_lib.ERR_INVALID)
        h = C.c_void_p()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().rvcmi_mel_create(int(n_fft), int(hop_length), int(win_length), int(basis.shape[0]), _lib.ptr(basis), float(clamp),
                                                   dev.index, C.byref(h)))
        self._h = _lib.Handle("rvcmi_mel_destroy", h)
        self.device, self.is_half, self.hop_length, self.n_fft = dev, bool(is_half), int(hop_length), int(n_fft)
        self.unet = net if isinstance(net, _unet.UNetHIP) else _unet.UNetHIP(net, dev)
        self.gru = gru if isinstance(gru, GRUHIP) else GRUHIP(gru, dev)
        self._w = linear.weight.detach().to(dev, torch.float32).contiguous().clone()  # uploaded once
        self._b = linear.bias.detach().to(dev, torch.float32).contiguous().clone()
        self._ws = {}

    @classmethod
    def from_reference(cls, rmvpe) -> Optional["RMVPEHIP"]:
        """``rmvpe``: an ``rvc.f0.rmvpe.RMVPE``-like object (``mel_extractor`` with ``n_fft, hop_length, win_length, clamp, mel_basis, is_half``
        and the ``E2E`` network as ``model``).  None -- and nothing touched -- for what the kernels do not serve: another mel or network
        geometry, a CPU model, the onnx session of a ``privateuseone`` device, a TorchScript model."""
        if "privateuseone" in str(getattr(rmvpe, "device", "")):
            return None
        me = getattr(rmvpe, "mel_extractor", None)
        try:
            n_fft, hop, win, clamp = int(me.n_fft), int(me.hop_length), int(me.win_length), float(me.clamp)
            basis, is_half = me.mel_basis, bool(me.is_half)
        except (AttributeError, TypeError, ValueError):
            return None
        if not torch.is_tensor(basis) or tuple(basis.shape) != (N_MELS, N_FFT // 2 + 1) or (n_fft, win) != (N_FFT, N_FFT) or hop < 1:
            return None
        parts = _network_parts(getattr(rmvpe, "model", None))
        if parts is None:
            return None
        net, gru, lin, dev = parts
        try:
            return cls(n_fft, hop, win, clamp, basis, is_half, net, gru, lin, dev)
        except _lib.RvcmiError as e:
            if e.code == _lib.ERR_INVALID:  # a configuration the kernels do not serve: the caller keeps torch
                return None
            raise

    def frames(self, n: int) -> int:
        return int(_lib.lib().rvcmi_mel_frames(self._h, int(n)))

    def _wav(self, wav) -> torch.Tensor:
        _lib.require_on(wav, self.device, "RMVPEHIP")
        x = wav.detach().float()
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2:
            raise _lib.RvcmiError("RMVPEHIP: expected a waveform [n] or [B, n], got %s" % (tuple(wav.shape),), code=_lib.ERR_INVALID)
        return x.contiguous()

    def _buffers(self, B: int, T_pad: int) -> dict:
        ws = self._ws.get((B, T_pad))
        if ws is None:
            nbytes = self.unet.workspace_bytes(B, T_pad)
            if not nbytes:
                msg = _lib.lib().rvcmi_last_error()
                raise _lib.RvcmiError("RMVPEHIP: B = %d, %d frames not served (%s)" % (B, T_pad, msg.decode(errors="replace") if msg else "?"), code=_lib.ERR_INVALID)
            dev, f32 = self.device, torch.float32
            ws = dict(mel=torch.empty(B, T_pad, N_MELS, device=dev, dtype=f32), feat=torch.empty(B, T_pad, 3 * N_MELS, device=dev, dtype=f32),
                      unet=torch.empty(nbytes, device=dev, dtype=torch.uint8), x16=torch.empty(B, T_pad, 3 * N_MELS, device=dev, dtype=torch.float16),
                      y=torch.empty(B, T_pad, 2 * self.gru.hidden_size, device=dev, dtype=f32), sal=torch.empty(B, T_pad, N_CLASS, device=dev, dtype=f32))
            if B * T_pad <= CACHE_ROWS:
                self._ws[(B, T_pad)] = ws
        return ws

    def _mel(self, x: torch.Tensor, ws=None) -> Tuple[torch.Tensor, int]:
        B, n = int(x.shape[0]), int(x.shape[1])
        T = self.frames(n)
        if T < 1:
            raise _lib.RvcmiError("RMVPEHIP: a %d-sample input is not longer than the reflection pad %d" % (n, self.n_fft // 2), code=_lib.ERR_INVALID)
        T_pad = 32 * ((T - 1) // 32 + 1)
        ws = ws if ws is not None else self._buffers(B, T_pad)
        _lib.check(_lib.lib().rvcmi_mel_forward(self._h, B, n, _lib.ptr(x), 1 if self.is_half else 0, T_pad, _lib.ptr(ws["mel"]), _lib.stream_ptr(self.device)))
        return ws, T

    def _salience(self, x: torch.Tensor) -> Tuple[torch.Tensor, int]:
        """-> ([B, T_pad, 360] fp32, T).  Up to ``CACHE_ROWS`` rows the tensor belongs to the object: the next call of the same shape overwrites it."""
        L = _lib.lib()
        with torch.cuda.device(self.device):
            ws, T = self._mel(x)
            B, T_pad = int(ws["mel"].shape[0]), int(ws["mel"].shape[1])
            st = _lib.stream_ptr(self.device)
            _lib.check(L.rvcmi_unet_forward(self.unet._h, B, T_pad, _lib.ptr(ws["mel"]), _lib.ptr(ws["feat"]), _lib.ptr(ws["unet"]), st))
            ws["x16"].copy_(ws["feat"])  # the fp32 -> fp16 cast GRUHIP.forward makes
            _lib.check(L.rvcmi_gru_forward(self.gru._h, B, T_pad, _lib.ptr(ws["x16"]), _lib.ptr(ws["y"]), None, st))
            _lib.check(L.rvcmi_rmvpe_head(_lib.ptr(ws["y"]), B * T_pad, _lib.ptr(self._w), _lib.ptr(self._b), 1 if self.is_half else 0, _lib.ptr(ws["sal"]), st))
        return ws["sal"], T

    def mel(self, wav: torch.Tensor) -> torch.Tensor:
        """[n] or [B, n] -> log-mel [B, T_pad, 128] fp32, T_pad = T rounded up to 32, frames T .. T_pad - 1 zero: the U-Net's input."""
        x = self._wav(wav)
        with torch.cuda.device(self.device):
            return self._mel(x)[0]["mel"].clone()

    def salience(self, wav: torch.Tensor) -> torch.Tensor:
        """[n] or [1, n] -> salience [T, 360] fp32 (``RMVPE._mel2hidden`` of the mel spectrogram, squeezed); [B, n] -> [B, T, 360]."""
        x = self._wav(wav)
        sal, T = self._salience(x)
        return sal[0, :T].clone() if x.shape[0] == 1 else sal[:, :T].clone()

    def _wavs(self, wavs) -> List[torch.Tensor]:
        """The members of a ragged batch, each checked as ``_wav`` checks a lone input and BEFORE anything is enqueued."""
        if isinstance(wavs, torch.Tensor) or not isinstance(wavs, (list, tuple)):
            raise _lib.RvcmiError("RMVPEHIP: a batch is a list of 1-D waveforms (got %s)" % type(wavs).__name__, code=_lib.ERR_INVALID)
        if len(wavs) == 0:
            raise _lib.RvcmiError("RMVPEHIP: an empty batch", code=_lib.ERR_INVALID)
        xs = []
        for w in wavs:
            if torch.is_tensor(w) and w.dim() != 1:
                raise _lib.RvcmiError("RMVPEHIP: a batch member must be a 1-D waveform, got %s" % (tuple(w.shape),), code=_lib.ERR_INVALID)
            x = self._wav(w)
            if x.shape[1] <= self.n_fft // 2:
                raise _lib.RvcmiError("RMVPEHIP: a %d-sample input is not longer than the reflection pad %d" % (x.shape[1], self.n_fft // 2), code=_lib.ERR_INVALID)
            xs.append(x)
        return xs

    def _salience_ragged(self, xs: List[torch.Tensor], mark=None) -> Tuple[torch.Tensor, List[int], List[int]]:
        """-> (packed salience [R, 360] fp32, row offsets, frame counts).  Mel of every sequence into its own rows (its own reflection pad,
        its own zero pad frames): ONE batched launch when all sequences have the same sample count -- one sequence included, so that a bank
        of one session issues the launches a larger bank issues -- else one launch per sequence; then ONE ragged U-Net, ONE ragged GRU and ONE head launch over the R packed rows.  ``mark(stage)``: called after each
        stage has been enqueued (tools/rmvpe_batch_time.py puts a synchronising clock there)."""
        mark = mark or (lambda stage: None)
        L = _lib.lib()
        frames = [self.frames(int(x.shape[1])) for x in xs]
        off, R = ragged_layout(frames)
        nseq = len(xs)
        off_host = (C.c_int * (nseq + 1))(*off)
        with torch.cuda.device(self.device):
            nbytes = L.rvcmi_unet_workspace_bytes_ragged(self.unet._h, nseq, off_host)
            if not nbytes:
                msg = L.rvcmi_last_error()
                raise _lib.RvcmiError("RMVPEHIP: a batch of %d sequences, %d frames not served (%s)" % (nseq, R, msg.decode(errors="replace") if msg else "?"),
                                      code=_lib.ERR_INVALID)
            dev, f32 = self.device, torch.float32
            off_dev = torch.tensor(off, dtype=torch.int32, device=dev)
            mel = torch.empty(R, N_MELS, device=dev, dtype=f32)
            feat = torch.empty(R, 3 * N_MELS, device=dev, dtype=f32)
            ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
            y = torch.empty(R, 2 * self.gru.hidden_size, device=dev, dtype=f32)
            sal = torch.empty(R, N_CLASS, device=dev, dtype=f32)
            st, half = _lib.stream_ptr(self.device), 1 if self.is_half else 0
            if len({int(x.shape[1]) for x in xs}) == 1:
                # equal lengths (a bank's f0 windows): every sequence has the same T_pad, so the packed rows ARE the dense
                # [B, T_pad, 128] layout of one batched call (k_rmvpe_logmel writes out[b][t][m] and tiles the frames per b from 0).
                # The stacked copy is a temporary: freeing it when this statement ends is safe only because `st` is torch's current
                # stream, the one its caching allocator orders the block's reuse on.
                _lib.check(L.rvcmi_mel_forward(self._h, nseq, int(xs[0].shape[1]), _lib.ptr(torch.cat(xs)), half, off[1] - off[0], _lib.ptr(mel), st))
            else:
                for i, x in enumerate(xs):
                    _lib.check(L.rvcmi_mel_forward(self._h, 1, int(x.shape[1]), _lib.ptr(x), half, off[i + 1] - off[i],
                                                   C.c_void_p(mel.data_ptr() + 4 * N_MELS * off[i]), st))
            mark("mel")
            _lib.check(L.rvcmi_unet_forward_ragged(self.unet._h, nseq, off_host, _lib.ptr(off_dev), _lib.ptr(mel), _lib.ptr(feat), _lib.ptr(ws), st))
            mark("unet")
            x16 = feat.half()  # the fp32 -> fp16 cast GRUHIP.forward makes
            _lib.check(L.rvcmi_gru_forward_ragged(self.gru._h, nseq, off_host, _lib.ptr(off_dev), _lib.ptr(x16), _lib.ptr(y), None, st))
            mark("gru")
            _lib.check(L.rvcmi_rmvpe_head(_lib.ptr(y), R, _lib.ptr(self._w), _lib.ptr(self._b), half, _lib.ptr(sal), st))
            mark("head")
        return sal, off, frames

    def salience_batch(self, wavs) -> List[torch.Tensor]:
        """A list of 1-D waveforms of ANY lengths -> their saliences ``[T_i, 360]`` fp32 from ONE pass over the packed batch; each is what
        ``salience`` of that waveform alone returns, to the summation order of the U-Net layers that split their K loop by launch size.
        The results are VIEWS of one packed tensor that belongs to this call alone (no copy per sequence: the launch count does not depend
        on the number of waveforms); ``.clone()`` one to keep it without the rest of the batch, or before writing into it."""
        sal, off, frames = self._salience_ragged(self._wavs(wavs))
        return [sal[o: o + t] for o, t in zip(off, frames)]   # views of the call's own packed tensor: no copy per sequence

    def f0_batch(self, wavs, p_lens, f0_up_key=0, thred: float = 0.03) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """-> per waveform (pitch int64 [1, p_len_i], pitchf float32 [1, p_len_i]): ``glue.rmvpe_f0`` of its rows of ``salience_batch``, for
        all waveforms in ONE ``glue.rmvpe_f0_ragged`` call on the packed salience (two launches).  ``f0_up_key``: one key, or one per waveform."""
        xs = self._wavs(wavs)
        if not isinstance(p_lens, (list, tuple)) or len(p_lens) != len(xs) or any(int(p) < 1 for p in p_lens):
            raise _lib.RvcmiError("RMVPEHIP.f0_batch: one positive p_len per waveform", code=_lib.ERR_INVALID)
        keys = list(f0_up_key) if isinstance(f0_up_key, (list, tuple)) else [f0_up_key] * len(xs)
        if len(keys) != len(xs):
            raise _lib.RvcmiError("RMVPEHIP.f0_batch: one key, or one per waveform (%d keys for %d waveforms)" % (len(keys), len(xs)), code=_lib.ERR_INVALID)
        sal, off, frames = self._salience_ragged(xs)
        return glue.rmvpe_f0_ragged(sal, [(o, t, int(p), k) for o, t, p, k in zip(off, frames, p_lens, keys)], thred)

    def f0(self, wav: torch.Tensor, p_len: int, f0_up_key=0, thred: float = 0.03) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (pitch int64 [1, p_len], pitchf float32 [1, p_len]) as ``glue.rmvpe_f0`` returns them; ``f0_up_key`` may be fractional."""
        x = self._wav(wav)
        if x.shape[0] != 1:
            raise _lib.RvcmiError("RMVPEHIP.f0: one waveform at a time (the decode is per sequence)", code=_lib.ERR_INVALID)
        sal, T = self._salience(x)
        return glue.rmvpe_f0(sal[0, :T], p_len, f0_up_key, thred)


def for_generator(gen, rmvpe) -> Optional[RMVPEHIP]:
    """The ``RMVPEHIP`` of ``rmvpe``, built once and remembered on the f0 generator that owns it (not on the reference object); None when the
    kernels do not serve it."""
    got = getattr(gen, "_rvcmi_rmvpe_hip", None)
    if got is None or got[0] is not rmvpe:
        got = (rmvpe, RMVPEHIP.from_reference(rmvpe))
        try:
            gen._rvcmi_rmvpe_hip = got
        except Exception:  # noqa  (an object without a __dict__: built again next time)
            pass
    return got[1]
