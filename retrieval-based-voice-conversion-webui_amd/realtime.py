"""Host-side mirror of the realtime caller ``infer/lib/rtrvc.py`` ``RVC.infer`` for everything after HuBERT and the f0
extractor (rtrvc.py:163-251): retrieval on the new frames only, pitch caches, x2 + protect, ``net_g.infer`` with
``skip_head / return_length / return_length2``.  All tensors live on the GPU; the compute runs in the HIP library
(``IVFFlatHIP``, ``glue``, the accelerated ``net_g``), this class only keeps the rolling state the reference keeps.

    rt = RealtimeVC(net_g, index=rvc_amd.read_index(path), index_rate=0.75, device="cuda:0")
    wav = rt.infer(hubert_feats, n_input_samples, block_frame_16k, skip_head, return_length, pitch=p, pitchf=pf)

HuBERT and the f0 estimators stay PyTorch, as in the reference; the optional formant resample
(``torchaudio.transforms.Resample``, rtrvc.py:249-259) is ``SincResample`` below: the same windowed-sinc polyphase filter on a
HIP kernel (torchaudio is not installable offline: its published formula is restated, parity unpinned).
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib, glue
from .gate import TorchGateBank, TorchGateHIP


def f0_extractor_frame(block_frame_16k: int, method: str = "fcpe", window: int = 160) -> int:
    """Samples of the rolling input the f0 estimator sees per block (rtrvc.py:203-207)."""
    n = int(block_frame_16k) + 800
    if method == "rmvpe":
        n = 5120 * ((n - 1) // 5120 + 1) - window
    return n


def sinc_resample_kernel(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """The filter bank of ``torchaudio.transforms.Resample(orig_freq, new_freq, dtype=torch.float32)`` (its defaults:
    ``sinc_interp_hann``, ``lowpass_filter_width`` 6, ``rolloff`` 0.99), restated from torchaudio's published
    ``functional._get_sinc_resample_kernel``: frequencies reduced by their gcd, ``base = min(orig, new) * rolloff``,
    ``width = ceil(lpw * orig / base)``, taps ``t = (-k/new + i/orig) * base`` for ``i`` in ``[-width, width + orig)`` clamped to
    ``+-lpw``, hann window ``cos(t * pi / lpw / 2)^2``, ``sinc(t * pi) * window * base / orig``; evaluated in float32 like
    torchaudio does for ``dtype=float32``.  -> (kernel [new, 2*width + orig] float32 CPU tensor, width, orig, new)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    of, nf = int(orig_freq) // g, int(new_freq) // g
    base = min(of, nf) * rolloff
    width = int(math.ceil(lowpass_filter_width * of / base))
    idx = torch.arange(-width, width + of, dtype=torch.float32)[None, :] / of
    t = torch.arange(0, -nf, -1, dtype=torch.float32)[:, None] / nf + idx
    t = t * base
    t = t.clamp(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    kern = torch.where(t == 0, torch.ones_like(t), t.sin() / t) * window * (base / of)
    return kern.contiguous(), width, of, nf


class SincResample:
    """``torchaudio.transforms.Resample(orig_freq, new_freq, dtype=torch.float32).to(device)`` as the realtime path uses it
    (rtrvc.py:251-259): call with a [1, n] or [n] float32 CUDA tensor, get ``ceil(new * n / orig)`` samples back."""

    def __init__(self, orig_freq: int, new_freq: int, device):
        k, self.width, self.orig, self.new = sinc_resample_kernel(orig_freq, new_freq)
        self.device = torch.device(device)
        self.kernel = k.to(self.device)

    def __call__(self, wav: torch.Tensor) -> torch.Tensor:
        if wav.device.type != "cuda":
            raise _lib.RvcmiError("SincResample input must live on the GPU (no CPU fallback)")
        shape = wav.shape
        x = wav.reshape(-1, shape[-1]).to(torch.float32).contiguous()
        if self.orig == self.new:
            return wav
        n = int(x.shape[1])
        n_out = -(-self.new * n // self.orig)
        out = torch.empty(x.shape[0], n_out, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            st = _lib.stream_ptr(x.device)
            for r in range(x.shape[0]):
                _lib.check(_lib.lib().rvcmi_glue_resample_poly(_lib.ptr(x[r]), n, _lib.ptr(self.kernel), self.orig, self.new, int(self.kernel.shape[1]),
                                                               self.width, _lib.ptr(out[r]), n_out, st))
        return out.reshape(shape[:-1] + (n_out,))

    def batch(self, wav: torch.Tensor) -> torch.Tensor:
        """``wav`` [S, n] float32 whose rows may be views into longer buffers -> [S, ceil(new * n / orig)]: ONE launch for all
        rows (``__call__`` issues one per row), each row bit-equal to ``__call__`` on it."""
        if wav.device.type != "cuda":
            raise _lib.RvcmiError("SincResample input must live on the GPU (no CPU fallback)")
        S, n, stride = glue.bank_rows(wav, "wav")
        if self.orig == self.new:
            return wav
        n_out = -(-self.new * n // self.orig)
        out = torch.empty(S, n_out, device=wav.device, dtype=torch.float32)
        with torch.cuda.device(wav.device):
            _lib.check(_lib.lib().rvcmi_glue_resample_poly_batch(S, _lib.ptr(wav), stride, n, _lib.ptr(self.kernel), self.orig, self.new,
                                                                 int(self.kernel.shape[1]), self.width, _lib.ptr(out), n_out, n_out,
                                                                 _lib.stream_ptr(wav.device)))
        return out


def formant_geometry(shift: float, return_length: int, tgt_sr: int):
    """What a formant shift of ``shift`` semitones makes of a realtime block (rtrvc.py:190-191, 248; no device needed) ->
    ``(factor, return_length2, upp_res)``: the generator decodes ``return_length2`` frames instead of ``return_length``, and their first
    ``return_length * upp_res`` samples are resampled from ``upp_res`` to ``tgt_sr // 100`` samples per frame (not at all when the two
    are equal).  The reference's own expressions, so that every caller rounds as it does."""
    factor = pow(2, shift / 12)                                                           # :190
    return_length2 = int(np.ceil(return_length * factor))                                 # :191
    upp_res = int(np.floor(factor * tgt_sr // 100))                                       # :248
    return factor, return_length2, upp_res


class SincResampleRagged:
    """``SincResample(orig_s, new_freq)`` for ``S`` rows with a rate ``orig_s`` of their own, in ONE launch
    (``rvcmi_glue_resample_poly_ragged``): row ``s`` of ``wav`` [S, >= frames * orig_s] -> row ``s`` of [S, frames * new_freq], bit-equal
    to ``SincResample(orig_s, new_freq)`` on its first ``frames * orig_s`` samples; a row with ``orig_s == new_freq`` is the first
    ``frames * new_freq`` samples of its input.  The bank's formant shift per session (rtrvc.py:248-259): ``orig_s`` is the session's
    ``upp_res``.

    The filter tables (``sinc_resample_kernel``) are kept per distinct ``orig``; the concatenated device buffer and the per-row descriptors
    are rebuilt only when the tuple of the rows' rates (or ``frames``) changes -- nothing is uploaded per block.  ``plan`` is the host part
    and needs no device."""

    def __init__(self, new_freq: int, device=None):
        self.new_freq = int(new_freq)
        self.device = None if device is None else torch.device(device)
        self._tables = {}     # orig -> (kernel [nf, K] CPU, width, of, nf)
        self.key = None       # (the rows' rates, frames) of the current plan
        self.rows = []        # per row: dict(w_off, n, orig, new, K, width), the fields of rvcmi_resample_row
        self.offsets = {}     # orig -> first float of its table in the concatenated buffer
        self.table_floats = 0
        self.rebuilds = 0
        self._dev = None      # (tables, descriptors) on the device

    def plan(self, origs, frames: int) -> bool:
        """Lay out the tables and descriptors for rows of rates ``origs`` and ``frames`` frames each; -> whether anything changed."""
        key = (tuple(int(o) for o in origs), int(frames))
        if key == self.key:
            return False
        if not key[0] or min(key[0]) < 1 or key[1] < 1:
            raise ValueError("SincResampleRagged needs at least one row, positive rates and frames >= 1 (got %s)" % (key,))
        self.offsets, self.rows, off = {}, [], 0
        for o in key[0]:
            if o != self.new_freq and o not in self.offsets:   # equal rates share one table; an un-resampled row has none
                if o not in self._tables:
                    self._tables[o] = sinc_resample_kernel(o, self.new_freq)
                k = self._tables[o][0]
                self.offsets[o] = off
                off += int(k.numel())
        self.table_floats = off
        for o in key[0]:
            if o == self.new_freq:
                self.rows.append(dict(w_off=0, n=key[1] * o, orig=1, new=1, K=0, width=0))
            else:
                k, width, of, nf = self._tables[o]
                self.rows.append(dict(w_off=self.offsets[o], n=key[1] * o, orig=of, new=nf, K=int(k.shape[1]), width=width))
        self.key, self._dev = key, None
        self.rebuilds += 1
        return True

    def _upload(self):
        import ctypes as C

        tabs = [self._tables[o][0].reshape(-1) for o in sorted(self.offsets, key=self.offsets.get)]
        table = torch.cat(tabs) if tabs else torch.zeros(1)
        desc = (_lib.ResampleRow * len(self.rows))(*[_lib.ResampleRow(r["w_off"], r["n"], r["orig"], r["new"], r["K"], r["width"]) for r in self.rows])
        raw = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8)
        self._dev = (table.to(self.device), raw.to(self.device), C.sizeof(desc))
        return self._dev

    def __call__(self, wav: torch.Tensor, origs, frames: int) -> torch.Tensor:
        if wav.device.type != "cuda":
            raise _lib.RvcmiError("SincResampleRagged input must live on the GPU (no CPU fallback)")
        if self.device is None:
            self.device = wav.device
        S, n, stride = glue.bank_rows(wav, "wav")
        self.plan(origs, frames)
        if len(self.rows) != S:
            raise ValueError("%d rates for %d rows" % (len(self.rows), S))
        n_max = max(r["n"] for r in self.rows)
        if n_max > n:
            raise ValueError("a row needs %d input samples, wav has %d" % (n_max, n))
        table, desc, _ = self._dev or self._upload()
        n_out = int(frames) * self.new_freq
        out = torch.empty(S, n_out, device=wav.device, dtype=torch.float32)
        with torch.cuda.device(wav.device):
            _lib.check(_lib.lib().rvcmi_glue_resample_poly_ragged(S, _lib.ptr(wav), stride, n_max, _lib.ptr(table), int(table.numel()), _lib.ptr(desc),
                                                                  _lib.ptr(out), n_out, n_out, _lib.stream_ptr(wav.device)))
        return out


class PitchCache:
    """``cache_pitch`` / ``cache_pitchf`` of rtrvc.py:63-66 and their per-block update (rtrvc.py:213-217)."""

    def __init__(self, device, size: int = 1024):
        self.pitch = torch.zeros(size, device=device, dtype=torch.long)
        self.pitchf = torch.zeros(size, device=device, dtype=torch.float32)

    def update(self, pitch: torch.Tensor, pitchf: torch.Tensor, block_frame_16k: int, window: int = 160) -> None:
        """Shift both caches left by one block and write the estimator's new frames (its first three and last one are
        dropped) at the end."""
        shift = int(block_frame_16k) // int(window)
        n = int(pitch.shape[0])
        if n < 5 or n - 4 > self.pitch.numel():
            raise ValueError("pitch block of %d frames does not fit the cache" % n)
        if shift > 0:
            self.pitch[:-shift] = self.pitch[shift:].clone()
            self.pitchf[:-shift] = self.pitchf[shift:].clone()
        self.pitch[4 - n:] = pitch[3:-1].to(self.pitch.device, torch.long)
        self.pitchf[4 - n:] = pitchf[3:-1].to(self.pitchf.device, torch.float32)

    def window(self, p_len: int, return_length: int, return_length2: int):
        """(pitch, pitchf) [1, p_len] handed to ``net_g.infer`` (rtrvc.py:216-219; pitchf follows the formant factor)."""
        return self.pitch[None, -p_len:], self.pitchf[None, -p_len:] * return_length2 / return_length


class RealtimeVC:
    def __init__(self, net_g, index=None, index_rate: float = 0.0, device="cuda:0", if_f0: int = 1, tgt_sr: int = 48000,
                 f0_up_key: float = 0.0, formant_shift: float = 0.0, window: int = 160):
        self.net_g, self.index, self.index_rate = net_g, index, float(index_rate)
        self.device = torch.device(device)
        self.if_f0, self.tgt_sr, self.window = int(if_f0), int(tgt_sr), int(window)
        self.f0_up_key, self.formant_shift = f0_up_key, formant_shift
        self.cache = PitchCache(self.device)
        self._resample = {}
        self._consts = {}

    def _const(self, v: int) -> torch.Tensor:
        t = self._consts.get(v)
        if t is None:
            t = self._consts[v] = torch.tensor([v], dtype=torch.long, device=self.device)
        return t

    # rtrvc.py:122-132
    def set_key(self, new_key):
        self.f0_up_key = new_key

    def set_formant(self, new_formant):
        self.formant_shift = new_formant

    def set_index_rate(self, new_index_rate):
        self.index_rate = float(new_index_rate)

    def infer(self, feats: torch.Tensor, n_input_samples: int, block_frame_16k: int, skip_head: int, return_length: int,
              pitch: Optional[torch.Tensor] = None, pitchf: Optional[torch.Tensor] = None, protect: float = 1.0,
              sid: int = 0) -> torch.Tensor:
        """``feats`` [1, n, d]: the HuBERT output of the whole rolling window (before its last frame is repeated,
        rtrvc.py:163).  ``pitch`` / ``pitchf`` [m]: what the f0 estimator returned for the last
        ``f0_extractor_frame`` samples (``None`` for a model without f0).  Returns the block's waveform [L]."""
        if feats.dim() != 3 or feats.shape[0] != 1:
            raise ValueError("feats must be [1, n, d]")
        feats = torch.cat((feats, feats[:, -1:, :]), 1)                                   # rtrvc.py:163
        p_len = int(n_input_samples) // self.window                                       # :189
        factor = pow(2, self.formant_shift / 12)                                          # :190
        return_length2 = int(math.ceil(return_length * factor))                           # :191
        pf = pitchf if (protect < 0.5 and pitch is not None and pitchf is not None) else None   # :224
        if pf is not None and pf.numel() != p_len:
            # rtrvc.py:221-231 multiplies feats [1, p_len, d] by the RAW estimator output pitchff [m, 1]: torch broadcasting makes
            # that an error unless m == p_len.  Truncating instead would mix frames that are not aligned with the feature rows.
            raise RuntimeError("protect < 0.5 needs pitchf of exactly p_len = %d frames (got %d), as the reference's broadcast at "
                               "infer/lib/rtrvc.py:229 does" % (p_len, pf.numel()))
        cache_pitch = cache_pitchf = None
        if self.if_f0 == 1:
            if pitch is None or pitchf is None:
                raise ValueError("an f0 model needs the block's pitch / pitchf")
            self.cache.update(pitch, pitchf, block_frame_16k, self.window)                # :213-217
            cache_pitch, cache_pitchf = self.cache.window(p_len, return_length, return_length2)
        use_index = self.index is not None and self.index_rate > 0                        # :167
        phone = glue.retrieve_blend_expand(feats, self.index if use_index else None, self.index_rate if use_index else 0.0,
                                           pf, protect if pf is not None else 1.0, p_len, realtime_guard=True,
                                           skip_rows=int(skip_head) // 2)                  # :167-185, 221-233
        lengths, sid_t = self._const(p_len), self._const(int(sid))   # cached: no host-to-device copy per block
        with torch.no_grad():
            audio = self.net_g.infer(phone, lengths, sid_t, pitch=cache_pitch, pitchf=cache_pitchf, skip_head=skip_head,
                                     return_length=return_length, return_length2=return_length2)   # :236-247
        audio = audio.squeeze(1).float()
        upp_res = int(math.floor(factor * self.tgt_sr // 100))                            # :248
        if upp_res != self.tgt_sr // 100:                                                 # :249-259 (formant shift only)
            if upp_res not in self._resample:
                self._resample[upp_res] = SincResample(upp_res, self.tgt_sr // 100, self.device)
            audio = self._resample[upp_res](audio[:, : return_length * upp_res].contiguous())
        return audio.squeeze()


class SessionSliders:
    """The hot-update controls a bank keeps per session (gui.py:666-681): for each name a list [S] whose entries are a session's own value
    or ``None`` (the session follows the bank-wide value).  Host only: no device, no library."""

    NAMES = ("index_rate", "protect", "rms_mix_rate", "threhold")

    def __init__(self, sessions: int, names=NAMES):
        self.S = int(sessions)
        self.own = {n: [None] * self.S for n in names}

    def set(self, name: str, i: int, v) -> None:
        """``IndexError`` for a session outside the bank, ``ValueError`` for a value that is not finite; ``None`` returns the session to the
        bank-wide value."""
        i = int(i)
        if not 0 <= i < self.S:
            raise IndexError("session %d of %d" % (i, self.S))
        if v is not None and not math.isfinite(float(v)):
            raise ValueError("%s must be finite (got %r)" % (name, v))
        self.own[name][i] = None if v is None else float(v)

    def values(self, name: str, bank_value) -> list:
        """Every session's effective value under the bank-wide ``bank_value``."""
        return [bank_value if v is None else v for v in self.own[name]]

    def differs(self, name: str, bank_value) -> bool:
        """Does some session's effective value differ from the bank-wide one?  (Only then does a bank leave its bank-wide code path.)"""
        return any(v is not None and v != bank_value for v in self.own[name])


class RealtimeVCBatch:
    """``RealtimeVC`` for a bank of ``S`` live sessions that share the model, the index, ``index_rate`` and ``protect``; each has its
    own pitch cache and speaker id.  One ``infer`` is one block of EVERY session: one roll of the ``[S, 1024]`` caches, one
    retrieval call (``glue.retrieve_blend_expand_batch``: one search over all sessions' new frames, the realtime guard per
    session) and one ``net_g.infer`` at batch ``S``.  The launch count does not depend on ``S``.

    The formant shift is per session: ``set_session_formant(i, shift)`` (or ``infer(..., formants=[...])``), kept in ``formants``.  A
    shifted bank decodes every session to its own ``return_length2`` in one ``net_g.infer`` (``return_length2`` = the list: a ragged
    partial decode) and brings the rows back to ``return_length * (tgt_sr // 100)`` samples with one ``SincResampleRagged`` launch; with
    every shift zero it issues exactly the launches it issues without the feature.  The bank-wide forms -- the constructor's
    ``formant_shift`` and the one-argument ``set_formant`` -- serve 0 only.

    ``index_rate`` and ``protect`` may also be set per session: ``set_session_index_rate(i, rate)`` / ``set_session_protect(i, protect)`` (or
    ``infer(..., index_rates=[...], protects=[...])``); a session without its own value follows the bank-wide one, and while none differs
    ``infer`` issues the calls it issues without the feature."""

    def __init__(self, net_g, sessions: int, index=None, index_rate: float = 0.0, device="cuda:0", if_f0: int = 1, tgt_sr: int = 48000,
                 formant_shift: float = 0.0, window: int = 160, cache_size: int = 1024):
        if int(sessions) < 1:
            raise ValueError("a bank has at least one session (got %d)" % int(sessions))
        if formant_shift != 0:
            raise ValueError("RealtimeVCBatch takes no bank-wide formant_shift (got %r): the formant shift is per session, set_session_formant(i, shift)"
                             % (formant_shift,))
        self.net_g, self.index, self.index_rate = net_g, index, float(index_rate)
        self.S, self.device = int(sessions), torch.device(device)
        self.if_f0, self.tgt_sr, self.window = int(if_f0), int(tgt_sr), int(window)
        self.pitch = torch.zeros(self.S, cache_size, device=self.device, dtype=torch.long)
        self.pitchf = torch.zeros(self.S, cache_size, device=self.device, dtype=torch.float32)
        self._sid_host, self._sid = None, None
        self._lengths = {}
        self.formants = [0.0] * self.S   # semitones per session (the GUI's slider: -2 .. 2)
        self._rl2_host, self._rl2 = None, None
        self._resample = SincResampleRagged(self.tgt_sr // 100, self.device)
        self.sliders = SessionSliders(self.S, ("index_rate", "protect"))   # a session's own index_rate / protect; None follows the bank-wide value

    def set_index_rate(self, new_index_rate):
        self.index_rate = float(new_index_rate)

    def set_session_index_rate(self, i: int, rate) -> None:
        """Session ``i``'s ``index_rate`` (rtrvc.py:130-132 per session; ``None``: follow the bank-wide one); takes effect at the next block.
        The session is searched and blended iff there is an index and its rate is above 0, the rule ``RealtimeVC`` applies to its scalar."""
        self.sliders.set("index_rate", i, rate)

    def set_session_protect(self, i: int, protect) -> None:
        """Session ``i``'s ``protect`` (``None``: follow the ``protect`` argument of ``infer``); its protect mix applies iff it is below 0.5
        and the model has f0 (rtrvc.py:224)."""
        self.sliders.set("protect", i, protect)

    def session_controls(self, protect: float):
        """-> (index_rates, protects, differs): every session's effective values under the bank-wide ``index_rate`` and ``protect``, and whether
        any of them is not the bank-wide one (only then does ``infer`` leave ``glue.retrieve_blend_expand_batch``)."""
        sl = self.sliders
        return (sl.values("index_rate", self.index_rate), sl.values("protect", float(protect)),
                sl.differs("index_rate", self.index_rate) or sl.differs("protect", float(protect)))

    def set_formant(self, new_formant):
        if new_formant != 0:
            raise ValueError("RealtimeVCBatch takes no bank-wide formant shift (got %r): use set_session_formant(i, shift)" % (new_formant,))

    def set_session_formant(self, i: int, shift: float) -> None:
        """Session ``i``'s formant shift in semitones (rtrvc.py:128-129 per session); takes effect at the next block."""
        i = int(i)
        if not 0 <= i < self.S:
            raise IndexError("session %d of %d" % (i, self.S))
        if not math.isfinite(float(shift)):
            raise ValueError("formant shift must be finite (got %r)" % (shift,))
        self.formants[i] = shift

    def reset(self, i: int) -> None:
        """Session ``i``'s pitch cache back to zeros (a new talker takes the slot)."""
        self.pitch[int(i)].zero_()
        self.pitchf[int(i)].zero_()

    def _sids(self, sid) -> torch.Tensor:
        host = [int(sid)] * self.S if np.isscalar(sid) else [int(v) for v in sid]
        if len(host) != self.S:
            raise ValueError("sid must hold %d values, got %d" % (self.S, len(host)))
        if host != self._sid_host:   # uploaded when a session's speaker changes, not per block
            self._sid_host, self._sid = host, torch.tensor(host, dtype=torch.long, device=self.device)
        return self._sid

    def infer(self, feats: torch.Tensor, n_input_samples: int, block_frame_16k: int, skip_head: int, return_length: int,
              pitch: Optional[torch.Tensor] = None, pitchf: Optional[torch.Tensor] = None, protect: float = 1.0, sid=0,
              formants=None, index_rates=None, protects=None) -> torch.Tensor:
        """``feats`` [S, n, d] (HuBERT of every session's rolling window), ``pitch`` / ``pitchf`` [S, m] (the estimator's output per
        session; ``None`` for a model without f0), ``sid``: one id or ``S`` of them, ``formants``: ``S`` shifts that replace
        ``self.formants`` (``None`` keeps them); ``index_rates`` / ``protects`` likewise replace the sessions' own values (an entry that is
        ``None`` follows the bank-wide ``index_rate`` / ``protect``).  While no session differs from the bank-wide values the retrieval is
        the one ``glue.retrieve_blend_expand_batch`` call; else ``glue.retrieve_blend_expand_sessions``, which searches only the sessions
        that blend.  Returns the block's waveforms [S, L]; row ``i`` is what ``RealtimeVC.infer`` gives
        session ``i`` alone (with ``formant_shift = formants[i]``), to the batch invariance of ``net_g.infer``.  A session
        whose shift leaves ``upp_res == tgt_sr // 100`` (32 kHz, +0.05) gets the first ``L`` samples of the longer block the solo object returns."""
        if feats.dim() != 3 or feats.shape[0] != self.S:
            raise ValueError("feats must be [%d, n, d], got %s" % (self.S, tuple(feats.shape)))
        if formants is not None:
            if len(formants) != self.S:
                raise ValueError("formants must hold %d values, got %d" % (self.S, len(formants)))
            self.formants = list(formants)
        for name, got in (("index_rates", index_rates), ("protects", protects)):
            if got is not None:
                if len(got) != self.S:
                    raise ValueError("%s must hold %d values, got %d" % (name, self.S, len(got)))
                for i, v in enumerate(got):
                    self.sliders.set(name[:-1], i, v)
        rates, prots, per_session = self.session_controls(protect)
        feats = torch.cat((feats, feats[:, -1:, :]), 1)                                   # rtrvc.py:163
        p_len = int(n_input_samples) // self.window                                       # :189
        shifted = any(f != 0 for f in self.formants)
        return_length2 = int(return_length)                                               # :190-191 at formant_shift 0
        if shifted:                                                                       # :190-191, 248 per session
            geo = [formant_geometry(f, return_length, self.tgt_sr) for f in self.formants]
            rl2s, upp_res = [g[1] for g in geo], [g[2] for g in geo]
            if rl2s != self._rl2_host:   # uploaded when a session's slider moves, not per block
                self._rl2_host, self._rl2 = rl2s, torch.tensor(rl2s, dtype=torch.float32, device=self.device)[:, None]
        pf = pitchf if (min(prots) < 0.5 and pitch is not None and pitchf is not None) else None   # :224 (some session's protect applies)
        if pf is not None and (pf.dim() != 2 or pf.shape[1] != p_len):
            raise RuntimeError("protect < 0.5 needs pitchf of exactly p_len = %d frames per session (got %s), as the reference's broadcast at "
                               "infer/lib/rtrvc.py:229 does" % (p_len, tuple(pf.shape)))
        cache_pitch = cache_pitchf = None
        if self.if_f0 == 1:
            if pitch is None or pitchf is None:
                raise ValueError("an f0 model needs the block's pitch / pitchf")
            if pitch.dim() != 2 or pitch.shape[0] != self.S or pitchf.shape != pitch.shape:
                raise ValueError("pitch / pitchf must be [%d, m], got %s / %s" % (self.S, tuple(pitch.shape), tuple(pitchf.shape)))
            shift = int(block_frame_16k) // self.window                                   # :213-217, every session at once
            n = int(pitch.shape[1])
            if n < 5 or n - 4 > self.pitch.shape[1]:
                raise ValueError("pitch block of %d frames does not fit the cache" % n)
            if shift > 0:
                self.pitch[:, :-shift] = self.pitch[:, shift:].clone()
                self.pitchf[:, :-shift] = self.pitchf[:, shift:].clone()
            self.pitch[:, 4 - n:] = pitch[:, 3:-1].to(self.device, torch.long)
            self.pitchf[:, 4 - n:] = pitchf[:, 3:-1].to(self.device, torch.float32)
            # :216-219; per session the same float32 product and quotient as the solo object's python scalars
            cache_pitch = self.pitch[:, -p_len:]
            cache_pitchf = self.pitchf[:, -p_len:] * (self._rl2 if shifted else return_length2) / return_length
        if per_session:   # :167-185, 221-233 with each session's own scalars: it blends iff index and rate > 0, protect-mixes iff protect < 0.5 and f0
            phone = glue.retrieve_blend_expand_sessions(feats, self.index, [r if r > 0 else 0.0 for r in rates], pf,
                                                        prots if pf is not None else [1.0] * self.S, p_len, realtime_guard=True,
                                                        skip_rows=int(skip_head) // 2)
        else:
            use_index = self.index is not None and self.index_rate > 0                    # :167
            phone = glue.retrieve_blend_expand_batch(feats, self.index if use_index else None, self.index_rate if use_index else 0.0,
                                                     pf, protect if pf is not None else 1.0, p_len, realtime_guard=True,
                                                     skip_rows=int(skip_head) // 2)        # :167-185, 221-233
        lengths = self._lengths.get(p_len)
        if lengths is None:
            lengths = self._lengths[p_len] = torch.full((self.S,), p_len, dtype=torch.long, device=self.device)
        with torch.no_grad():
            audio = self.net_g.infer(phone, lengths, self._sids(sid), pitch=cache_pitch, pitchf=cache_pitchf, skip_head=skip_head,
                                     return_length=return_length, return_length2=rl2s if shifted else return_length2)   # :236-247
        audio = audio.squeeze(1).float()
        if shifted:                                                                       # :248-259: [S, max(rl2) * upp] -> [S, return_length * tgt_sr // 100]
            audio = self._resample(audio, upp_res, int(return_length))
        return audio


def stream_geometry(samplerate: int, block_time: float = 0.25, crossfade_time: float = 0.05, extra_time: float = 2.5) -> dict:
    """The realtime GUI's block geometry (gui.py:783-840), in samples at ``samplerate`` unless named ``_16k``; no device needed."""
    sr = int(samplerate)
    zc = sr // 100
    block = int(np.round(block_time * sr / zc)) * zc
    crossfade = int(np.round(crossfade_time * sr / zc)) * zc
    sola_buffer = min(crossfade, 4 * zc)
    search = zc
    extra = int(np.round(extra_time * sr / zc)) * zc
    n_in = extra + crossfade + search + block
    return dict(zc=zc, block_frame=block, block_frame_16k=160 * block // zc, crossfade_frame=crossfade, sola_buffer_frame=sola_buffer,
                sola_search_frame=search, extra_frame=extra, skip_head=extra // zc, return_length=(block + sola_buffer + search) // zc,
                input_wav_len=n_in, input_wav_res_len=160 * n_in // zc)


def frame_rms_np(y: np.ndarray, frame_length: int, hop_length: int) -> np.ndarray:
    """``librosa.feature.rms(y=y, frame_length, hop_length)[0]`` (librosa >= 0.10.2: centred, zero padding) in numpy; the float32
    squares are summed in float64 and the mean rounded to float32, as the device's k_frame_rms_batch does."""
    y = np.asarray(y, dtype=np.float32)
    pad = frame_length // 2
    yp = np.pad(y, (pad, pad), mode="constant")
    n_frames = 1 + (len(yp) - frame_length) // hop_length
    sq = (yp * yp).astype(np.float64)
    sums = np.array([sq[i * hop_length: i * hop_length + frame_length].sum() for i in range(n_frames)], dtype=np.float64)
    return np.sqrt((sums / frame_length).astype(np.float32))


def amplitude_to_db(s: np.ndarray, amin: float = 1e-5, top_db: float = 80.0) -> np.ndarray:
    """``librosa.amplitude_to_db(s, ref=1.0, amin=1e-5, top_db=80.0)`` in float32: ``10 log10(max(amin^2, s^2))``, clipped at
    ``max - top_db``."""
    power = np.square(np.abs(np.asarray(s, dtype=np.float32)))
    log_spec = (np.float32(10.0) * np.log10(np.maximum(np.float32(amin * amin), power))).astype(np.float32)
    if log_spec.size:
        log_spec = np.maximum(log_spec, log_spec.max() - np.float32(top_db))
    return log_spec


def input_gate(indata: np.ndarray, rms_buffer: np.ndarray, zc: int, threhold: float) -> np.ndarray:
    """The GUI's input gate (gui.py:950-963), on the host where the block arrives: frame RMS over the last ``4 zc`` samples of
    the previous block and this one, frames below ``threhold`` dB zeroed ``zc`` samples at a time.  Updates ``rms_buffer``
    [4 zc] in place and returns ``block + 2 zc`` samples (the GUI rewrites the last ``2 zc`` of the previous block too)."""
    x = np.append(rms_buffer, np.asarray(indata, dtype=np.float32))
    rms = frame_rms_np(x, 4 * zc, zc)[2:]
    rms_buffer[:] = x[-4 * zc:]
    x = x[2 * zc - zc // 2:]
    quiet = amplitude_to_db(rms) < threhold
    for i in np.flatnonzero(quiet):
        x[i * zc: (i + 1) * zc] = 0
    return x[zc // 2:]


_GATE_CUTOFFS: dict = {}


def _first_true(pred) -> np.float32:
    """The smallest non-negative float32 ``r`` (+inf included) with ``pred(r)``, for a ``pred`` that is monotone in ``r`` (false, then
    true): bisection over the bit patterns 0 .. 0x7f800000, which order like the values.  +inf when there is none."""
    bits = lambda b: np.array([b], np.uint32).view(np.float32)[0]  # noqa: E731
    lo, hi = 0, 0x7F800000
    if not pred(bits(hi)):
        return np.float32(np.inf)
    while lo < hi:
        mid = (lo + hi) // 2
        if pred(bits(mid)):
            hi = mid
        else:
            lo = mid + 1
    return bits(lo)


def input_gate_cutoffs(threhold: float):
    """The gate's decision ``amplitude_to_db(rms)[i] < threhold`` (``input_gate``) as two float32 RMS cutoffs, for the device gate
    (``glue.input_gate_batch``), which evaluates no logarithm: ``amplitude_to_db`` is monotone in the RMS, and with the 80 dB clip
    ``db[i] = max(db1(rms[i]), db1(max rms) - 80)``, so

        frame i is quiet  iff  rms[i] < cut_a  and  max_i rms[i] < cut_b

    with ``cut_a`` the smallest float32 ``r >= 0`` for which ``db1(r) < threhold`` is false and ``cut_b`` the smallest for which
    ``float32(db1(r) - float32(80)) < threhold`` is false; ``db1`` is ``amplitude_to_db`` itself on the single value.  Both are found by
    bisection over float32 bit patterns and cached per threshold; no device is needed.  The ends: a threshold at or below the floor of
    ``db1`` (-100 dB, the ``amin`` of 1e-5) gives ``cut_a == 0`` -- no frame is ever quiet; a threshold above every level a finite
    ``rms ** 2`` reaches (385.3 dB) puts a cutoff where the float32 square overflows (1.8447e19), or at +inf if not even that level
    fails the comparison.  -> (cut_a, cut_b) as python floats that are exact float32 values."""
    t = float(threhold)
    hit = _GATE_CUTOFFS.get(t)
    if hit is None:
        db1 = lambda r: amplitude_to_db(np.array([r], np.float32))  # noqa: E731  (arrays, so that `< threhold` promotes as in input_gate)
        with np.errstate(over="ignore", invalid="ignore"):
            cut_a = _first_true(lambda r: not bool((db1(r) < t)[0]))
            cut_b = _first_true(lambda r: not bool(((db1(r) - np.float32(80.0)).astype(np.float32) < t)[0]))
        if len(_GATE_CUTOFFS) > 256:
            _GATE_CUTOFFS.clear()
        hit = _GATE_CUTOFFS[t] = (float(cut_a), float(cut_b))
    return hit


BANK_DEVICE_GATE = True      # RealtimeBank(device_gate=None); RVCMI_RT_DEVICE_GATE=1 / =0 overrides both defaults.  Decided by tools/rt_bank_gate_time.py
STREAM_DEVICE_GATE = True    # RealtimeStream(device_gate=None)                          (profiles/rt_bank_gate_time.json: the device gate's range lies below the host gate's)


def _device_gate(arg, default: bool) -> bool:
    import os

    if arg is not None:
        return bool(arg)
    env = os.environ.get("RVCMI_RT_DEVICE_GATE")
    return default if env in (None, "") else env != "0"


class RealtimeStream:
    """The per-block audio path of the realtime GUI (``audio_infer``, gui.py:934-1090) around any ``rtrvc.RVC``-like object
    (``.tgt_sr`` and ``.infer(input_wav_res, block_frame_16k, skip_head, return_length, f0method)``; the reference's own after
    ``rvc_amd.install()``), without the PySimpleGUI front end:

        rt = RealtimeStream(rvc, samplerate=48000, use_pv=True)
        out = rt.process(block)        # host float32 [block_frame] or [block_frame, channels] -> device float32 [block_frame]

    Per block: the input gate (when ``threhold > -60``; on the host, or with ``device_gate=True`` on the device: ``glue.input_gate_batch`` at
    ``S = 1``, bit-equal; ``None`` reads ``RVCMI_RT_DEVICE_GATE``, else ``STREAM_DEVICE_GATE``), rolling ``input_wav`` / ``input_wav_res`` buffers and the 16 kHz
    resample, ``rvc.infer``, the ``tgt_sr -> samplerate`` resample, the envelope mix (``rms_mix_rate < 1``) and the SOLA stitch
    (sin^2 or phase-vocoder fade), all on the device: one host-to-device copy (the block), none back.  The keyword names are the
    GUI's ``GUIConfig`` fields; ``samplerate=None`` is the model rate.  ``I_noise_reduce`` / ``O_noise_reduce`` (the GUI's
    noise-reduction boxes, gui.py:974-992, 1015-1022) gate the input and the converted block with ``TorchGateHIP``;
    ``function="im"`` is the monitor mode (gui.py:1000-1013: no ``rvc.infer``, ``rvc`` may be None when ``samplerate`` is given).
    All three are plain attributes that may change between blocks, as the GUI's hot update does."""

    def __init__(self, rvc, samplerate: Optional[int] = None, block_time: float = 0.25, crossfade_time: float = 0.05, extra_time: float = 2.5,
                 threhold: float = -60, rms_mix_rate: float = 0.0, use_pv: bool = False, f0method: str = "rmvpe", device=None,
                 I_noise_reduce: bool = False, O_noise_reduce: bool = False, function: str = "vc", device_gate: Optional[bool] = None):
        self.rvc = rvc
        self.device_gate = _device_gate(device_gate, STREAM_DEVICE_GATE)
        if rvc is None and samplerate is None:
            raise ValueError("RealtimeStream without an rvc object (the \"im\" mode) needs samplerate")
        self.tgt_sr = int(rvc.tgt_sr) if rvc is not None else int(samplerate)
        self.samplerate = self.tgt_sr if samplerate is None else int(samplerate)
        self.block_time, self.crossfade_time, self.extra_time = block_time, crossfade_time, extra_time
        self.threhold, self.rms_mix_rate, self.use_pv, self.f0method = threhold, float(rms_mix_rate), bool(use_pv), f0method
        self.I_noise_reduce, self.O_noise_reduce, self.function = I_noise_reduce, O_noise_reduce, function
        if device is None:
            device = getattr(rvc, "device", None) or "cuda:0"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.RvcmiError("RealtimeStream runs on the GPU (got %s); there is no CPU fallback" % self.device)
        g = stream_geometry(self.samplerate, block_time, crossfade_time, extra_time)
        for k, v in g.items():
            setattr(self, k, v)
        self.input_wav = torch.zeros(self.input_wav_len, device=self.device, dtype=torch.float32)
        self.input_wav_res = torch.zeros(self.input_wav_res_len, device=self.device, dtype=torch.float32)
        # the input gate's 4 zc samples of history: on the host with the host gate, on the device with the device gate
        self.rms_buffer = torch.zeros(4 * self.zc, device=self.device, dtype=torch.float32) if self.device_gate else np.zeros(4 * self.zc, dtype="float32")
        self._gate_scratch = None
        self.sola_buffer = torch.zeros(self.sola_buffer_frame, device=self.device, dtype=torch.float32)
        # gui.py:825, 835-836: kept whatever the noise-reduction boxes say, updated only while they are ticked
        self.input_wav_denoise = self.input_wav.clone()
        self.nr_buffer = self.sola_buffer.clone()
        self.output_buffer = self.input_wav.clone()
        # the GUI's fp32 expression (gui.py:841-855), on the CPU and uploaded once
        fade_in = torch.sin(0.5 * np.pi * torch.linspace(0.0, 1.0, steps=self.sola_buffer_frame, dtype=torch.float32)) ** 2
        self.fade_in_window = fade_in.to(self.device)
        self.fade_out_window = (1 - fade_in).to(self.device)
        self.resampler = SincResample(self.samplerate, 16000, self.device)
        self.resampler2 = SincResample(self.tgt_sr, self.samplerate, self.device) if self.tgt_sr != self.samplerate else None
        self.tg = TorchGateHIP(sr=self.samplerate, n_fft=4 * self.zc, prop_decrease=0.9).to(self.device)   # gui.py:869-871
        self.last_offset = None  # device int32 [1]: the SOLA offset of the last block

    def process(self, indata) -> torch.Tensor:
        x = np.asarray(indata, dtype=np.float32)
        if x.ndim == 2:
            x = np.mean(x.T, axis=0)       # librosa.to_mono(indata.T)
        if x.shape[0] != self.block_frame:
            raise ValueError("a block has %d samples, got %d" % (self.block_frame, x.shape[0]))
        blk, blk16 = self.block_frame, self.block_frame_16k
        on_device = self.threhold > -60 and self.device_gate
        if self.threhold > -60 and not on_device:
            x = input_gate(x, self.rms_buffer, self.zc, self.threhold)
        m = blk + 2 * self.zc if on_device else int(x.shape[0])
        self.input_wav[:-blk] = self.input_wav[blk:].clone()
        if on_device:   # the bank's entry at S = 1: the raw block goes up, the gate writes the tail of input_wav
            if self._gate_scratch is None:
                self._gate_scratch = torch.empty(glue.input_gate_scratch_floats(self.zc, blk), device=self.device, dtype=torch.float32)
            glue.input_gate_batch(torch.from_numpy(np.ascontiguousarray(x)).to(self.device)[None], self.rms_buffer[None], self.input_wav[None, -m:],
                                  self.zc, *input_gate_cutoffs(self.threhold), scratch=self._gate_scratch)
        else:
            self.input_wav[-m:] = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        self.input_wav_res[:-blk16] = self.input_wav_res[blk16:].clone()
        Lb = self.sola_buffer_frame
        if self.I_noise_reduce:                                                          # gui.py:974-992
            self.input_wav_denoise[:-blk] = self.input_wav_denoise[blk:].clone()
            input_wav = self.tg(self.input_wav[None, -Lb - blk:], self.input_wav[None]).squeeze(0)
            input_wav[:Lb] *= self.fade_in_window
            input_wav[:Lb] += self.nr_buffer * self.fade_out_window
            self.input_wav_denoise[-blk:] = input_wav[:blk]
            self.nr_buffer[:] = input_wav[blk:]
            self.input_wav_res[-blk16 - 160:] = self.resampler(self.input_wav_denoise[-blk - 2 * self.zc:])[160:]
        else:
            self.input_wav_res[-160 * (m // self.zc + 1):] = self.resampler(self.input_wav[-m - 2 * self.zc:])[160:]
        vc = self.function == "vc"
        if vc:
            infer_wav = self.rvc.infer(self.input_wav_res, blk16, self.skip_head, self.return_length, self.f0method)
            if self.resampler2 is not None:
                infer_wav = self.resampler2(infer_wav)
            infer_wav = infer_wav.reshape(-1)
            if infer_wav.dtype != torch.float32 or not infer_wav.is_contiguous():
                infer_wav = infer_wav.float().contiguous()
        else:                                                                            # gui.py:1000-1013, "im"
            infer_wav = (self.input_wav_denoise if self.I_noise_reduce else self.input_wav)[self.extra_frame:].clone()
        if self.O_noise_reduce and vc:                                                   # gui.py:1015-1022
            self.output_buffer[:-blk] = self.output_buffer[blk:].clone()
            self.output_buffer[-blk:] = infer_wav[-blk:]
            infer_wav = self.tg(infer_wav[None], self.output_buffer[None]).squeeze(0)
        if self.rms_mix_rate < 1 and vc:
            n = int(infer_wav.numel())
            src = self.input_wav_denoise if self.I_noise_reduce else self.input_wav
            glue.envelope_mix(src[self.extra_frame: self.extra_frame + n], infer_wav, self.zc, self.rms_mix_rate)
        out, self.last_offset = glue.sola(infer_wav, self.sola_buffer, self.fade_in_window, self.fade_out_window, blk, self.sola_search_frame,
                                          return_offset=True, use_pv=self.use_pv)
        return out


RT_GRAPH_AFTER = 3  # eager calls of one (window length, key) before its f0 chain is captured (MIOpen / rocFFT pick their algorithms and plans first)


def _rmvpe_f0_graphed(self, wav: torch.Tensor, p_len: int, key: int):
    """``pipeline._rmvpe_on_device`` for the realtime loop, whose f0 window has the SAME length block after block (rtrvc.py:203-207): the chain
    waveform -> mel -> RMVPE -> salience decode is ~400 launches for a 32-frame input -- 7 ms of host time eager, 90 M parameters of U-Net at a
    tiny size -- so after ``RT_GRAPH_AFTER`` eager calls it is captured ONCE per (window length, key) into a hipGraph with a static input buffer
    and replayed (the launch-bound inner loop the design captures everywhere else too).  Same kernels, same results.  ``RVCMI_RT_GRAPH=0``, a
    capture that fails (an op that cannot be captured in this build), or a CPU / foreign estimator keep the eager call.  -> (pitch, pitchf)
    [1, p_len] like ``_rmvpe_on_device`` (tensors the next replay overwrites: the caller copies them into its pitch cache at once), or None."""
    import os

    from .pipeline import _rmvpe_on_device

    if os.environ.get("RVCMI_RT_GRAPH", "1") == "0" or not (torch.is_tensor(wav) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 1):
        return _rmvpe_on_device(self, wav, p_len, key)
    cache = self.__dict__.setdefault("_rvcmi_f0_graphs", {})
    k = (int(wav.shape[0]), int(p_len), int(key) if float(key).is_integer() else float(key), str(wav.device))  # (the key's factor is baked into the graph)
    e = cache.setdefault(k, {"calls": 0})
    if "graph" in e:
        e["in"].copy_(wav)
        e["graph"].replay()
        return e["out"]
    out = _rmvpe_on_device(self, wav, p_len, key)
    e["calls"] += 1
    if out is not None and e["calls"] == RT_GRAPH_AFTER:
        try:
            static_in = wav.clone()
            torch.cuda.synchronize(wav.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                o = _rmvpe_on_device(self, static_in, p_len, key)
            if o is None:
                raise RuntimeError("no device f0 inside the capture")
            e.update(graph=g, out=o)
            e["in"] = static_in
        except Exception as ex:  # noqa  (keeps the eager path; never tried again for this key)
            import warnings

            warnings.warn("rvc_amd: the realtime f0 chain could not be captured into a hipGraph (%s: %s); running it eager" % (type(ex).__name__, ex))
            torch.cuda.synchronize(wav.device)
    return out


def rvc_infer_hip(self, input_wav: torch.Tensor, block_frame_16k, skip_head, return_length, f0method, protect: float = 1.0):
    """Drop-in ``RVC.infer`` (infer/lib/rtrvc.py:134-260; bound by ``rvc_amd.install()``): HuBERT and the f0 estimator are the
    object's own PyTorch modules, everything after them runs on the device through a ``RealtimeVC`` that lives on the object.
    A precomputed ``(pitch, pitchf)`` tuple or an index object that is not ours goes to the reference's own method."""
    from .ivf import IVFFlatHIP

    index = getattr(self, "index", None)
    if isinstance(f0method, tuple) or (index is not None and not isinstance(index, IVFFlatHIP)):
        orig = getattr(rvc_infer_hip, "_rvcmi_original", None)
        if orig is None:
            raise TypeError("RVC.infer: unsupported arguments for the HIP path and no reference method is bound")
        return orig(self, input_wav, block_frame_16k, skip_head, return_length, f0method, protect)
    rt = getattr(self, "_rvcmi_rt", None)
    if rt is None or rt.net_g is not self.net_g:
        rt = self._rvcmi_rt = RealtimeVC(self.net_g, index=index, index_rate=self.index_rate, device=self.device, if_f0=self.if_f0,
                                         tgt_sr=self.tgt_sr, f0_up_key=self.f0_up_key, formant_shift=self.formant_shift,
                                         window=self.window)
    rt.index, rt.index_rate = index, float(self.index_rate)      # set_index_rate / set_key / set_formant act on the RVC object
    rt.f0_up_key, rt.formant_shift = self.f0_up_key, self.formant_shift
    with torch.no_grad():                                           # rtrvc.py:142-162
        feats = input_wav.half() if self.is_half else input_wav.float()
        feats = feats.to(self.device)
        if feats.dim() == 2:
            feats = feats.mean(-1)
        feats = feats.view(1, -1)
        mask = torch.zeros(feats.shape, dtype=torch.bool, device=feats.device)
        from .hubert import accelerate_hubert_layers_once, accelerate_hubert_once

        accelerate_hubert_once(self.hubert)  # (opt-in, a no-op with the switch off)
        accelerate_hubert_layers_once(self.hubert)  # (RVCMI_HUBERT_ENC, opt-in, likewise)
        logits = self.hubert.extract_features(source=feats, padding_mask=mask, output_layer=9 if self.version == "v1" else 12)
        feats = self.hubert.final_proj(logits[0]) if self.version == "v1" else logits[0]
    pitch = pitchf = None
    if self.if_f0 == 1:                                             # rtrvc.py:203-212
        n = f0_extractor_frame(block_frame_16k, f0method, self.window)
        key = self.f0_up_key - self.formant_shift
        got = None
        from .rmvpe import rmvpe_on

        if f0method == "rmvpe" and (float(key).is_integer() or rmvpe_on()) and getattr(self, "f0_gen", None) is not None:
            # RMVPE stays on the device from the waveform to (pitch, pitchf): the reference's Generator.calculate (rvc/f0/gen.py:58-59, 103-113) copies
            # the window to the host, the salience back, and decodes it in numpy with a python loop over frames; pipeline._rmvpe_on_device is the same
            # chain (mel, network, rvcmi_glue_rmvpe_f0 = _decode + _resize_f0 + _interpolate_f0 + post_process, golden-tested against the reference's)
            # without a host hop, and swaps the network's GRU for the HIP one (3.7 / 7.2 ms -> 0.06 / 0.10 ms for a 32- / 64-frame window,
            # tools/gru_time.py), replayed from a hipGraph after the first blocks (_rmvpe_f0_graphed).  A fractional key (formant slider) takes the
            # reference's own method below unless the opt-in RMVPE switch (rmvpe.py) is on: then it stays on the device too.
            w_f0 = input_wav[-n:]
            got = _rmvpe_f0_graphed(self, w_f0.contiguous() if torch.is_tensor(w_f0) else w_f0, int(w_f0.shape[0]) // self.window, int(key) if float(key).is_integer() else float(key))
        if got is not None:
            pitch, pitchf = got[0][0], got[1][0]
        else:
            if f0method == "rmvpe" and getattr(getattr(self, "f0_gen", None), "rmvpe", None) is not None:
                from .gru import accelerate_f0_rmvpe

                accelerate_f0_rmvpe(self.f0_gen.rmvpe)   # (beyond SURVEY 8) at least the network's GRU, once the generator has loaded it
            pitch, pitchf = self._get_f0(input_wav[-n:], key, method=f0method)
    return rt.infer(feats, int(input_wav.shape[0]), block_frame_16k, skip_head, return_length, pitch=pitch, pitchf=pitchf, protect=protect)


def rvc_infer_batch_hip(self, input_wav: torch.Tensor, block_frame_16k, skip_head, return_length, f0method, protect: float = 1.0,
                        keys=None, sids=None, rt: Optional[RealtimeVCBatch] = None, formants=None, index_rates=None,
                        protects=None) -> torch.Tensor:
    """``rvc_infer_hip`` for ``S`` sessions of one voice: ``input_wav`` [S, n16] (every session's rolling 16 kHz window) -> [S, L].
    HuBERT runs once on the ``[S, n16]`` batch (equal lengths: the padding mask is all-false), the RMVPE network once on the
    ``[S, .]`` f0 windows, and the salience decode of all sessions in one ``glue.rmvpe_f0_ragged`` call, each with its own key (``keys``,
    default the object's ``f0_up_key``; ``sids`` default 0).  ``rt``: the ``RealtimeVCBatch`` that holds the sessions' pitch caches (default: one kept on
    the object).  ``formants``: a formant shift per session (default: the ones ``rt`` holds); session ``s``'s f0 key is then
    ``keys[s] - formants[s]`` (rtrvc.py:208) and ``rt.infer`` decodes and resamples it by its own factor.  ``index_rates`` / ``protects``: an
    ``index_rate`` / ``protect`` per session (default: the ones ``rt`` holds; an entry that is ``None`` follows the object's ``index_rate`` /
    the ``protect`` argument), handed to ``rt.infer``.  Not served, and refused: a
    precomputed ``(pitch, pitchf)`` tuple, an index object that is not ours, a bank-wide ``formant_shift`` on the object."""
    from .ivf import IVFFlatHIP

    index = getattr(self, "index", None)
    if isinstance(f0method, tuple) or (index is not None and not isinstance(index, IVFFlatHIP)):
        raise TypeError("rvc_infer_batch_hip serves neither a precomputed (pitch, pitchf) tuple nor a foreign index object")
    if input_wav.dim() != 2 or input_wav.shape[0] < 1:
        raise ValueError("input_wav must be [S, n16] with S >= 1, got %s" % (tuple(input_wav.shape),))
    if getattr(self, "formant_shift", 0) != 0:
        raise ValueError("a bank takes no bank-wide formant_shift (got %r on the rvc object): pass formants= per session / RealtimeBank.set_formant(i, shift)"
                         % (self.formant_shift,))
    S = int(input_wav.shape[0])
    keys = [self.f0_up_key] * S if keys is None else list(keys)
    sids = [0] * S if sids is None else list(sids)
    if len(keys) != S or len(sids) != S:
        raise ValueError("keys / sids must hold one value per session (%d)" % S)
    if rt is None:
        rt = getattr(self, "_rvcmi_rt_bank", None)
        if rt is None or rt.net_g is not self.net_g or rt.S != S:
            rt = self._rvcmi_rt_bank = RealtimeVCBatch(self.net_g, S, index=index, index_rate=self.index_rate, device=self.device,
                                                       if_f0=self.if_f0, tgt_sr=self.tgt_sr, window=self.window)
    elif rt.S != S:
        raise ValueError("the RealtimeVCBatch holds %d sessions, input_wav %d" % (rt.S, S))
    rt.index, rt.index_rate = index, float(self.index_rate)
    formants = list(rt.formants) if formants is None else list(formants)
    if len(formants) != S:
        raise ValueError("formants must hold one value per session (%d)" % S)
    keys = [k - f if f != 0 else k for k, f in zip(keys, formants)]   # rtrvc.py:208: f0_up_key - formant_shift, per session
    with torch.no_grad():                                           # rtrvc.py:142-162, all sessions at once
        feats = input_wav.half() if self.is_half else input_wav.float()
        feats = feats.to(self.device)
        mask = torch.zeros(feats.shape, dtype=torch.bool, device=feats.device)
        from .hubert import accelerate_hubert_layers_once, accelerate_hubert_once

        accelerate_hubert_once(self.hubert)
        accelerate_hubert_layers_once(self.hubert)
        logits = self.hubert.extract_features(source=feats, padding_mask=mask, output_layer=9 if self.version == "v1" else 12)
        feats = self.hubert.final_proj(logits[0]) if self.version == "v1" else logits[0]
    pitch = pitchf = None
    if self.if_f0 == 1:                                             # rtrvc.py:203-212
        from .pipeline import RMVPE_THRED, _torch_rmvpe
        from .rmvpe import for_generator, rmvpe_on

        n = f0_extractor_frame(block_frame_16k, f0method, self.window)
        w = input_wav[:, -n:]
        m = int(w.shape[1]) // self.window
        r = _torch_rmvpe(self) if (f0method == "rmvpe" and getattr(self, "f0_gen", None) is not None) else None
        if r is not None:
            hip = for_generator(self.f0_gen, r) if rmvpe_on() else None
            if hip is not None:   # the packed rows of the ragged pass, as they lie (no clone per session)
                sal, off, frames = hip._salience_ragged(hip._wavs([w[s].float().to(hip.device) for s in range(S)]))
                rows = [(off[s], frames[s], m, keys[s]) for s in range(S)]
            else:
                from .gru import accelerate_f0_rmvpe

                accelerate_f0_rmvpe(r)
                with torch.no_grad():
                    hidden = r._mel2hidden(r.mel_extractor(w.float().to(r.device), center=True))
                T = int(hidden.shape[1])
                sal = hidden.float().contiguous().view(S * T, int(hidden.shape[2]))   # [S, T, 360] seen as [S * T, 360]
                rows = [(s * T, T, m, keys[s]) for s in range(S)]
            # every session asks glue.rmvpe_f0 for its rows with its own key, as before; inside glue._f0_gather the calls launch nothing and the
            # block ends in ONE rvcmi_glue_rmvpe_f0_ragged: two launches whatever S, each row the bits of the call alone
            with glue._f0_gather(sal, S * m, RMVPE_THRED) as gathered:
                for r0, nr, p, k in rows:
                    glue.rmvpe_f0(sal[r0: r0 + nr], p, k if (hip is not None or not float(k).is_integer()) else int(k), RMVPE_THRED)
            if len(gathered.rows) != S:   # (a glue.rmvpe_f0 that did not recognise its rows would have decoded alone: never quietly)
                raise _lib.RvcmiError("rvc_infer_batch_hip: %d of %d sessions' decodes were gathered" % (len(gathered.rows), S))
            pitch, pitchf = gathered.pitch.view(S, m).to(self.device), gathered.pitchf.view(S, m).to(self.device)
        else:
            got = []
            for s in range(S):
                p, pf = self._get_f0(input_wav[s, -n:], keys[s], method=f0method)
                got.append((p.reshape(1, -1), pf.reshape(1, -1)))
            pitch = torch.cat([g[0].to(self.device) for g in got], 0)
            pitchf = torch.cat([g[1].to(self.device) for g in got], 0)
    return rt.infer(feats, int(input_wav.shape[1]), block_frame_16k, skip_head, return_length, pitch=pitch, pitchf=pitchf, protect=protect,
                    sid=sids, formants=formants, index_rates=index_rates, protects=protects)


class RealtimeBank:
    """``S`` live streams of ONE voice in one pass per block: a bank of ``RealtimeStream`` sessions that share the model, the index,
    the sample rate and the block geometry.  Each session has its own rolling buffers, SOLA tail, input gate, pitch cache, speaker
    id, pitch key and formant shift:

        bank = RealtimeBank(rvc, sessions=S, samplerate=48000, use_pv=True)
        out = bank.process(blocks)     # host float32 [S, block_frame] -> device float32 [S, block_frame]
        bank.set_key(i, key); bank.set_sid(i, sid); bank.set_formant(i, shift); bank.set_noise_reduce(i, I=True, O=False); bank.reset(i)
        bank.last_offsets              # device int32 [S]: every session's SOLA offset of the last block

    Per block: the input gate (when ``threhold > -60``: on the host per session, or with ``device_gate=True`` one
    ``glue.input_gate_batch`` for all sessions, bit-equal; ``None`` reads ``RVCMI_RT_DEVICE_GATE``, else ``BANK_DEVICE_GATE``), ONE
    host-to-device copy of the block (``[S, m]`` gated, or raw ``[S, block_frame]`` with the device gate), then on the device the 16 kHz
    resample, ``rvc_infer_batch_hip`` (HuBERT, f0, retrieval and ``net_g.infer`` at batch ``S``), the ``tgt_sr -> samplerate`` resample,
    the envelope mix and the SOLA stitch, each as ONE set of launches for all sessions (``rvcmi_glue_*_batch``).  Nothing is read back.
    Every DSP step is bit-equal, per session, to ``RealtimeStream``'s.  ``rvc`` is an ``rtrvc.RVC``-like object; one that has an
    ``infer_batch(input_wav_res [S, n16], block_frame_16k, skip_head, return_length, f0method, keys, sids)`` method is asked instead
    of ``rvc_infer_batch_hip``.

    The GUI's noise-reduction boxes (gui.py:974-992, 1015-1022) are per session and switchable between blocks: ``set_noise_reduce(i, I,
    O)``.  The gate of all ticked sessions is one ``TorchGateBank`` call per box (six launches whatever ``S``) that keeps every session's
    noise spectra from block to block and transforms only the frames the block rewrote; the cross-fade, the rolling ``input_wav_denoise`` /
    ``nr_buffer`` / ``output_buffer`` rows and the 16 kHz write-back are masked per session, so each session equals a ``RealtimeStream``
    with its boxes bit for bit.  The launch count depends on whether any session has I and whether any has O ticked, never on ``S`` or on
    which sessions they are; with no box ticked the step issues exactly the launches it issues without this feature.  The spectrum caches
    are allocated at the first block that needs them: ``TorchGateBank.ring_bytes``, 4.3 MB per session and box at 48 kHz.

    Not served, and refused by the constructor: bank-wide ``I_noise_reduce`` / ``O_noise_reduce`` arguments (the boxes are per session),
    the monitor mode ``function="im"``; a bank-wide formant shift (``rvc.formant_shift != 0``) is refused at the first block.  The step
    is eager: it is not captured into a hipGraph.

    The formant slider is per session and switchable between blocks like the key: ``set_formant(i, shift)``.  A shifted bank decodes each
    session to its own length in the one ``net_g.infer`` and resamples all rows in one launch (``RealtimeVCBatch``); that adds three
    launches to the block whatever ``S`` and however many distinct shifts there are, and with every shift zero the step issues exactly the
    launches it issues without this feature.  A custom ``rvc.infer_batch`` is passed ``formants=`` only while some session's shift is non-zero.

    The GUI's remaining hot-update sliders are per session too: ``set_index_rate(i, rate)``, ``set_protect(i, protect)``,
    ``set_rms_mix_rate(i, rate)`` and ``set_threhold(i, db)`` (``SessionSliders``), each effective at the next block and ``None`` to return to
    the bank-wide value (``rvc.index_rate`` and the constructor's ``protect`` / ``rms_mix_rate`` / ``threhold``).  While no session differs
    from the bank-wide value of a control, its step is the bank-wide one above, launch for launch.  Otherwise the step reads the sessions'
    values from device memory (``glue.input_gate_sessions``, ``glue.envelope_mix_sessions``, ``glue.retrieve_blend_expand_sessions``; uploaded
    when a slider moves, not per block): gated sessions get ``blk + 2 zc`` gated samples and their own 16 kHz range, the others their raw
    ``blk``; only the sessions whose ``index_rate`` is above 0 are searched.  The launch count depends on neither ``S`` nor on which sessions
    are active.  What stays the bank's: the sample rate, the block geometry, ``use_pv``, the model and the index."""

    def __init__(self, rvc, sessions: int, samplerate: Optional[int] = None, block_time: float = 0.25, crossfade_time: float = 0.05,
                 extra_time: float = 2.5, threhold: float = -60, rms_mix_rate: float = 0.0, use_pv: bool = False, f0method: str = "rmvpe",
                 device=None, I_noise_reduce: bool = False, O_noise_reduce: bool = False, function: str = "vc", protect: float = 1.0,
                 device_gate: Optional[bool] = None):
        if int(sessions) < 1:
            raise ValueError("a bank has at least one session (got %d)" % int(sessions))
        if I_noise_reduce or O_noise_reduce:
            raise ValueError("RealtimeBank does not serve noise reduction (I_noise_reduce / O_noise_reduce) bank-wide: tick the boxes per session "
                             "with set_noise_reduce(i, I, O)")
        if function != "vc":
            raise ValueError("RealtimeBank serves function=\"vc\" only (got %r); the monitor mode is RealtimeStream's" % (function,))
        if rvc is None:
            raise ValueError("RealtimeBank needs an rvc object")
        self.rvc, self.S = rvc, int(sessions)
        self.tgt_sr = int(rvc.tgt_sr)
        self.samplerate = self.tgt_sr if samplerate is None else int(samplerate)
        self.block_time, self.crossfade_time, self.extra_time = block_time, crossfade_time, extra_time
        self.threhold, self.rms_mix_rate, self.use_pv, self.f0method = threhold, float(rms_mix_rate), bool(use_pv), f0method
        self.protect = float(protect)
        if device is None:
            device = getattr(rvc, "device", None) or "cuda:0"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.RvcmiError("RealtimeBank runs on the GPU (got %s); there is no CPU fallback" % self.device)
        for k, v in stream_geometry(self.samplerate, block_time, crossfade_time, extra_time).items():
            setattr(self, k, v)
        S, f32 = self.S, torch.float32
        self.input_wav = torch.zeros(S, self.input_wav_len, device=self.device, dtype=f32)
        self.input_wav_res = torch.zeros(S, self.input_wav_res_len, device=self.device, dtype=f32)
        self.device_gate = _device_gate(device_gate, BANK_DEVICE_GATE)
        # the input gate's 4 zc samples of history per session: host rows with the host gate, a device tensor with the device gate
        self.rms_buffer = torch.zeros(S, 4 * self.zc, device=self.device, dtype=f32) if self.device_gate else np.zeros((S, 4 * self.zc), dtype="float32")
        self._gate_scratch = None
        self.sola_buffer = torch.zeros(S, self.sola_buffer_frame, device=self.device, dtype=f32)
        fade_in = torch.sin(0.5 * np.pi * torch.linspace(0.0, 1.0, steps=self.sola_buffer_frame, dtype=torch.float32)) ** 2   # gui.py:841-855
        self.fade_in_window = fade_in.to(self.device)
        self.fade_out_window = (1 - fade_in).to(self.device)
        self.resampler = SincResample(self.samplerate, 16000, self.device)
        self.resampler2 = SincResample(self.tgt_sr, self.samplerate, self.device) if self.tgt_sr != self.samplerate else None
        # gui.py:825, 835-836, per session: kept whatever the boxes say, updated only while they are ticked
        self.input_wav_denoise = torch.zeros_like(self.input_wav)
        self.nr_buffer = torch.zeros_like(self.sola_buffer)
        self.output_buffer = torch.zeros_like(self.input_wav)
        self.I_noise_reduce, self.O_noise_reduce = [False] * S, [False] * S
        self.tg = TorchGateHIP(sr=self.samplerate, n_fft=4 * self.zc, prop_decrease=0.9).to(self.device)   # gui.py:869-871
        self.gate_I = self.gate_O = None   # the boxes' TorchGateBank (spectrum cache + session states), made when a box is first ticked
        self._masks = {}
        self.keys = [getattr(rvc, "f0_up_key", 0)] * S
        self.sids = [0] * S
        self.formants = [0.0] * S
        # the GUI's hot-update sliders per session (gui.py:666-681); None follows the bank-wide value (rvc.index_rate, protect, rms_mix_rate, threhold)
        self.sliders = SessionSliders(S)
        self.vc = None            # the sessions' RealtimeVCBatch (pitch caches), made at the first block of a real rvc object
        self.last_offsets = None  # device int32 [S]

    def set_index_rate(self, i: int, rate) -> None:
        """Session ``i``'s ``index_rate`` (gui.py:676-679); ``None``: back to the bank-wide ``rvc.index_rate``.  Takes effect at the next block;
        ``reset(i)`` leaves it as it is, as it leaves the key.  A session blends iff there is an index and its rate is above 0."""
        self.sliders.set("index_rate", i, rate)

    def set_protect(self, i: int, protect) -> None:
        """Session ``i``'s ``protect`` (rtrvc.py:221-233); ``None``: back to the bank's ``protect``.  Applies iff below 0.5 and the model has f0."""
        self.sliders.set("protect", i, protect)

    def set_rms_mix_rate(self, i: int, rate) -> None:
        """Session ``i``'s ``rms_mix_rate`` (gui.py:1024-1056); ``None``: back to the bank-wide one.  The envelope mix runs for the sessions
        whose rate is below 1."""
        self.sliders.set("rms_mix_rate", i, rate)

    def set_threhold(self, i: int, db) -> None:
        """Session ``i``'s input-gate threshold in dB (gui.py:950-963); ``None``: back to the bank-wide one.  At or below -60 the session is
        not gated (and its ``rms_buffer`` row stays as it is, as the reference leaves it)."""
        self.sliders.set("threhold", i, db)

    def set_key(self, i: int, key) -> None:
        self.keys[int(i)] = key

    def set_sid(self, i: int, sid: int) -> None:
        self.sids[int(i)] = int(sid)

    def set_formant(self, i: int, shift: float) -> None:
        """Session ``i``'s formant shift in semitones (the GUI's slider, -2 .. 2); takes effect at the next block.  ``reset(i)`` leaves it
        as it is, as it leaves the key."""
        i = int(i)
        if not 0 <= i < self.S:
            raise IndexError("session %d of %d" % (i, self.S))
        if not math.isfinite(float(shift)):
            raise ValueError("formant shift must be finite (got %r)" % (shift,))
        self.formants[i] = shift

    def set_noise_reduce(self, i: int, I: Optional[bool] = None, O: Optional[bool] = None) -> None:
        """Session ``i``'s noise-reduction boxes (``None`` leaves a box as it is); takes effect at the next block.  A session whose box was
        not ticked in the previous block starts from a full transform of its noise buffer (cold); after that only the rewritten frames are."""
        i = int(i)
        if not 0 <= i < self.S:
            raise IndexError("session %d of %d" % (i, self.S))
        if I is not None:
            if I and self.block_frame < self.sola_buffer_frame:
                raise ValueError("the bank's input gate needs block_frame = %d >= sola_buffer_frame = %d (a block shorter than the cross-fade); "
                                 "use RealtimeStream" % (self.block_frame, self.sola_buffer_frame))
            self.I_noise_reduce[i] = bool(I)
            if I and self.gate_I is None:
                self.gate_I = TorchGateBank(self.tg, self.S, self.input_wav_len)
        if O is not None:
            self.O_noise_reduce[i] = bool(O)
            if O and self.gate_O is None:
                self.gate_O = TorchGateBank(self.tg, self.S, self.input_wav_len)

    def _mask(self, name: str, flags) -> torch.Tensor:
        """The device copy of a box's per-session flags (uint8 [S]), uploaded when they change."""
        host, t = self._masks.get(name, (None, None))
        if host != flags:
            host, t = list(flags), torch.tensor([1 if f else 0 for f in flags], dtype=torch.uint8, device=self.device)
            self._masks[name] = (host, t)
        return t

    def reset(self, i: int) -> None:
        """Session ``i``'s state back to zeros (a new talker takes the slot); the other sessions are not touched.  The session's
        noise-reduction boxes stay as they are; its cached noise spectra are dropped."""
        i = int(i)
        if not 0 <= i < self.S:
            raise IndexError("session %d of %d" % (i, self.S))
        for t in (self.input_wav, self.input_wav_res, self.sola_buffer, self.input_wav_denoise, self.nr_buffer, self.output_buffer):
            t[i].zero_()
        for g in (self.gate_I, self.gate_O):
            if g is not None:
                g.invalidate(i)
        self.rms_buffer[i] = 0   # (a host row or a device row)
        if self.vc is not None:
            self.vc.reset(i)

    def _infer(self) -> torch.Tensor:
        args = (self.input_wav_res, self.block_frame_16k, self.skip_head, self.return_length, self.f0method)
        sl, bank_rate = self.sliders, getattr(self.rvc, "index_rate", 0.0)
        if hasattr(self.rvc, "infer_batch"):
            fm = {"formants": list(self.formants)} if any(f != 0 for f in self.formants) else {}
            if sl.differs("index_rate", bank_rate):   # handed on only while some session differs, as formants= is
                fm["index_rates"] = sl.values("index_rate", bank_rate)
            if sl.differs("protect", self.protect):
                fm["protects"] = sl.values("protect", self.protect)
            return self.rvc.infer_batch(*args, keys=list(self.keys), sids=list(self.sids), **fm)
        if self.vc is None or self.vc.net_g is not self.rvc.net_g:
            if getattr(self.rvc, "formant_shift", 0) != 0:
                raise ValueError("a bank takes no bank-wide formant_shift (got %r on the rvc object): the formant shift is per session, "
                                 "set_formant(i, shift)" % (self.rvc.formant_shift,))
            self.vc = RealtimeVCBatch(self.rvc.net_g, self.S, index=getattr(self.rvc, "index", None), index_rate=self.rvc.index_rate,
                                      device=self.device, if_f0=self.rvc.if_f0, tgt_sr=self.tgt_sr, window=getattr(self.rvc, "window", 160))
        return rvc_infer_batch_hip(self.rvc, *args, protect=self.protect, keys=self.keys, sids=self.sids, rt=self.vc, formants=self.formants,
                                   index_rates=sl.own["index_rate"], protects=sl.own["protect"])

    def process(self, blocks) -> torch.Tensor:
        x = np.asarray(blocks, dtype=np.float32)
        if x.ndim != 2 or x.shape != (self.S, self.block_frame):
            raise ValueError("a bank block is [%d, %d] (sessions, samples), got %s" % (self.S, self.block_frame, x.shape))
        blk, blk16, zc = self.block_frame, self.block_frame_16k, self.zc
        # the threshold per session: None while every session follows the bank-wide one (then the step is the bank-wide one below), else
        # which sessions gate (threhold > -60, gui.py:950); a bank whose sessions differ but none of which gates is the ungated bank
        thr = self.sliders.values("threhold", self.threhold) if self.sliders.differs("threhold", self.threhold) else None
        gates = None if thr is None or not any(t > -60 for t in thr) else [t > -60 for t in thr]
        bank_gate = self.threhold > -60 if thr is None else False
        on_device = bank_gate and self.device_gate
        if bank_gate and not on_device:   # the host gate, per session (gui.py:950-963)
            x = np.stack([input_gate(x[s], self.rms_buffer[s], self.zc, self.threhold) for s in range(self.S)])
        elif gates is not None and not self.device_gate:   # ... with a threshold each: gated rows are blk + 2 zc samples, the others their raw blk
            rows = np.zeros((self.S, blk + 2 * zc), np.float32)
            for s in range(self.S):
                if gates[s]:
                    rows[s] = input_gate(x[s], self.rms_buffer[s], zc, thr[s])
                else:
                    rows[s, 2 * zc:] = x[s]
            x = rows
        m = blk + 2 * zc if (on_device or gates is not None) else int(x.shape[1])   # (with a mix of sessions: the gated ones' m)
        self.input_wav[:, :-blk] = self.input_wav[:, blk:].clone()
        xd = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)                       # the block's one host-to-device copy
        if on_device or (gates is not None and self.device_gate):
            # the raw block went up; the gate of all sessions writes the gated blk + 2 zc samples (three launches whatever S)
            if self._gate_scratch is None:
                self._gate_scratch = torch.empty(self.S * glue.input_gate_scratch_floats(zc, blk), device=self.device, dtype=torch.float32)
            if gates is None:
                glue.input_gate_batch(xd, self.rms_buffer, self.input_wav[:, -m:], zc, *input_gate_cutoffs(self.threhold), scratch=self._gate_scratch)
            else:   # a threshold each; a session that does not gate gets its raw blk samples and keeps its rms_buffer row
                glue.input_gate_sessions(xd, self.rms_buffer, self.input_wav[:, -m:], zc, thr, scratch=self._gate_scratch)
        elif gates is not None:   # gated on the host: blk + 2 zc samples for the gated sessions, the last blk for the others
            glue.masked_write_batch(self.input_wav, self._mask("gated", gates), xd, self.input_wav_len - m, xd[:, 2 * zc:], self.input_wav_len - blk)
        else:
            self.input_wav[:, -m:] = xd
        self.input_wav_res[:, :-blk16] = self.input_wav_res[:, blk16:].clone()
        Lb = self.sola_buffer_frame
        any_I, any_O = any(self.I_noise_reduce), any(self.O_noise_reduce)
        if self.gate_I is not None:                                                      # gui.py:974-992, the ticked sessions only
            den_prev = self.input_wav_denoise[:, blk:].clone() if any_I else None
            gated = self.gate_I.forward(self.input_wav[:, -Lb - blk:], self.input_wav, blk, m, self.I_noise_reduce)
        if any_I:
            mask_I = self.gate_I.mode
            glue.nr_stitch_batch(gated, self.nr_buffer, self.input_wav_denoise, self.fade_in_window, self.fade_out_window, blk, mask_I, den_prev=den_prev)
            # both resamples go to staging; each session's own range is written from its own source (the ranges differ when the host input
            # gate is on: m = blk + 2 zc)
            res_I = self.resampler.batch(self.input_wav_denoise[:, -blk - 2 * zc:])[:, 160:]
            res = self.resampler.batch(self.input_wav[:, -m - 2 * zc:])[:, 160:]
            n16 = self.input_wav_res_len
            if gates is None:
                glue.masked_write_batch(self.input_wav_res, mask_I, res_I, n16 - int(res_I.shape[1]), res, n16 - int(res.shape[1]))
            else:   # three ranges: the gated sessions' m + 2 zc, the ungated ones' blk + 2 zc, and over either the ticked sessions' denoised one
                res_u = self.resampler.batch(self.input_wav[:, -blk - 2 * zc:])[:, 160:]
                long_ = self._mask("gated_not_I", [g and not i for g, i in zip(gates, self.I_noise_reduce)])
                glue.masked_write_batch(self.input_wav_res, long_, res, n16 - int(res.shape[1]), res_u, n16 - int(res_u.shape[1]))
                glue.masked_write_batch(self.input_wav_res, mask_I, res_I, n16 - int(res_I.shape[1]))
        elif gates is not None:   # the 16 kHz range differs per session with m: both resamples, each session's own range written (also when every
            # session gates: the launches do not depend on which sessions do)
            res = self.resampler.batch(self.input_wav[:, -m - 2 * zc:])[:, 160:]
            res_u = self.resampler.batch(self.input_wav[:, -blk - 2 * zc:])[:, 160:]
            n16 = self.input_wav_res_len
            glue.masked_write_batch(self.input_wav_res, self._mask("gated", gates), res, n16 - int(res.shape[1]), res_u, n16 - int(res_u.shape[1]))
        else:
            self.input_wav_res[:, -160 * (m // zc + 1):] = self.resampler.batch(self.input_wav[:, -m - 2 * zc:])[:, 160:]
        infer_wav = self._infer()
        if infer_wav.dim() != 2 or infer_wav.shape[0] != self.S:
            raise ValueError("the model returned %s for %d sessions" % (tuple(infer_wav.shape), self.S))
        if infer_wav.dtype != torch.float32:
            infer_wav = infer_wav.float()
        if self.resampler2 is not None:
            infer_wav = self.resampler2.batch(infer_wav if infer_wav.stride(1) == 1 else infer_wav.contiguous())
        if not infer_wav.is_contiguous():
            infer_wav = infer_wav.contiguous()
        if any_O:                                                                        # gui.py:1015-1022, in place on the ticked sessions' rows
            n = int(infer_wav.shape[1])
            if n % zc or n < blk:
                raise ValueError("the bank's output gate needs a converted block of a whole number of hops (got %d samples, hop %d)" % (n, zc))
            rolled = torch.cat((self.output_buffer[:, blk:], infer_wav[:, -blk:]), 1)
            glue.masked_write_batch(self.output_buffer, self._mask("O", self.O_noise_reduce), rolled, 0)
        if self.gate_O is not None:
            self.gate_O.forward(infer_wav, self.output_buffer, blk, blk, self.O_noise_reduce, out=infer_wav if any_O else None)
        mix = self.sliders.values("rms_mix_rate", self.rms_mix_rate) if self.sliders.differs("rms_mix_rate", self.rms_mix_rate) else None
        if self.rms_mix_rate < 1 if mix is None else any(r < 1 for r in mix):
            n = int(infer_wav.shape[1])
            src = self.input_wav[:, self.extra_frame: self.extra_frame + n]
            if any_I:   # the envelope's source is per session: the denoised input where I is ticked
                src = src.clone()
                glue.masked_write_batch(src, mask_I, self.input_wav_denoise[:, self.extra_frame: self.extra_frame + n], 0)
            if mix is None:
                glue.envelope_mix_batch(src, infer_wav, zc, self.rms_mix_rate)
            else:   # a rate each: the sessions at 1 or above keep their rows
                glue.envelope_mix_sessions(src, infer_wav, zc, mix)
        out, self.last_offsets = glue.sola_batch(infer_wav, self.sola_buffer, self.fade_in_window, self.fade_out_window, blk,
                                                 self.sola_search_frame, use_pv=self.use_pv)
        return out
