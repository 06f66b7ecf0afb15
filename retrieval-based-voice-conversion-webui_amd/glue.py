"""Device-resident versions of the host-side glue of ``Pipeline.vc`` / ``Pipeline.pipeline`` (SURVEY.md section 8f
row 2), so that nothing between the PyTorch-ROCm feature extractors and ``net_g.infer`` has to visit the host:

    retrieve_blend_expand(feats, index, index_rate, pitchf, protect, p_len)   pipeline.py:118-159
    rmvpe_f0(salience, p_len, f0_up_key, thred)                               rvc/f0/rmvpe.py:115-164, f0.py:31-78, gen.py:10-41
    f0_post(f0, f0_up_key)                                                    rvc/f0/gen.py:10-41
    change_rms(audio16k, 16000, audio_opt, tgt_sr, rms_mix_rate)              pipeline.py:26-46,351
    scale_int16_range(audio)                                                  pipeline.py:355-359
    cut_points(audio64, window, t_center, t_query)                            pipeline.py:219-236
    filtfilt(x, b, a) / highpass16k(x)                                        pipeline.py:23,221 (scipy.signal.filtfilt)

and of the realtime GUI's block (gui.py:934-1090, assembled by ``realtime.RealtimeStream``):

    envelope_mix(input_wav, infer_wav, zc, rms_mix_rate)                      gui.py:1023-1056
    sola(infer_wav, sola_buffer, fade_in, fade_out, block, search, use_pv)    gui.py:1057-1090
    phase_vocoder(a, b, fade_out, fade_in)                                    gui.py:27-49
    spectral_gate(x, xn, n_fft, hop, window, smoothing_filter, ...)           torchgate.py (gui.py:974-992, 1015-1022)

and their forms for a bank of S realtime sessions (``realtime.RealtimeBank``; launch count independent of S).  The library has one
kernel and one launch recipe per step: a single-stream call above is the bank form at S = 1 with contiguous rows, so a session's
results are bit-equal to a single-stream call on its row:

    retrieve_blend_expand_batch(feats [S, nq, d], index, ..., skip_rows)       one search, the realtime guard per session
    sola_batch(infer_wav [S, n], sola_buffer [S, Lb], ...) / envelope_mix_batch(input_wav [S, .], infer_wav [S, n], zc, rate)
    spectral_gate_ring(x [S, n], xn [S, nn], shift, tail, ring, ring_base, mode, ...)   the gate over a rolling cache of noise spectra
    nr_stitch_batch(...) / masked_write_batch(...) / gate_ring_plan(nn, n_fft, hop, shift, tail)   per-session noise reduction (gate.TorchGateBank)
    rmvpe_f0_ragged(salience [R, 360], ((first_row, n, p_len, key), ...))     rmvpe_f0 of many packed sequences, a key each, in two launches
    input_gate_batch(block [S, blk], rms_buffer [S, 4 zc], dst [S, blk + 2 zc], zc, cut_a, cut_b)   the GUI's input gate (gui.py:950-963)
    retrieve_blend_expand_sessions(feats, index, index_rates, pitchf, protects, p_len, skip_rows) / envelope_mix_sessions(..., rates) /
    input_gate_sessions(..., threholds)                                        the same three with their control per session

All take and return CUDA (ROCm) tensors and enqueue on the current stream; a CPU tensor raises (no fallback).
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib


def _blend_expand_into(out: torch.Tensor, f: torch.Tensor, index, index_rate: float, pf: Optional[torch.Tensor], protect: float,
                       realtime_guard: bool) -> None:
    """out [p_len, d] (a contiguous row slice) <- x2(f [nq, d]), blended against ``index`` first when given, protect-mixed."""
    nq, d = int(f.shape[0]), int(f.shape[1])
    p_len = int(out.shape[0])
    dev = f.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        if index is not None and index_rate != 0:
            if d != index.d:
                raise ValueError("index mistatch")  # the reference's message (pipeline.py:128)
            if _lib.device_index(index.device) != _lib.device_index(dev):
                raise _lib.RvcmiError("the index lives on %s, the features on %s: read the index on the pipeline's device "
                                      "(read_index(path, device=...))" % (index.device, dev))
            index.reserve(nq)
            _lib.check(L.rvcmi_ivf_search_blend_expand(index._h, nq, _lib.ptr(f), float(index_rate), 8, 1 if realtime_guard else 0,
                                                       _lib.ptr(pf), float(protect), p_len, _lib.ptr(out), _lib.stream_ptr(dev)))
        else:
            _lib.check(L.rvcmi_glue_expand_protect(_lib.ptr(f), nq, d, 2, _lib.ptr(pf), float(protect), p_len, _lib.ptr(out), _lib.stream_ptr(dev)))


def retrieve_blend_expand(feats: torch.Tensor, index, index_rate: float, pitchf: Optional[torch.Tensor] = None,
                          protect: float = 0.5, p_len: Optional[int] = None, realtime_guard: bool = False,
                          skip_rows: int = 0) -> torch.Tensor:
    """``feats`` [1, nq, d] HuBERT features -> [1, p_len, d]: retrieval blend (when ``index`` is given and
    ``index_rate != 0``), x2 nearest interpolation, truncation to ``p_len`` and the protect mix
    (``pitchf`` [1, >= p_len], applied when ``protect < 0.5`` as in pipeline.py:153).

    ``skip_rows`` > 0 is the realtime form (rtrvc.py:167-185, 221-233): only ``feats[0][skip_rows:]`` is searched and
    blended (the rolling window's old frames keep their HuBERT features); the protect mix runs over all rows."""
    dev = _lib.on_gpu(feats, "feats")
    if feats.dim() != 3 or feats.shape[0] != 1:
        raise ValueError("feats must be [1, nq, d]")
    nq, d = int(feats.shape[1]), int(feats.shape[2])
    p_len = 2 * nq if p_len is None else min(int(p_len), 2 * nq)
    f = feats[0].to(torch.float32).contiguous()
    pf = None
    if pitchf is not None and protect < 0.5:
        pf = pitchf.reshape(-1)[:p_len].to(dev, torch.float32).contiguous()
        if pf.numel() < p_len:
            raise ValueError("pitchf has %d frames, p_len is %d" % (pf.numel(), p_len))
    out = torch.empty(p_len, d, device=dev, dtype=torch.float32)
    h = max(0, min(int(skip_rows), nq))
    if h and index is not None and index_rate != 0:
        # rows [0, h): un-blended (feats0 == feats in the protect mix); rows [h, nq): searched and blended
        head = min(2 * h, p_len)
        _blend_expand_into(out[:head], f[:h], None, 0.0, None if pf is None else pf[:head], protect, False)
        if head < p_len:
            _blend_expand_into(out[head:], f[h:], index, index_rate, None if pf is None else pf[head:], protect, realtime_guard)
    else:
        _blend_expand_into(out, f, index, index_rate, pf, protect, realtime_guard)
    return out.unsqueeze(0).to(feats.dtype)


def retrieve_blend_expand_batch(feats: torch.Tensor, index, index_rate: float, pitchf: Optional[torch.Tensor] = None,
                                protect: float = 0.5, p_len: Optional[int] = None, realtime_guard: bool = True,
                                skip_rows: int = 0) -> torch.Tensor:
    """``retrieve_blend_expand(..., skip_rows=...)`` for a bank of ``S`` realtime sessions: ``feats`` [S, nq, d] -> [S, p_len, d]
    (``pitchf`` [S, >= p_len], used when ``protect < 0.5``).  Row ``s`` equals the single-session call on ``feats[s:s+1]`` bit for
    bit, with one difference that is the point: the realtime guard is evaluated per session, so one talker whose frames probe a
    short list does not switch retrieval off for the others.  All ``S * (nq - skip_rows)`` searched rows go through one search;
    the launch count does not depend on ``S``."""
    dev = _lib.on_gpu(feats, "feats")
    if feats.dim() != 3 or feats.shape[0] < 1:
        raise ValueError("feats must be [S, nq, d] with S >= 1")
    S, nq, d = int(feats.shape[0]), int(feats.shape[1]), int(feats.shape[2])
    p_len = 2 * nq if p_len is None else min(int(p_len), 2 * nq)
    f = feats.to(torch.float32).contiguous()
    pf = None
    if pitchf is not None and protect < 0.5:
        if pitchf.dim() != 2 or pitchf.shape[0] != S or pitchf.shape[1] < p_len:
            raise ValueError("pitchf must be [%d, >= %d], got %s" % (S, p_len, tuple(pitchf.shape)))
        pf = pitchf[:, :p_len].to(dev, torch.float32).contiguous()
    out = torch.empty(S, p_len, d, device=dev, dtype=torch.float32)
    h = max(0, min(int(skip_rows), nq))
    L = _lib.lib()
    with torch.cuda.device(dev):
        if index is not None and index_rate != 0:
            if d != index.d:
                raise ValueError("index mistatch")  # the reference's message (pipeline.py:128)
            if _lib.device_index(index.device) != _lib.device_index(dev):
                raise _lib.RvcmiError("the index lives on %s, the features on %s: read the index on the pipeline's device "
                                      "(read_index(path, device=...))" % (index.device, dev))
            index.reserve(S * (nq - h))
            _lib.check(L.rvcmi_ivf_search_blend_expand_batch(index._h, S, nq, h, _lib.ptr(f), float(index_rate), 8, 1 if realtime_guard else 0,
                                                             _lib.ptr(pf), float(protect), p_len, _lib.ptr(out), _lib.stream_ptr(dev)))
        else:
            _lib.check(L.rvcmi_glue_expand_protect_batch(S, _lib.ptr(f), nq, d, 2, _lib.ptr(pf), float(protect), p_len, _lib.ptr(out),
                                                         _lib.stream_ptr(dev)))
    return out.to(feats.dtype)


def rmvpe_f0(salience: torch.Tensor, p_len: int, f0_up_key=0, thred: float = 0.03) -> Tuple[torch.Tensor, torch.Tensor]:
    """RMVPE salience [n, 360] -> (pitch int64 [1, p_len], pitchf float32 [1, p_len]) as ``Generator.calculate`` +
    pipeline.py:270-277 produce them.  ``f0_up_key``: an int or a float (the realtime GUI's key minus its formant shift); the factor is
    ``pow(2, f0_up_key / 12)`` in fp64 either way, as in rvc/f0/gen.py:18."""
    dev = _lib.on_gpu(salience, "salience")
    if salience.dim() != 2:
        raise ValueError("salience must be [n, bins]")
    open_blocks = getattr(_F0_GATHER, "blocks", None)
    if open_blocks:   # inside ``with _f0_gather(...)`` (this thread's): rows of its packed salience are noted, decoded when the block ends
        got = open_blocks[-1].add(salience, p_len, f0_up_key, thred)
        if got is not None:
            return got
    s = salience.to(torch.float32).contiguous()
    n, nb = int(s.shape[0]), int(s.shape[1])
    scratch = torch.empty(n, device=dev, dtype=torch.float64)
    pitch = torch.empty(int(p_len), device=dev, dtype=torch.int64)
    pitchf = torch.empty(int(p_len), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_rmvpe_f0_key(_lib.ptr(s), n, nb, float(thred), int(p_len), float(f0_up_key), _lib.ptr(scratch), _lib.ptr(pitch),
                                                      _lib.ptr(pitchf), _lib.stream_ptr(dev)))
    return pitch.unsqueeze(0), pitchf.unsqueeze(0)


_F0_ROWS: dict = {}     # (device index, rows) -> (host descriptors, their device copy, total p_len): kept until the tuple of rows changes
_F0_ROWS_KEEP = 8       # distinct row tuples remembered (a bank's step, a folder's batch); the oldest goes first
f0_rows_uploads = 0     # how often descriptors went to the device (tests read it)


def f0_rows(rows, dev):
    """The descriptors of ``rmvpe_f0_ragged`` for ``rows`` = ((first_row, n, p_len, key), ...): -> (host array of ``rvcmi_f0_row``, the same
    bytes on ``dev``, total output length).  Item ``i``'s output starts at the sum of the ``p_len`` before it; its factor is
    ``rvcmi_glue_f0_key_mul(key)``, the double the single entry uses.  Cached per tuple of rows: an unchanged bank step uploads nothing."""
    global f0_rows_uploads
    key = (_lib.device_index(dev), tuple((int(r), int(n), int(p), float(k)) for r, n, p, k in rows))
    hit = _F0_ROWS.get(key)
    if hit is None:
        L = _lib.lib()
        desc, off = (_lib.F0Row * len(key[1]))(), 0
        for d, (r, n, p, k) in zip(desc, key[1]):
            d.out_off, d.key_mul, d.first_row, d.n, d.p_len = off, L.rvcmi_glue_f0_key_mul(k), r, n, p
            off += max(p, 0)
        raw = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8) if len(desc) else torch.zeros(0, dtype=torch.uint8)
        while len(_F0_ROWS) >= _F0_ROWS_KEEP:
            _F0_ROWS.pop(next(iter(_F0_ROWS)))
        hit = _F0_ROWS[key] = (desc, raw.to(dev), off)
        f0_rows_uploads += 1
    return hit


def rmvpe_f0_ragged_packed(salience: torch.Tensor, rows, thred: float = 0.03, out=None):
    """``rmvpe_f0_ragged`` without the views: -> (pitch int64 [sum p_len], pitchf float32 [sum p_len]), item ``i`` behind the items before it.
    ``out``: a (pitch, pitchf) pair of contiguous device tensors of exactly that length to write into."""
    dev = _lib.on_gpu(salience, "salience")
    if salience.dim() != 2 or salience.dtype != torch.float32 or not salience.is_contiguous():
        raise ValueError("salience must be a contiguous float32 tensor [R, bins]")
    rows = list(rows)
    R, nb = int(salience.shape[0]), int(salience.shape[1])
    desc, desc_dev, total = f0_rows(rows, dev)
    scratch = torch.empty(max(R, 1), device=dev, dtype=torch.float64)
    if out is None:
        pitch = torch.empty(max(total, 1), device=dev, dtype=torch.int64)
        pitchf = torch.empty(max(total, 1), device=dev, dtype=torch.float32)
    else:
        pitch, pitchf = out
        if (pitch.dtype != torch.int64 or pitchf.dtype != torch.float32 or pitch.device != dev or pitchf.device != dev or pitch.dim() != 1 or pitchf.dim() != 1
                or pitch.numel() != total or pitchf.numel() != total or not pitch.is_contiguous() or not pitchf.is_contiguous() or total < 1):
            raise ValueError("out must be (int64 [%d], float32 [%d]) contiguous on %s" % (total, total, dev))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_rmvpe_f0_ragged(_lib.ptr(salience), R, nb, len(rows), C.cast(desc, C.c_void_p), _lib.ptr(desc_dev), float(thred),
                                                         _lib.ptr(scratch), _lib.ptr(pitch), _lib.ptr(pitchf), total, _lib.stream_ptr(dev)))
    return pitch[:total], pitchf[:total]


def rmvpe_f0_ragged(salience: torch.Tensor, rows, thred: float = 0.03):
    """``rmvpe_f0`` for many sequences whose salience rows lie packed in ``salience`` [R, 360] (contiguous float32), in TWO launches whatever
    their number: ``rows`` is a sequence of ``(first_row, n, p_len, key)``.  -> a list of ``(pitch int64 [1, p_len_i], pitchf float32
    [1, p_len_i])``, views of two packed tensors; item ``i`` equals ``rmvpe_f0(salience[first_row : first_row + n], p_len, key, thred)``
    bit for bit.  Rows between items are allowed; items must not share rows (``RvcmiError`` with ``ERR_INVALID``, as for ``p_len < 1`` or
    a key that is not finite, before anything is launched)."""
    rows = list(rows)
    pitch, pitchf = rmvpe_f0_ragged_packed(salience, rows, thred)
    out, off = [], 0
    for _, _, p, _ in rows:
        out.append((pitch[off: off + int(p)].unsqueeze(0), pitchf[off: off + int(p)].unsqueeze(0)))
        off += int(p)
    return out


_F0_GATHER = threading.local()   # .blocks: this thread's open _f0_gather blocks, innermost last


class _f0_gather:
    """Private to the package (``rvc_infer_batch_hip``): ``rmvpe_f0`` calls of one block, decoded together:

        with glue._f0_gather(salience_packed, total_p_len, thred) as g:
            pairs = [glue.rmvpe_f0(salience_packed[r: r + n], p_len, key, thred) for r, n, p_len, key in ...]   # nothing is launched here
        g.pitch, g.pitchf                                                   # packed [total_p_len], filled by ONE rmvpe_f0_ragged call

    Inside the block a ``rmvpe_f0`` call whose salience is a run of whole rows of ``salience_packed`` (a view of it, same ``thred``) launches
    nothing: it is noted as an item and gets views of the packed outputs, which the two launches at the end of the block fill -- item for
    item the bits the call alone would have produced.  UNTIL THE BLOCK EXITS THE RETURNED VIEWS ARE UNDEFINED (nothing has written them yet):
    the caller must not read them inside the block, and after an exception they are never filled.  Any other ``rmvpe_f0`` call inside the block runs at once, as outside.  The caller
    keeps calling ``rmvpe_f0`` per sequence, each with its own key, and the launch count does not depend on how many there are."""

    def __init__(self, salience: torch.Tensor, total_p_len: int, thred: float = 0.03):
        _lib.on_gpu(salience, "salience")
        if salience.dim() != 2 or salience.dtype != torch.float32 or not salience.is_contiguous():
            raise ValueError("salience must be a contiguous float32 tensor [R, bins]")
        self.salience, self.thred, self.total = salience, float(thred), int(total_p_len)
        self.pitch = torch.empty(max(self.total, 1), device=salience.device, dtype=torch.int64)[: self.total]
        self.pitchf = torch.empty(max(self.total, 1), device=salience.device, dtype=torch.float32)[: self.total]
        self.rows, self.used = [], 0

    def add(self, sal: torch.Tensor, p_len: int, key, thred: float):
        """-> views of the packed outputs for this item, or None when ``sal`` is not a run of rows of the packed salience."""
        base, nb = self.salience, int(self.salience.shape[1])
        off = sal.storage_offset() - base.storage_offset()
        if (sal.dtype != torch.float32 or sal.device != base.device or sal.untyped_storage().data_ptr() != base.untyped_storage().data_ptr()
                or not sal.is_contiguous() or sal.shape[1] != nb or sal.shape[0] < 1 or off < 0 or off % nb
                or off // nb + sal.shape[0] > base.shape[0] or float(thred) != self.thred):
            return None
        p_len = int(p_len)
        if p_len < 1 or self.used + p_len > self.total:
            raise ValueError("_f0_gather: %d output frames were announced, item %d asks for %d more than are left" % (self.total, len(self.rows), p_len))
        self.rows.append((off // nb, int(sal.shape[0]), p_len, float(key)))
        lo, self.used = self.used, self.used + p_len
        return self.pitch[lo: lo + p_len].unsqueeze(0), self.pitchf[lo: lo + p_len].unsqueeze(0)

    def __enter__(self):
        if not hasattr(_F0_GATHER, "blocks"):
            _F0_GATHER.blocks = []
        _F0_GATHER.blocks.append(self)
        return self

    def __exit__(self, exc_type, exc, tb):
        _F0_GATHER.blocks.remove(self)
        if exc_type is None and self.rows:
            rmvpe_f0_ragged_packed(self.salience, self.rows, self.thred, out=(self.pitch, self.pitchf))
        return False


def f0_post(f0: torch.Tensor, f0_up_key=0) -> Tuple[torch.Tensor, torch.Tensor]:
    """f0 in Hz [n] (any estimator) -> (pitch int64 [1, n], pitchf float32 [1, n]): rvc/f0/gen.py post_process (``f0_up_key``: int or float)."""
    dev = _lib.on_gpu(f0, "f0")
    x = f0.reshape(-1).to(torch.float64).contiguous()
    n = int(x.numel())
    pitch = torch.empty(n, device=dev, dtype=torch.int64)
    pitchf = torch.empty(n, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_f0_post_key(_lib.ptr(x), n, float(f0_up_key), _lib.ptr(pitch), _lib.ptr(pitchf), _lib.stream_ptr(dev)))
    return pitch.unsqueeze(0), pitchf.unsqueeze(0)


def change_rms(data1: torch.Tensor, sr1: int, data2: torch.Tensor, sr2: int, rate: float) -> torch.Tensor:
    """``change_rms(audio, 16000, audio_opt, tgt_sr, rms_mix_rate)`` of pipeline.py:26-46,351 on the device, IN PLACE on
    ``data2`` (returned): ``data2 *= rms1**(1-rate) * max(rms2, 1e-6)**(rate-1)`` with half-second frame RMS envelopes."""
    dev = _lib.on_gpu(data2, "data2")
    for t, nm in ((data1, "data1"), (data2, "data2")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 1 or t.device != dev:
            raise ValueError("%s must be a contiguous 1-D float32 tensor on %s" % (nm, dev))
    n1, n2 = int(data1.numel()), int(data2.numel())
    scratch = torch.empty(2 + n1 // (int(sr1) // 2) + n2 // (int(sr2) // 2), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_change_rms(_lib.ptr(data1), n1, int(sr1), _lib.ptr(data2), n2, int(sr2), float(rate), _lib.ptr(scratch),
                                                    _lib.stream_ptr(dev)))
    return data2


def cut_count(n: int, t_center: int) -> int:
    """How many cuts an input of ``n`` samples gets: ``len(range(t_center, n, t_center))`` (pipeline.py:228)."""
    return len(range(int(t_center), int(n), int(t_center)))


def cut_points(audio: torch.Tensor, window: int, t_center: int, t_query: int, return_sums: bool = False):
    """The quiet-point search of pipeline.py:219-236 on the device: ``audio`` [n] float64 (the ``filtfilt`` output) -> int64 tensor
    ``[cut_count(n, t_center)]``, ``cut = t - t_query + first argmin of audio_sum[t - t_query : t + t_query]`` for every multiple
    ``t`` of ``t_center`` below ``n``; the window sums are numpy's, bit for bit (include/rvcmi.h).  ``return_sums=True`` also
    returns them as ``[cuts, 2 t_query]`` float64, NaN where a search window runs past the end of the signal.  A tensor that is
    not float64 raises ``TypeError``: a cast would change the sums.  Enqueue-only; the caller reads the cuts back."""
    if audio.dtype != torch.float64:
        raise TypeError("audio must be float64 (got %s): the sums are defined on the float64 signal" % audio.dtype)
    dev = _lib.on_gpu(audio, "audio")
    if audio.dim() != 1 or not audio.is_contiguous():
        raise ValueError("audio must be a contiguous 1-D tensor")
    n, window, t_center, t_query = int(audio.numel()), int(window), int(t_center), int(t_query)
    L = _lib.lib()
    ncuts = cut_count(n, t_center) if t_center > 0 else 0
    nbytes = int(L.rvcmi_glue_cut_points_scratch_bytes(n, window, t_center, t_query))
    cuts = torch.empty(ncuts, device=dev, dtype=torch.int64)
    sums = torch.full((ncuts, 2 * max(t_query, 0)), float("nan"), device=dev, dtype=torch.float64) if return_sums else None
    scratch = torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(L.rvcmi_glue_cut_points(_lib.ptr(audio), n, window, t_center, t_query, _lib.ptr(cuts), ncuts, _lib.ptr(sums), _lib.ptr(scratch),
                                           _lib.stream_ptr(dev)))
    return (cuts, sums) if return_sums else cuts


# ---- scipy.signal.filtfilt on the device (csrc/filt_kernels.hpp) ---------------------------------------------------------------------
FILT_MAX_ORDER = 8
FILT_LANE = 1024            # outputs per thread of a pass (csrc/filt_kernels.hpp FILT_LANE)
FILT_WARMUP_CAP = 1 << 16   # samples; a filter whose poles ask for a longer warm-up is refused (see filt_warmup)
# scipy.signal.butter(N=5, Wn=48, btype="high", fs=16000) (pipeline.py:23) as scipy 1.15 gives it; used by highpass16k only when
# neither the reference module nor scipy is there to ask
_HP16K = (tuple(float.fromhex(h) for h in ("0x1.f09eae82f17f2p-1", "-0x1.36632d11d6ef7p+2", "0x1.36632d11d6ef7p+3", "-0x1.36632d11d6ef7p+3",
                                            "0x1.36632d11d6ef7p+2", "-0x1.f09eae82f17f2p-1")),
          tuple(float.fromhex(h) for h in ("0x1.0000000000000p+0", "-0x1.3c189b160d9bbp+2", "0x1.38406b02c5ae9p+3", "-0x1.347726c291cb2p+3",
                                            "0x1.30bc870194e75p+2", "-0x1.e1b3a34ba432ap-1")))
_FILT_PLANS: dict = {}


def _normalized_ba(b, a):
    """``b``, ``a`` as ``lfilter`` / ``lfilter_zi`` see them: 1-D float64, leading zeros of ``a`` dropped, divided by ``a[0]``,
    zero-padded to one length.  scipy's own ValueErrors for what it refuses."""
    b = np.atleast_1d(np.asarray(b, dtype=np.float64))
    a = np.atleast_1d(np.asarray(a, dtype=np.float64))
    if b.ndim != 1:
        raise ValueError("Numerator b must be 1-D.")
    if a.ndim != 1:
        raise ValueError("Denominator a must be 1-D.")
    while len(a) > 1 and a[0] == 0.0:
        a = a[1:]
    if a.size < 1 or a[0] == 0.0:
        raise ValueError("There must be at least one nonzero `a` coefficient.")
    if a[0] != 1.0:
        b = b / a[0]
        a = a / a[0]
    n = max(len(a), len(b))
    if len(a) < n:
        a = np.r_[a, np.zeros(n - len(a))]
    elif len(b) < n:
        b = np.r_[b, np.zeros(n - len(b))]
    return b, a


def lfilter_zi(b, a) -> np.ndarray:
    """``scipy.signal.lfilter_zi(b, a)`` in numpy, the same arithmetic and therefore the same bits: the steady state of the step
    response, ``(I - companion(a).T) zi = b[1:] - a[1:] b[0]``, solved by ``np.linalg.solve`` as scipy does (its explicit
    running-sum formulas give the same numbers to a few ulp, not the same bits)."""
    b, a = _normalized_ba(b, a)
    n = len(a)
    if n < 2:
        return np.zeros(0)
    comp = np.zeros((n - 1, n - 1))  # scipy.linalg.companion(a): first row -a[1:] / a[0], ones on the sub-diagonal
    comp[0, :] = -a[1:] / (1.0 * a[0])
    comp[np.arange(1, n - 1), np.arange(0, n - 2)] = 1.0
    return np.linalg.solve(np.eye(n - 1) - comp.T, b[1:] - a[1:] * b[0])


def filt_warmup(a) -> int:
    """Samples a thread of the device filter runs before its first stored output, derived from the poles (never a constant).

    The state of direct form II transposed obeys ``z[n + 1] = A z[n] + B x[n]`` with ``A = companion(a).T``, so two runs over the
    same input whose states differ by ``e`` at sample ``s`` differ by ``A^W e = V diag(lambda^W) V^-1 e`` after ``W`` more samples:
    at most ``cond(V) rho^W |e|`` in the 2-norm, ``rho`` the largest pole radius and ``V`` the eigenvectors of ``A``.  A thread
    starts from the steady state of a constant input instead of the true state; ``W`` is the smallest multiple of ``FILT_LANE`` with

        cond(V) * rho ** W < 2 ** -64,

    i.e. what is left of that start is 2^-11 of ONE rounding error of a state of its own size, far below the rounding noise the
    recurrence itself accumulates (which the poles amplify by about cond(V)).  For the pipeline's high-pass (rho = 0.99419, cond(V) =
    9.2e8) the bound asks for 11 161 samples, W = 11 264.  ``RvcmiError`` when the filter is unstable (rho >= 1), has a defective
    pole set, or W would exceed ``FILT_WARMUP_CAP`` = 65 536 samples (rho above about 0.9992): a thread would spend its time warming up."""
    a = _normalized_ba([1.0], a)[1]
    while len(a) > 1 and a[-1] == 0.0:  # trailing zeros are poles at the origin: they decay in one step each
        a = a[:-1]
    m = len(a) - 1
    if m < 1:
        return 0
    comp = np.zeros((m, m))
    comp[0, :] = -a[1:]
    comp[np.arange(1, m), np.arange(0, m - 1)] = 1.0
    lam, V = np.linalg.eig(comp.T)
    rho = float(np.abs(lam).max())
    cond = float(np.linalg.cond(V))
    if not (rho < 1.0) or not np.isfinite(cond):
        raise _lib.RvcmiError("filtfilt: the filter is not strictly stable (largest pole radius %.6g, cond(V) %.3g)" % (rho, cond), code=_lib.ERR_INVALID)
    if rho == 0.0:
        return FILT_LANE
    need = (64.0 * np.log(2.0) + np.log(cond)) / -np.log(rho)
    W = int(-(-need // FILT_LANE)) * FILT_LANE
    if not W <= FILT_WARMUP_CAP:
        raise _lib.RvcmiError("filtfilt: largest pole radius %.9g with cond(V) = %.3g needs a warm-up of %.0f samples per thread, above the "
                              "cap of %d" % (rho, cond, need, FILT_WARMUP_CAP), code=_lib.ERR_INVALID)
    return max(W, FILT_LANE)


def _filt_plan(b, a):
    """-> (b, a normalised [order + 1] float64, zi [order], order, padlen, warm-up); cached per coefficient set."""
    b, a = _normalized_ba(b, a)
    key = (b.tobytes(), a.tobytes())
    hit = _FILT_PLANS.get(key)
    if hit is None:
        order = len(a) - 1
        if not 1 <= order <= FILT_MAX_ORDER:
            raise _lib.RvcmiError("filtfilt: filter order %d; the kernel serves 1 .. %d" % (order, FILT_MAX_ORDER), code=_lib.ERR_INVALID)
        hit = (np.ascontiguousarray(b), np.ascontiguousarray(a), np.ascontiguousarray(lfilter_zi(b, a)), order, 3 * (order + 1), filt_warmup(a))
        if len(_FILT_PLANS) > 64:
            _FILT_PLANS.clear()
        _FILT_PLANS[key] = hit
    return hit


def filtfilt_exact_len(b, a) -> int:
    """The longest input ``filtfilt`` computes from scipy's own initial state in every thread, i.e. BIT-equal to
    ``scipy.signal.filtfilt``: ``n + 2 padlen <= warm-up + FILT_LANE``."""
    plan = _filt_plan(b, a)
    return plan[5] + FILT_LANE - 2 * plan[4]


def filtfilt_flat(flat: torch.Tensor, lengths, b, a, reflect_pad: int = 0):
    """``filtfilt`` for a ragged batch that already lies in one flat device buffer: ``flat`` 1-D float32 or float64, item ``i`` =
    the next ``lengths[i]`` samples.  -> list of float64 views (one per item) into one output buffer; with ``reflect_pad`` > 0 a
    second list, ``np.pad(out_i, reflect_pad, mode="reflect")`` per item (every item must be longer than the pad).  One call:
    two launches, whatever the number of items."""
    if flat.dtype not in (torch.float32, torch.float64):
        raise TypeError("x must be float32 or float64 (got %s)" % flat.dtype)
    if flat.dim() != 1 or not flat.is_contiguous():
        raise ValueError("x must be a contiguous 1-D tensor")
    lengths = [int(n) for n in lengths]
    bn, an, zi, order, padlen, warm = _filt_plan(b, a)
    pad = int(reflect_pad)
    if not lengths or sum(lengths) != int(flat.numel()):
        raise ValueError("lengths %s do not add up to the %d samples of x" % (lengths[:8], int(flat.numel())))
    for n in lengths:
        if n <= padlen:  # scipy's message (signal/_signaltools.py _validate_pad)
            raise ValueError("The length of the input vector x must be greater than padlen, which is %d." % padlen)
        if pad < 0 or (pad and n <= pad):
            raise ValueError("reflect_pad = %d needs every item longer than it (got %d samples)" % (pad, n))
    dev = _lib.on_gpu(flat, "x")  # (after the argument checks: they are scipy's and need no GPU)
    B, total, max_len = len(lengths), int(flat.numel()), max(lengths)
    L = _lib.lib()
    nbytes = int(L.rvcmi_glue_filtfilt_scratch_bytes(B, total, order))
    if nbytes == 0:
        raise _lib.RvcmiError("filtfilt: a batch of %d items / %d samples is out of range" % (B, total), code=_lib.ERR_INVALID)
    starts = [0]
    for n in lengths:
        starts.append(starts[-1] + n)
    offsets = torch.tensor(starts, dtype=torch.int64).to(dev)
    out = torch.empty(total, device=dev, dtype=torch.float64)
    out_pad = torch.empty(total + 2 * pad * B, device=dev, dtype=torch.float64) if pad else None
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    dptr = lambda v: v.ctypes.data_as(C.c_void_p)  # noqa: E731
    with torch.cuda.device(dev):
        _lib.check(L.rvcmi_glue_filtfilt(_lib.ptr(flat), 1 if flat.dtype == torch.float64 else 0, _lib.ptr(offsets), B, max_len, total, dptr(bn), dptr(an),
                                         dptr(zi), order, warm, _lib.ptr(out), _lib.ptr(out_pad), pad, _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev)))
    outs = [out[starts[i]: starts[i + 1]] for i in range(B)]
    if not pad:
        return outs
    return outs, [out_pad[starts[i] + 2 * pad * i: starts[i + 1] + 2 * pad * (i + 1)] for i in range(B)]


def filtfilt(x, b, a, reflect_pad: int = 0):
    """``scipy.signal.filtfilt(b, a, x)`` with scipy's defaults (odd extension by ``padlen = 3 max(len(a), len(b))``, both passes
    from ``lfilter_zi(b, a) * first sample``, direct form II transposed in fp64) on the device.  ``x``: a 1-D float32 or float64
    device tensor, or a list of them (a ragged batch, one call; item ``i`` is computed exactly as a call with it alone) -> float64
    tensor(s).  ``reflect_pad`` > 0 also returns ``np.pad(result, reflect_pad, mode="reflect")``: ``(y, y_padded)``.

    An input of at most ``filtfilt_exact_len(b, a)`` samples equals scipy bit for bit.  A longer one is computed by independent
    threads, each warmed up over ``filt_warmup(a)`` samples, and differs from scipy as two fp64 evaluations of an ill-conditioned
    recurrence do: for the pipeline's high-pass both are about 3e-8 (signal peak 0.5) from the exact result.
    ``ValueError`` for an input not longer than ``padlen`` (scipy's), ``RvcmiError`` for a filter order above 8 or poles so close to
    the unit circle that the warm-up would exceed ``FILT_WARMUP_CAP``.  zi is computed here on the host; scipy is not needed."""
    single = isinstance(x, torch.Tensor)
    xs = [x] if single else list(x)
    if not xs:
        raise ValueError("no input")
    for t in xs:
        if t.dim() != 1:
            raise ValueError("x must be 1-D (got shape %s)" % (tuple(t.shape),))
        if t.dtype != xs[0].dtype or t.device != xs[0].device:
            raise ValueError("the items of a batch must share dtype and device")
    flat = xs[0].contiguous() if len(xs) == 1 else torch.cat(xs)
    got = filtfilt_flat(flat, [int(t.numel()) for t in xs], b, a, reflect_pad)
    if not reflect_pad:
        return got[0] if single else got
    return (got[0][0], got[1][0]) if single else got


def highpass_coefficients(ref_module=None):
    """``bh, ah`` of the pipeline's input high-pass (pipeline.py:23: ``signal.butter(N=5, Wn=48, btype="high", fs=16000)``): the
    reference module's own when it is bound (``ref_module``, or ``infer.modules.vc.pipeline`` if imported), else computed by scipy,
    else -- no scipy -- the stored fp64 values of that call."""
    import sys

    mod = ref_module if ref_module is not None else sys.modules.get("infer.modules.vc.pipeline")
    if mod is not None and hasattr(mod, "bh") and hasattr(mod, "ah"):
        return np.asarray(mod.bh, dtype=np.float64), np.asarray(mod.ah, dtype=np.float64)
    try:
        from scipy import signal
    except ImportError:
        return np.array(_HP16K[0]), np.array(_HP16K[1])
    return signal.butter(N=5, Wn=48, btype="high", fs=16000)


def highpass16k(x, reflect_pad: int = 0, ref_module=None):
    """The input preparation of ``Pipeline.pipeline`` (pipeline.py:221): ``filtfilt(bh, ah, x)`` on the device (see ``filtfilt``)."""
    bh, ah = highpass_coefficients(ref_module)
    return filtfilt(x, bh, ah, reflect_pad)


def scale_int16_range(audio: torch.Tensor) -> torch.Tensor:
    """In place: ``audio *= 32768 / max(1, |audio|.max() / 0.99)`` (pipeline.py:355-359); returns ``audio``."""
    dev = _lib.on_gpu(audio, "audio")
    if audio.dtype != torch.float32 or not audio.is_contiguous():
        raise ValueError("audio must be a contiguous float32 tensor")
    scratch = torch.empty(256, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_scale_int16_range(_lib.ptr(audio), audio.numel(), _lib.ptr(scratch), _lib.stream_ptr(dev)))
    return audio


def sola(infer_wav: torch.Tensor, sola_buffer: torch.Tensor, fade_in: torch.Tensor, fade_out: torch.Tensor, block_frame: int,
         search_frame: int, return_offset: bool = False, use_pv: bool = False):
    """The SOLA stitch of gui.py:1057-1090 in one launch: returns the ``block_frame`` output samples and updates
    ``sola_buffer`` in place (``return_offset=True`` also returns the chosen offset as a 1-element int32 tensor).
    ``use_pv=True`` is the GUI's phase-vocoder branch (gui.py:1081-1087): the same search, then the ``len(sola_buffer)``
    samples at the offset are cross-faded by ``phase_vocoder`` (four launches; the offset never leaves the device)."""
    dev = _lib.on_gpu(infer_wav, "infer_wav")
    for t, nm in ((infer_wav, "infer_wav"), (sola_buffer, "sola_buffer"), (fade_in, "fade_in"), (fade_out, "fade_out")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError("%s must be a contiguous float32 tensor on %s" % (nm, dev))
    Lb = int(sola_buffer.numel())
    out = torch.empty(int(block_frame), device=dev, dtype=torch.float32)
    off = torch.empty(1, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        if use_pv:
            scratch = torch.empty(3 * (Lb // 2 + 1) + Lb // 2 + 1, device=dev, dtype=torch.float64)
            _lib.check(_lib.lib().rvcmi_glue_sola_pv(_lib.ptr(infer_wav), infer_wav.numel(), _lib.ptr(sola_buffer), Lb, int(search_frame), _lib.ptr(fade_in),
                                                     _lib.ptr(fade_out), int(block_frame), _lib.ptr(out), _lib.ptr(off), _lib.ptr(scratch), _lib.stream_ptr(dev)))
        else:
            _lib.check(_lib.lib().rvcmi_glue_sola(_lib.ptr(infer_wav), infer_wav.numel(), _lib.ptr(sola_buffer), Lb, int(search_frame), _lib.ptr(fade_in),
                                                  _lib.ptr(fade_out), int(block_frame), _lib.ptr(out), _lib.ptr(off), _lib.stream_ptr(dev)))
    return (out, off) if return_offset else out


def bank_rows(t: torch.Tensor, name: str, dev=None):
    """``t`` as the batched block DSP takes a per-session array: 2-D float32 on the GPU, unit stride along a row; the rows may be
    slices of longer rolling buffers (row stride >= row length, which any such view has).  -> (S, row length, row stride)."""
    if t.dim() != 2 or t.dtype != torch.float32 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError("%s must be a 2-D float32 tensor [S, n] with contiguous rows" % name)
    if dev is not None and t.device != dev:
        raise ValueError("%s must live on %s" % (name, dev))
    if t.shape[0] < 1:
        raise ValueError("%s: a bank has at least one session (got S = 0)" % name)
    return int(t.shape[0]), int(t.shape[1]), int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def sola_batch(infer_wav: torch.Tensor, sola_buffer: torch.Tensor, fade_in: torch.Tensor, fade_out: torch.Tensor, block_frame: int,
               search_frame: int, use_pv: bool = False):
    """``sola`` for a bank: ``infer_wav`` [S, n] and ``sola_buffer`` [S, Lb] (updated in place), rows of either may be views into
    longer buffers.  -> (out [S, block_frame], offsets int32 [S]); session ``s`` equals ``sola`` on its rows bit for bit.  One
    launch (four with ``use_pv``) whatever ``S``."""
    dev = _lib.on_gpu(infer_wav, "infer_wav")
    S, n, ws = bank_rows(infer_wav, "infer_wav")
    Sb, Lb, bs = bank_rows(sola_buffer, "sola_buffer", dev)
    if Sb != S:
        raise ValueError("infer_wav has %d sessions, sola_buffer %d" % (S, Sb))
    for t, nm in ((fade_in, "fade_in"), (fade_out, "fade_out")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() != Lb:
            raise ValueError("%s must be a contiguous float32 tensor of %d samples on %s" % (nm, Lb, dev))
    out = torch.empty(S, int(block_frame), device=dev, dtype=torch.float32)
    off = torch.empty(S, device=dev, dtype=torch.int32)
    L = _lib.lib()
    with torch.cuda.device(dev):
        if use_pv:
            scratch = torch.empty(S * (3 * (Lb // 2 + 1) + Lb // 2 + 1), device=dev, dtype=torch.float64)
            _lib.check(L.rvcmi_glue_sola_pv_batch(S, _lib.ptr(infer_wav), ws, n, _lib.ptr(sola_buffer), bs, Lb, int(search_frame), _lib.ptr(fade_in),
                                                  _lib.ptr(fade_out), int(block_frame), _lib.ptr(out), int(block_frame), _lib.ptr(off), _lib.ptr(scratch),
                                                  _lib.stream_ptr(dev)))
        else:
            _lib.check(L.rvcmi_glue_sola_batch(S, _lib.ptr(infer_wav), ws, n, _lib.ptr(sola_buffer), bs, Lb, int(search_frame), _lib.ptr(fade_in),
                                               _lib.ptr(fade_out), int(block_frame), _lib.ptr(out), int(block_frame), _lib.ptr(off), _lib.stream_ptr(dev)))
    return out, off


def envelope_mix_batch(input_wav: torch.Tensor, infer_wav: torch.Tensor, zc: int, rms_mix_rate: float) -> torch.Tensor:
    """``envelope_mix`` for a bank, IN PLACE on ``infer_wav`` [S, n] (returned) against the first ``n`` samples of the rows of
    ``input_wav`` [S, >= n]; rows may be views into longer buffers.  Three launches whatever ``S``; bit-equal per session."""
    dev = _lib.on_gpu(infer_wav, "infer_wav")
    S, n, ws = bank_rows(infer_wav, "infer_wav")
    Si, ni, ins = bank_rows(input_wav, "input_wav", dev)
    if Si != S:
        raise ValueError("infer_wav has %d sessions, input_wav %d" % (S, Si))
    if ni < n:
        raise ValueError("input_wav has %d samples, infer_wav %d" % (ni, n))
    zc = int(zc)
    if zc < 1:
        raise ValueError("zc must be positive")
    scratch = torch.empty(S * 2 * (1 + n // zc), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_envelope_mix_batch(S, _lib.ptr(input_wav), ins, _lib.ptr(infer_wav), ws, n, zc, float(rms_mix_rate),
                                                            _lib.ptr(scratch), _lib.stream_ptr(dev)))
    return infer_wav


def input_gate_scratch_floats(zc: int, blk: int) -> int:
    """Floats of scratch per session of ``input_gate_batch`` (0: the geometry is refused)."""
    return int(_lib.lib().rvcmi_glue_input_gate_scratch_floats(int(zc), int(blk)))


def input_gate_batch(block: torch.Tensor, rms_buffer: torch.Tensor, dst: torch.Tensor, zc: int, cut_a: float, cut_b: float,
                     scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``realtime.input_gate`` (gui.py:950-963) for a bank, on the device: ``block`` [S, blk] (the raw block), ``rms_buffer`` [S, 4 zc]
    (updated in place), ``dst`` [S, blk + 2 zc] (written: the gated samples; its rows are usually the tails of the rolling ``input_wav``),
    ``cut_a`` / ``cut_b`` = ``realtime.input_gate_cutoffs(threhold)``.  Rows of all three may be views into longer buffers.  Session ``s``
    equals ``input_gate`` on its rows bit for bit; three launches whatever ``S``.  ``scratch``: float32, at least ``S *
    input_gate_scratch_floats(zc, blk)`` elements (allocated when None).  Returns ``dst``."""
    dev = _lib.on_gpu(block, "block")
    S, blk, bs = bank_rows(block, "block")
    Sr, nr, rs = bank_rows(rms_buffer, "rms_buffer", dev)
    Sd, nd, ds = bank_rows(dst, "dst", dev)
    zc = int(zc)
    if Sr != S or Sd != S:
        raise ValueError("block, rms_buffer and dst must hold the same number of sessions")
    per = input_gate_scratch_floats(zc, blk)
    if per == 0:
        raise _lib.RvcmiError("input_gate_batch: a block of %d samples must be a whole number (>= 1) of hops of zc = %d >= 1 samples" % (blk, zc),
                              code=_lib.ERR_INVALID)
    if nr != 4 * zc or nd != blk + 2 * zc:
        raise ValueError("rms_buffer must be [S, %d] and dst [S, %d], got %s / %s" % (4 * zc, blk + 2 * zc, tuple(rms_buffer.shape), tuple(dst.shape)))
    if S > 1 and (rs < nr or ds < nd):
        raise ValueError("the rows of rms_buffer / dst overlap")
    if scratch is None:
        scratch = torch.empty(S * per, device=dev, dtype=torch.float32)
    elif scratch.dtype != torch.float32 or scratch.device != dev or not scratch.is_contiguous() or scratch.numel() < S * per:
        raise ValueError("scratch must be a contiguous float32 tensor of at least %d elements on %s" % (S * per, dev))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_input_gate_batch(S, _lib.ptr(block), bs, _lib.ptr(rms_buffer), rs, _lib.ptr(dst), ds, zc, blk, float(cut_a),
                                                          float(cut_b), _lib.ptr(scratch), _lib.stream_ptr(dev)))
    return dst


# ---- the realtime controls per session (RealtimeBank's index_rate / protect / rms_mix_rate / threhold sliders) ----------------------------
# Each entry takes its per-session values twice (rvcmi.h): a host array that the library checks, and the same bytes on the device that the
# kernels read.  The plans below are pure host functions; the device copy of a plan is kept until the values change (the pattern of
# RealtimeBank._mask), so an unchanged bank step uploads nothing.

def session_blend_plan(index_rates, protects, has_index: bool, has_pitchf: bool):
    """Per session ``(index_rate, protect, slot, protect_on)`` of ``retrieve_blend_expand_sessions``: a session is searched and blended iff
    there is an index and its rate is not 0 (``retrieve_blend_expand``'s rule), and then ``slot`` is its position among those that are (else
    -1); its protect mix applies iff there is a pitchf and its protect is below 0.5.  No device needed."""
    rates, protects = [float(r) for r in index_rates], [float(p) for p in protects]
    if len(rates) != len(protects) or not rates:
        raise ValueError("index_rates and protects must hold one value per session (got %d / %d)" % (len(rates), len(protects)))
    out, nxt = [], 0
    for r, p in zip(rates, protects):
        if not (np.isfinite(r) and np.isfinite(p)):
            raise ValueError("index_rate / protect must be finite (got %r / %r)" % (r, p))
        blend, on = bool(has_index) and r != 0, bool(has_pitchf) and p < 0.5
        out.append((r if blend else 0.0, p if on else 1.0, nxt if blend else -1, 1 if on else 0))
        nxt += 1 if blend else 0
    return out


def session_mix_plan(rms_mix_rates):
    """Per session ``(exponent, on)`` of ``envelope_mix_sessions``: ``float32(1 - rate)`` computed in double and rounded once, as the scalar
    entry does, and on iff ``rate < 1`` (gui.py:1024)."""
    out = []
    for r in rms_mix_rates:
        r = float(r)
        if not np.isfinite(r):
            raise ValueError("rms_mix_rate must be finite (got %r)" % (r,))
        out.append((float(np.float32(1.0 - r)), 1 if r < 1 else 0))
    if not out:
        raise ValueError("rms_mix_rates must hold one value per session")
    return out


def session_gate_plan(threholds):
    """Per session ``(cut_a, cut_b, on)`` of ``input_gate_sessions``: on iff ``threhold > -60`` (gui.py:950), the cutoffs those of
    ``realtime.input_gate_cutoffs`` (0, 0 for a session that is off)."""
    from .realtime import input_gate_cutoffs

    out = []
    for t in threholds:
        t = float(t)
        if not np.isfinite(t):
            raise ValueError("threhold must be finite (got %r)" % (t,))
        out.append(input_gate_cutoffs(t) + (1,) if t > -60 else (0.0, 0.0, 0))
    if not out:
        raise ValueError("threholds must hold one value per session")
    return out


_SESSION_ROWS: dict = {}   # (device index, struct, plan) -> (host array, its bytes on the device)
_SESSION_ROWS_KEEP = 16
session_rows_uploads = 0   # how often a plan went to the device (tests read it)


def _session_rows(struct, plan, dev):
    """``plan`` (a list of per-session field tuples) as an array of ``struct`` on the host and the same bytes on ``dev``; cached per plan."""
    global session_rows_uploads
    key = (_lib.device_index(dev), struct.__name__, tuple(plan))
    hit = _SESSION_ROWS.get(key)
    if hit is None:
        arr = (struct * len(plan))(*[struct(*row) for row in plan])
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        while len(_SESSION_ROWS) >= _SESSION_ROWS_KEEP:
            _SESSION_ROWS.pop(next(iter(_SESSION_ROWS)))
        hit = _SESSION_ROWS[key] = (arr, raw.to(dev))
        session_rows_uploads += 1
    return hit


def retrieve_blend_expand_sessions(feats: torch.Tensor, index, index_rates, pitchf: Optional[torch.Tensor] = None, protects=None,
                                   p_len: Optional[int] = None, realtime_guard: bool = True, skip_rows: int = 0) -> torch.Tensor:
    """``retrieve_blend_expand_batch`` with an ``index_rate`` and a ``protect`` per session: ``feats`` [S, nq, d] -> [S, p_len, d].  Row ``s``
    equals ``retrieve_blend_expand(feats[s:s+1], index, index_rates[s], pitchf[s], protects[s], p_len, realtime_guard, skip_rows)`` bit for
    bit.  Only the sessions whose rate is not 0 contribute rows to the one search (none: no search); a session whose rate is 0 comes out as
    the bits of its input rows; the guard stays per session.  ``index`` may be None (a protect per session without an index).  The launch
    count depends on neither ``S`` nor on which sessions blend."""
    dev = _lib.on_gpu(feats, "feats")
    if feats.dim() != 3 or feats.shape[0] < 1:
        raise ValueError("feats must be [S, nq, d] with S >= 1")
    S, nq, d = int(feats.shape[0]), int(feats.shape[1]), int(feats.shape[2])
    p_len = 2 * nq if p_len is None else min(int(p_len), 2 * nq)
    protects = [1.0] * S if protects is None else list(protects)
    index_rates = list(index_rates)
    if len(index_rates) != S or len(protects) != S:
        raise ValueError("index_rates / protects must hold %d values, got %d / %d" % (S, len(index_rates), len(protects)))
    f = feats.to(torch.float32).contiguous()
    plan = session_blend_plan(index_rates, protects, index is not None, pitchf is not None)
    pf = None
    if any(row[3] for row in plan):
        if pitchf.dim() != 2 or pitchf.shape[0] != S or pitchf.shape[1] < p_len:
            raise ValueError("pitchf must be [%d, >= %d], got %s" % (S, p_len, tuple(pitchf.shape)))
        pf = pitchf[:, :p_len].to(dev, torch.float32).contiguous()
    active = sum(1 for row in plan if row[2] >= 0)
    h = max(0, min(int(skip_rows), nq))
    host, on_dev = _session_rows(_lib.SessionBlend, plan, dev)
    out = torch.empty(S, p_len, d, device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        handle = None
        if index is not None:
            if d != index.d:
                raise ValueError("index mistatch")  # the reference's message (pipeline.py:128)
            if _lib.device_index(index.device) != _lib.device_index(dev):
                raise _lib.RvcmiError("the index lives on %s, the features on %s: read the index on the pipeline's device "
                                      "(read_index(path, device=...))" % (index.device, dev))
            if active:
                index.reserve(active * (nq - h))
            handle = index._h
        _lib.check(_lib.lib().rvcmi_ivf_search_blend_expand_sessions(handle, S, nq, d, h, _lib.ptr(f), C.cast(host, C.c_void_p), _lib.ptr(on_dev), 8,
                                                                     1 if realtime_guard else 0, _lib.ptr(pf), p_len, _lib.ptr(out),
                                                                     _lib.stream_ptr(dev)))
    return out.to(feats.dtype)


def envelope_mix_sessions(input_wav: torch.Tensor, infer_wav: torch.Tensor, zc: int, rms_mix_rates) -> torch.Tensor:
    """``envelope_mix_batch`` with a ``rms_mix_rate`` per session, IN PLACE on ``infer_wav`` [S, n] (returned): row ``s`` equals
    ``envelope_mix`` with its own rate bit for bit; the row of a session whose rate is 1 or more is not written.  Three launches whatever
    ``S`` and whichever sessions mix (none when no session does)."""
    dev = _lib.on_gpu(infer_wav, "infer_wav")
    S, n, ws = bank_rows(infer_wav, "infer_wav")
    Si, ni, ins = bank_rows(input_wav, "input_wav", dev)
    if Si != S:
        raise ValueError("infer_wav has %d sessions, input_wav %d" % (S, Si))
    if ni < n:
        raise ValueError("input_wav has %d samples, infer_wav %d" % (ni, n))
    zc = int(zc)
    if zc < 1:
        raise ValueError("zc must be positive")
    plan = session_mix_plan(rms_mix_rates)
    if len(plan) != S:
        raise ValueError("rms_mix_rates must hold %d values, got %d" % (S, len(plan)))
    host, on_dev = _session_rows(_lib.SessionMix, plan, dev)
    scratch = torch.empty(S * 2 * (1 + n // zc), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_envelope_mix_sessions(S, _lib.ptr(input_wav), ins, _lib.ptr(infer_wav), ws, n, zc, C.cast(host, C.c_void_p),
                                                               _lib.ptr(on_dev), _lib.ptr(scratch), _lib.stream_ptr(dev)))
    return infer_wav


def input_gate_sessions(block: torch.Tensor, rms_buffer: torch.Tensor, dst: torch.Tensor, zc: int, threholds,
                        scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``input_gate_batch`` with a ``threhold`` per session (the arguments are its: ``block`` [S, blk], ``rms_buffer`` [S, 4 zc], ``dst``
    [S, blk + 2 zc]).  A session with ``threhold > -60`` equals ``realtime.input_gate`` with its own threshold bit for bit.  A session at or
    below -60 ends as the stream that does not call the gate: the last ``blk`` samples of its ``dst`` row are the raw block, the ``2 zc`` in
    front of them and its ``rms_buffer`` row are not touched.  Three launches whatever ``S`` and whichever sessions gate.  Returns ``dst``."""
    dev = _lib.on_gpu(block, "block")
    S, blk, bs = bank_rows(block, "block")
    Sr, nr, rs = bank_rows(rms_buffer, "rms_buffer", dev)
    Sd, nd, ds = bank_rows(dst, "dst", dev)
    zc = int(zc)
    if Sr != S or Sd != S:
        raise ValueError("block, rms_buffer and dst must hold the same number of sessions")
    per = input_gate_scratch_floats(zc, blk)
    if per == 0:
        raise _lib.RvcmiError("input_gate_sessions: a block of %d samples must be a whole number (>= 1) of hops of zc = %d >= 1 samples" % (blk, zc),
                              code=_lib.ERR_INVALID)
    if nr != 4 * zc or nd != blk + 2 * zc:
        raise ValueError("rms_buffer must be [S, %d] and dst [S, %d], got %s / %s" % (4 * zc, blk + 2 * zc, tuple(rms_buffer.shape), tuple(dst.shape)))
    if S > 1 and (rs < nr or ds < nd):
        raise ValueError("the rows of rms_buffer / dst overlap")
    plan = session_gate_plan(threholds)
    if len(plan) != S:
        raise ValueError("threholds must hold %d values, got %d" % (S, len(plan)))
    host, on_dev = _session_rows(_lib.SessionGate, [row + (0,) for row in plan], dev)
    if scratch is None:
        scratch = torch.empty(S * per, device=dev, dtype=torch.float32)
    elif scratch.dtype != torch.float32 or scratch.device != dev or not scratch.is_contiguous() or scratch.numel() < S * per:
        raise ValueError("scratch must be a contiguous float32 tensor of at least %d elements on %s" % (S * per, dev))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_input_gate_sessions(S, _lib.ptr(block), bs, _lib.ptr(rms_buffer), rs, _lib.ptr(dst), ds, zc, blk,
                                                             C.cast(host, C.c_void_p), _lib.ptr(on_dev), _lib.ptr(scratch), _lib.stream_ptr(dev)))
    return dst


def phase_vocoder(a: torch.Tensor, b: torch.Tensor, fade_out: torch.Tensor, fade_in: torch.Tensor) -> torch.Tensor:
    """``phase_vocoder(a, b, fade_out, fade_in)`` of gui.py:27-49 on the device (n = len(a) <= 4096): the windowed spectra of
    both signals, their summed magnitudes and wrapped phase difference, and the O(n^2 / 2) phase-interpolating synthesis, in
    fp64.  A bin whose spectrum is exactly zero has phase 0.  Returns a new float32 tensor [n]."""
    dev = _lib.on_gpu(a, "a")
    n = int(a.numel())
    for t, nm in ((a, "a"), (b, "b"), (fade_out, "fade_out"), (fade_in, "fade_in")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.dim() != 1 or t.numel() != n:
            raise ValueError("%s must be a contiguous 1-D float32 tensor of %d samples on %s" % (nm, n, dev))
    out = torch.empty(n, device=dev, dtype=torch.float32)
    scratch = torch.empty(3 * (n // 2 + 1), device=dev, dtype=torch.float64)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_phase_vocoder(_lib.ptr(a), _lib.ptr(b), _lib.ptr(fade_out), _lib.ptr(fade_in), n, _lib.ptr(out), _lib.ptr(scratch),
                                                       _lib.stream_ptr(dev)))
    return out


def envelope_mix(input_wav: torch.Tensor, infer_wav: torch.Tensor, zc: int, rms_mix_rate: float) -> torch.Tensor:
    """The realtime GUI's volume-envelope mix (gui.py:1023-1056), IN PLACE on ``infer_wav`` (returned): frame RMS of
    ``input_wav[:len(infer_wav)]`` and of ``infer_wav`` (frame 4 zc, hop zc), both interpolated with ``align_corners=True``,
    ``infer_wav *= pow(rms1 / max(rms2, 1e-3), 1 - rms_mix_rate)``.  Not ``change_rms``: that is the offline formula."""
    dev = _lib.on_gpu(infer_wav, "infer_wav")
    for t, nm in ((input_wav, "input_wav"), (infer_wav, "infer_wav")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 1 or t.device != dev:
            raise ValueError("%s must be a contiguous 1-D float32 tensor on %s" % (nm, dev))
    n, zc = int(infer_wav.numel()), int(zc)
    if input_wav.numel() < n:
        raise ValueError("input_wav has %d samples, infer_wav %d" % (input_wav.numel(), n))
    if zc < 1:
        raise ValueError("zc must be positive")
    scratch = torch.empty(2 * (1 + n // zc), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_envelope_mix(_lib.ptr(input_wav), _lib.ptr(infer_wav), n, zc, float(rms_mix_rate), _lib.ptr(scratch),
                                                      _lib.stream_ptr(dev)))
    return infer_wav


def spectral_gate(x: torch.Tensor, xn: Optional[torch.Tensor], n_fft: int, hop: int, window: torch.Tensor,
                  smoothing_filter: Optional[torch.Tensor] = None, nonstationary: bool = False, n_std_thresh: float = 1.5,
                  n_thresh_ns: float = 1.3, temp_coeff: float = 0.1, n_movemean: int = 20, prop_decrease: float = 1.0) -> torch.Tensor:
    """``TorchGate.forward(x, xn)`` (infer/modules/gui/torchgate.py) in one enqueue-only call: x [B, L] and xn [B, Ln] (or None)
    contiguous float32, ``window`` [n_fft] float64 (the hann window zero-padded to the centre), ``smoothing_filter`` [nf, nt]
    float32 or None.  Returns a new float32 tensor [B, hop * (L // hop)].  STFT, statistics and overlap-add in fp64
    (rvcmi.h); n_fft must be even and <= 4096.  The overlap-add divides by the summed squared window unchecked: a window / hop pair
    that leaves a kept sample uncovered (``torch.istft`` refuses those) gives inf / NaN there; that is the caller's to rule out
    (``TorchGateHIP`` does, on the host)."""
    dev = _lib.on_gpu(x, "x")
    tensors = [(x, "x", torch.float32), (window, "window", torch.float64)]
    if xn is not None:
        tensors.append((xn, "xn", torch.float32))
    if smoothing_filter is not None:
        tensors.append((smoothing_filter, "smoothing_filter", torch.float32))
    for t, nm, dt in tensors:
        _lib.on_gpu(t, nm)
        if t.device != dev:
            raise _lib.RvcmiError("%s lives on %s, x on %s" % (nm, t.device, dev))
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor" % (nm, dt))
    if x.dim() != 2 or (xn is not None and (xn.dim() != 2 or xn.shape[0] != x.shape[0])):
        raise ValueError("x must be [B, L] and xn [B, Ln]")
    if window.dim() != 1 or window.numel() != int(n_fft):
        raise ValueError("window must have n_fft = %d samples" % int(n_fft))
    B, n = int(x.shape[0]), int(x.shape[1])
    nn = int(xn.shape[1]) if xn is not None else 0
    hop = int(hop)
    nf, nt = (int(smoothing_filter.shape[-2]), int(smoothing_filter.shape[-1])) if smoothing_filter is not None else (0, 0)
    L = _lib.lib()
    nbytes = int(L.rvcmi_glue_spectral_gate_scratch_bytes(B, n, nn, int(n_fft), hop))
    if nbytes == 0:
        raise _lib.RvcmiError("spectral_gate: n_fft = %d (even, <= 4096), hop = %d (1..n_fft) or the shapes %s / %s are out of range"
                              % (int(n_fft), hop, tuple(x.shape), tuple(xn.shape) if xn is not None else None), code=_lib.ERR_INVALID)
    out = torch.empty(B, hop * (n // hop) if hop > 0 else 0, device=dev, dtype=torch.float32)
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        _lib.check(L.rvcmi_glue_spectral_gate(_lib.ptr(x), B, n, _lib.ptr(xn), nn, int(n_fft), hop, _lib.ptr(window), _lib.ptr(smoothing_filter), nf, nt,
                                              1 if nonstationary else 0, float(n_std_thresh), float(n_thresh_ns), float(temp_coeff),
                                              int(n_movemean), float(prop_decrease), _lib.ptr(out), _lib.ptr(scratch), nbytes, _lib.stream_ptr(dev)))
    return out


def gate_ring_plan(nn: int, n_fft: int, hop: int, shift: int, tail: int) -> dict:
    """The dirty-frame rule of ``spectral_gate_ring`` (rvcmi.h, csrc/gate_ring.hpp; host only, no device): of the ``Fn = 1 + nn // hop``
    frames of a rolling noise buffer that moved left by ``shift`` samples and whose last ``tail`` samples were rewritten, the frames
    ``[0, head)`` and ``[back, Fn)`` must be transformed again (``head == back == Fn``: all of them); ``advance`` is what the caller adds to
    its ring base before the call.  -> dict(Fn, K, head, back, advance, n_dirty)."""
    out = (C.c_int * 6)()
    _lib.check(_lib.lib().rvcmi_glue_gate_ring_plan(int(nn), int(n_fft), int(hop), int(shift), int(tail), out))
    return dict(zip(("Fn", "K", "head", "back", "advance", "n_dirty"), (int(v) for v in out)))


def _bank_mode(mode: torch.Tensor, S: int, dev) -> None:
    if mode.dtype != torch.uint8 or mode.dim() != 1 or mode.numel() != S or mode.device != dev or not mode.is_contiguous():
        raise ValueError("mode must be a contiguous uint8 tensor [%d] on %s" % (S, dev))


def _rows_overlap(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Do the memory spans of two row arrays intersect?  (Spans, not elements: interleaved rows of one buffer count as overlapping.)"""
    def span(t):
        lo = t.data_ptr()
        return lo, lo + 4 * ((t.shape[0] - 1) * t.stride(0) + t.shape[1] if t.shape[0] > 1 else t.shape[1])
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def spectral_gate_ring(x: torch.Tensor, xn: torch.Tensor, shift: int, tail: int, ring: torch.Tensor, ring_base: int, mode: torch.Tensor,
                       any_cold: bool, n_fft: int, hop: int, window: torch.Tensor, smoothing_filter: Optional[torch.Tensor] = None,
                       n_std_thresh: float = 1.5, prop_decrease: float = 1.0, out: Optional[torch.Tensor] = None,
                       scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The stationary ``spectral_gate(x, xn)`` for a bank whose noise rows ``xn`` [S, nn] are rolling buffers (rvcmi.h,
    ``rvcmi_glue_spectral_gate_ring_batch``): ``ring`` (uint8, ``>= rvcmi_glue_spectral_gate_ring_bytes``) keeps every session's noise
    spectra, ``mode`` uint8 [S] says per session off (0) / warm (1: only the frames ``gate_ring_plan`` calls dirty are transformed) / cold
    (2), ``any_cold`` whether some session is cold.  Rows of ``x`` [S, n], ``xn`` and ``out`` [S, hop * (n // hop)] may be slices of
    longer buffers; ``out`` may be ``x`` itself (in place), must not overlap ``xn``, and is allocated when None (rows of off sessions are
    then uninitialised).  Active rows equal ``spectral_gate`` on contiguous copies bit for bit.  ``TorchGateBank`` keeps the state."""
    dev = _lib.on_gpu(x, "x")
    S, n, xs = bank_rows(x, "x")
    Sn, nn, ns = bank_rows(xn, "xn", dev)
    if Sn != S:
        raise ValueError("x has %d sessions, xn %d" % (S, Sn))
    _bank_mode(mode, S, dev)
    hop, n_fft = int(hop), int(n_fft)
    if window.dtype != torch.float64 or window.dim() != 1 or window.numel() != n_fft or not window.is_contiguous() or window.device != dev:
        raise ValueError("window must be a contiguous float64 tensor of n_fft = %d samples on %s" % (n_fft, dev))
    if smoothing_filter is not None and (smoothing_filter.dtype != torch.float32 or smoothing_filter.dim() != 2 or not smoothing_filter.is_contiguous()
                                         or smoothing_filter.device != dev):
        raise ValueError("smoothing_filter must be a contiguous float32 tensor [nf, nt] on %s" % dev)
    L = _lib.lib()
    nbytes, rbytes = int(L.rvcmi_glue_spectral_gate_ring_scratch_bytes(S, n, n_fft, hop)), int(L.rvcmi_glue_spectral_gate_ring_bytes(S, nn, n_fft, hop))
    if nbytes == 0 or rbytes == 0:
        raise _lib.RvcmiError("spectral_gate_ring: n_fft = %d (even, <= 4096), hop = %d (1..n_fft) or the shapes %s / %s are out of range"
                              % (n_fft, hop, tuple(x.shape), tuple(xn.shape)), code=_lib.ERR_INVALID)
    if ring.dtype != torch.uint8 or ring.device != dev or not ring.is_contiguous() or ring.numel() < rbytes:
        raise ValueError("ring must be a contiguous uint8 tensor of at least %d bytes on %s" % (rbytes, dev))
    Lout = hop * (n // hop)
    if out is None:
        out = torch.empty(S, Lout, device=dev, dtype=torch.float32)
    So, no, os_ = bank_rows(out, "out", dev)
    if So != S or no != Lout:
        raise ValueError("out must be [%d, %d], got %s" % (S, Lout, tuple(out.shape)))
    if _rows_overlap(out, xn):
        raise ValueError("out must not overlap xn")
    if _rows_overlap(out, x) and not (out.data_ptr() == x.data_ptr() and os_ == xs):
        raise ValueError("out may be x itself (in place) but must not overlap it otherwise")
    if S > 1 and os_ < Lout:
        raise ValueError("the rows of out overlap")
    if scratch is None:
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    elif scratch.dtype != torch.uint8 or scratch.device != dev or not scratch.is_contiguous() or scratch.numel() < nbytes:
        raise ValueError("scratch must be a contiguous uint8 tensor of at least %d bytes on %s" % (nbytes, dev))
    nf, nt = (int(smoothing_filter.shape[0]), int(smoothing_filter.shape[1])) if smoothing_filter is not None else (0, 0)
    with torch.cuda.device(dev):
        _lib.check(L.rvcmi_glue_spectral_gate_ring_batch(S, _lib.ptr(x), xs, n, _lib.ptr(xn), ns, nn, _lib.ptr(out), os_, int(shift), int(tail),
                                                         _lib.ptr(ring), ring.numel(), int(ring_base), _lib.ptr(mode), 1 if any_cold else 0, n_fft, hop,
                                                         _lib.ptr(window), _lib.ptr(smoothing_filter), nf, nt, 0, float(n_std_thresh),
                                                         float(prop_decrease), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr(dev)))
    return out


def nr_stitch_batch(g: torch.Tensor, nr_buffer: torch.Tensor, denoise: torch.Tensor, fade_in: torch.Tensor, fade_out: torch.Tensor,
                    block_frame: int, mode: torch.Tensor, den_prev: Optional[torch.Tensor] = None) -> None:
    """The GUI's cross-fade of the gated input (gui.py:986-990) for the sessions with ``mode != 0``, in place on ``nr_buffer`` [S, Lb] and
    ``denoise`` [S, n]: ``g[:Lb] = g[:Lb] * fade_in + nr_buffer * fade_out; denoise[-blk:] = g[:blk]; nr_buffer = g[blk:]`` with ``g``
    [S, blk + Lb] the gate's output (not written), bit-equal to the torch statements.  ``den_prev`` [S, n - blk]: a copy of
    ``denoise[:, blk:]`` taken before, written to ``denoise[:, :-blk]`` (the roll, only for those sessions).  One launch."""
    dev = _lib.on_gpu(g, "g")
    S, ng, gs = bank_rows(g, "g")
    Sb, Lb, bs = bank_rows(nr_buffer, "nr_buffer", dev)
    Sd, nd, ds = bank_rows(denoise, "denoise", dev)
    blk = int(block_frame)
    if Sb != S or Sd != S or ng != blk + Lb:
        raise ValueError("g must be [S, block_frame + Lb] with nr_buffer [S, Lb] and denoise [S, n]")
    _bank_mode(mode, S, dev)
    for t, nm in ((fade_in, "fade_in"), (fade_out, "fade_out")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() != Lb:
            raise ValueError("%s must be a contiguous float32 tensor of %d samples on %s" % (nm, Lb, dev))
    ps = 0
    if den_prev is not None:
        Sp, npv, ps = bank_rows(den_prev, "den_prev", dev)
        if Sp != S or npv != nd - blk or _rows_overlap(den_prev, denoise):
            raise ValueError("den_prev must be a copy [S, %d] of denoise[:, block_frame:]" % (nd - blk))
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_nr_stitch_batch(S, _lib.ptr(g), gs, Lb, blk, _lib.ptr(fade_in), _lib.ptr(fade_out), _lib.ptr(nr_buffer), bs,
                                                         _lib.ptr(denoise), ds, nd, _lib.ptr(den_prev), ps, _lib.ptr(mode), _lib.stream_ptr(dev)))


def masked_write_batch(dst: torch.Tensor, mode: torch.Tensor, a: torch.Tensor, off_a: int, b: Optional[torch.Tensor] = None, off_b: int = 0) -> None:
    """Per session ``s``: ``dst[s, off_a : off_a + a.shape[1]] = a[s]`` where ``mode[s] != 0``, else ``dst[s, off_b : off_b + b.shape[1]] =
    b[s]`` (nothing when ``b`` is None).  Rows may be slices of longer buffers; ``a`` / ``b`` must not overlap ``dst``.  One launch."""
    dev = _lib.on_gpu(dst, "dst")
    S, nd, ds = bank_rows(dst, "dst")
    Sa, na, as_ = bank_rows(a, "a", dev)
    _bank_mode(mode, S, dev)
    Sb, nb, bs = (S, 0, 0)
    if b is not None:
        Sb, nb, bs = bank_rows(b, "b", dev)
    if Sa != S or Sb != S:
        raise ValueError("dst, a and b must hold the same number of sessions")
    if _rows_overlap(dst, a) or (b is not None and _rows_overlap(dst, b)):
        raise ValueError("a / b must not overlap dst")
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().rvcmi_glue_masked_write_batch(S, _lib.ptr(dst), ds, nd, _lib.ptr(a), as_, int(off_a), na, _lib.ptr(b), bs, int(off_b), nb,
                                                            _lib.ptr(mode), _lib.stream_ptr(dev)))
