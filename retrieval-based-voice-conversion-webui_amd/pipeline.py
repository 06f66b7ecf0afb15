"""Retrieval glue of ``Pipeline.vc`` (infer/modules/vc/pipeline.py:113-138) and ``RVC.infer``
(infer/lib/rtrvc.py:167-187), device resident.

The reference moves HuBERT features to the host, calls faiss, blends with numpy and moves the result
back (2x D2H + 2x H2D per chunk).  ``retrieve_blend`` does the same arithmetic on the GPU in one call.
"""
from __future__ import annotations

import torch

from . import _lib
from .ivf import IVFFlatHIP


def retrieve_blend(feats: torch.Tensor, index: IVFFlatHIP, index_rate: float, k: int = 8,
                   realtime_guard: bool = False) -> torch.Tensor:
    """feats [1 or B, T, d] (HuBERT output, any float dtype, CUDA) -> same shape/dtype with

        score, ix = index.search(npy, k=8); weight = square(1/score); weight /= weight.sum(1)
        npy = sum(big_npy[ix] * weight[..., None], 1); feats = npy*index_rate + (1-index_rate)*feats

    (pipeline.py:126-138).  ``index is None`` or ``index_rate == 0`` returns feats untouched, as the
    reference's guard at pipeline.py:113-117 does.  ``realtime_guard`` = rtrvc.py:173.
    """
    if index is None or index_rate == 0:
        return feats
    shape, dtype = feats.shape, feats.dtype
    flat = feats.reshape(-1, shape[-1]).to(torch.float32).contiguous()
    if flat.data_ptr() == feats.data_ptr():
        flat = flat.clone()  # the reference builds a new tensor; keep the caller's feats0 copy valid
    index.search_blend(flat, float(index_rate), k, skip_if_short=realtime_guard)
    return flat.reshape(shape).to(dtype)


# ------------------------------------------------------------------------------------------------------------------------
# Device-resident ``Pipeline.vc`` / ``Pipeline.pipeline`` (infer/modules/vc/pipeline.py:76-184, 186-360)
# ------------------------------------------------------------------------------------------------------------------------
# ``install()`` binds ``vc_hip`` / ``pipeline_hip`` as the ``vc`` / ``pipeline`` methods of the reference's own ``Pipeline``
# class (whose ``__init__`` state -- x_pad, window, t_pad*, is_half, device, f0_gen -- they read), so an unmodified
# ``VC.vc_single`` runs them.  HuBERT stays the caller's ``model`` on PyTorch-ROCm; from its output on nothing visits the host:
# search + blend + x2 + protect mix in one launch (rvcmi_ivf_search_blend_expand), ``net_g.infer`` on the HIP front + generator,
# segments concatenated, ``change_rms`` and the int16-range scaling on the device, ONE copy to the host at the very end
# (the API returns a numpy array).  Host work that remains is the reference's own input preparation on the 16 kHz waveform
# (high-pass ``filtfilt``) and estimators other than RMVPE.  The quiet-point search that chooses the cut positions of a long input
# runs on the device (``glue.cut_points``, bit-equal to the host loop): one upload of the filtered fp64 signal, which
# ``change_rms`` then shares, and one small synchronising read-back of the cuts per long file -- segment shapes depend on them.
#
# Opt-in (``install(device_prep=True)`` or ``RVCMI_DEVICE_PREP=1``; default off): the input preparation itself on the device.
# The raw input is uploaded ONCE in its own dtype, ``glue.filtfilt_flat`` filters it (all files of a ``convert_files`` group in one
# call; a call with less than ``DEVICE_PREP_MIN_SAMPLES`` of audio, where the host filter is faster, stays on the host) and writes the
# ``t_pad`` reflection pad in the same launch; the cut search, the HuBERT segments, RMVPE and ``change_rms``
# read device slices of that one signal, and it visits the host (one D2H, the same signal, never a second host-filtered one) only
# when an f0 estimator other than the device RMVPE path needs ``audio_pad`` as numpy.  It is off by default because it cannot be
# bit-equal to scipy beyond ``glue.filtfilt_exact_len`` samples: the recurrence is ill-conditioned, and the device result is as far
# from the exact one as scipy's own is, which after the fp32 / fp16 cast moves about half the samples by one ulp.
# The casts themselves are the host's: ``.float()`` of an fp64 device tensor is the one IEEE rounding ``torch.as_tensor(numpy_f64)
# .float()`` does, and ``.half()`` goes through fp32 on both (c10::Half is constructed from float), which
# tests/test_gpu_prep.py::test_device_casts_round_as_the_host_casts checks on values that tell the two routes apart.

def _ref_module(self):
    import sys

    return sys.modules[type(self).__module__]


def _is_hip_index(index) -> bool:
    return isinstance(index, IVFFlatHIP)


def _hubert_wave(self, audio0):
    """The waveform as HuBERT takes it (pipeline.py:93-99): 1-D, fp16 / fp32 by ``is_half``, two channels averaged."""
    feats = torch.as_tensor(audio0)
    feats = feats.half() if self.is_half else feats.float()
    if feats.dim() == 2:  # double channels (pipeline.py:98-99)
        feats = feats.mean(-1)
    assert feats.dim() == 1, feats.dim()
    return feats


def hubert_device(self, model, audio0, pitch, pitchf, version, feats=None):
    """The HuBERT half of ``Pipeline.vc`` (pipeline.py:90-112, 146-151): -> (feats [1, nq, d] on the GPU, BEFORE retrieval,
    pitch [1, p_len] or None, pitchf or None, p_len).  ``feats``: the model's output for this segment when it has been computed already
    (``hubert_device_many``); only the tail -- ``final_proj``, ``p_len``, the pitch cut -- runs then."""
    if feats is None:
        dev = torch.device(self.device)
        feats = _hubert_wave(self, audio0).view(1, -1)
        padding_mask = torch.zeros(feats.shape, dtype=torch.bool, device=dev)
        from .hubert import accelerate_hubert_layers_once, accelerate_hubert_once

        accelerate_hubert_once(model)  # (beyond SURVEY 8; opt-in, a no-op with the switch off) the extractor's seven convolutions on HIP
        accelerate_hubert_layers_once(model)  # (RVCMI_HUBERT_ENC, opt-in, likewise) the transformer's layers on HIP
        with torch.no_grad():
            logits = model.extract_features(source=feats.to(dev), padding_mask=padding_mask, output_layer=9 if version == "v1" else 12)
            feats = model.final_proj(logits[0]) if version == "v1" else logits[0]
    elif version == "v1":
        with torch.no_grad():
            feats = model.final_proj(feats)
    use_f0 = pitch is not None and pitchf is not None
    nq = int(feats.shape[1])
    p_len = min(int(audio0.shape[0]) // self.window, 2 * nq)  # pipeline.py:146-151
    if use_f0:
        pitch, pitchf = pitch[:, :p_len], pitchf[:, :p_len]
    return feats, (pitch if use_f0 else None), (pitchf if use_f0 else None), p_len


def hubert_batched(model) -> bool:
    """Whether the segments of a call go through ``hubert_device_many``'s grouped path: both switches on (``RVCMI_HUBERT_FE`` and
    ``RVCMI_HUBERT_BATCH``, off by default) and a model that honours ``padding_mask`` (``hubert.batch_capable``).  Swaps the extractor first."""
    from . import hubert as hb

    if not hb.hubert_batch_on():
        return False
    hb.accelerate_hubert_once(model)
    hb.accelerate_hubert_layers_once(model)  # (RVCMI_HUBERT_ENC, opt-in: the swapped layers take the padding mask as their key mask)
    return hb.batch_capable(model)


def hubert_device_many(self, model, pending, version):
    """``hubert_device`` for every ``(audio0, pitch, pitchf)`` of ``pending``, in that order, with HuBERT run ONCE per planned group of
    segments of similar length (``hubert.plan_groups`` / ``hubert.extract_features_batch``: a ragged batch) instead of once
    per segment.  A group of fewer than ``hubert.HUBERT_BATCH_MIN_ITEMS`` segments, and everything when ``hubert_batched(model)`` is false,
    takes the per-segment call."""
    from . import hubert as hb

    out = [None] * len(pending)
    if not pending or not hubert_batched(model):
        return [hubert_device(self, model, a0, pt, pf, version) for a0, pt, pf in pending]
    waves = [_hubert_wave(self, a0) for a0, _, _ in pending]
    layer = 9 if version == "v1" else 12
    for group in hb.plan_groups([int(w.shape[0]) for w in waves], hb.HUBERT_BATCH_MAX_WASTE):
        if len(group) < hb.HUBERT_BATCH_MIN_ITEMS:
            for i in group:
                out[i] = hubert_device(self, model, *pending[i], version)
            continue
        for i, f in zip(group, hb.extract_features_batch(model, [waves[i] for i in group], layer)):
            out[i] = hubert_device(self, model, *pending[i], version, feats=f)
    return out


def features_device(self, model, audio0, pitch, pitchf, times, index, index_rate, version, protect):
    """``Pipeline.vc`` from HuBERT to the tensor handed to ``net_g.infer`` (pipeline.py:90-159): features on the GPU, retrieval
    blend + x2 + protect mix in one launch.  Returns (feats [1, p_len, d], pitch [1, p_len] or None, pitchf or None, p_len)."""
    from time import time

    from . import glue

    t0 = time()
    feats, pitch, pitchf, p_len = hubert_device(self, model, audio0, pitch, pitchf, version)
    use_f0 = pitch is not None
    use_index = index is not None and index_rate != 0
    feats = glue.retrieve_blend_expand(feats, index if use_index else None, float(index_rate), pitchf if use_f0 else None,
                                       float(protect) if use_f0 else 0.5, p_len)
    times[0] += time() - t0
    return feats, pitch, pitchf, p_len


MAX_FILES_PER_GROUP = 64   # inputs of convert_files whose HuBERT frames / waveforms are resident at once (BASELINE configs[2]: 64 clips per GPU)
MAX_BATCH_QUERIES = 65536  # HuBERT frames per retrieval call of blend_segments (22 minutes of audio; the score scratch stays < 1 GiB)


def blend_segments(raw, index, index_rate, protect):
    """The retrieval half of ``Pipeline.vc`` (pipeline.py:113-159) for MANY segments at once.  ``raw``: ``hubert_device`` results
    (of one file or of several).  All their HuBERT frames go through ONE ``rvcmi_ivf_search_blend_expand`` call per
    ``MAX_BATCH_QUERIES`` frames -- one coarse pass, one list-major scan: the rows of a probed list are read once for every segment
    that probes it -- and every segment gets back exactly the rows its own call would have produced (a row's search, blend, x2 and
    protect mix depend on nothing but that row).  -> items for ``infer_segments``."""
    from . import glue

    use_index = index is not None and index_rate != 0
    items = [None] * len(raw)
    start = 0
    while start < len(raw):
        end, n = start, 0
        while end < len(raw) and (end == start or n + int(raw[end][0].shape[1]) <= MAX_BATCH_QUERIES):
            n += int(raw[end][0].shape[1])
            end += 1
        grp = raw[start:end]
        dev, dtype = grp[0][0].device, grp[0][0].dtype
        use_f0 = grp[0][1] is not None
        F = torch.cat([g[0][0] for g in grp]).to(torch.float32).contiguous()  # [n, d]
        pf = None
        if use_f0 and float(protect) < 0.5:  # the frame-rate pitchf of every segment at ITS output rows (2 x its first query row)
            pf = torch.ones(2 * n, device=dev, dtype=torch.float32)
            o = 0
            for f, _, pff, p_len in grp:
                if pff.numel() < p_len:  # the message of glue.retrieve_blend_expand (the per-segment path) instead of a slice-size mismatch
                    raise ValueError("pitchf has %d frames, p_len is %d" % (pff.numel(), p_len))
                pf[2 * o: 2 * o + p_len] = pff.reshape(-1)[:p_len].to(dev, torch.float32)
                o += int(f.shape[1])
        out = torch.empty(2 * n, F.shape[1], device=dev, dtype=torch.float32)
        glue._blend_expand_into(out, F, index if use_index else None, float(index_rate), pf, float(protect) if use_f0 else 0.5, False)
        o = 0
        for i, (f, pt, pff, p_len) in enumerate(grp):
            items[start + i] = (out[2 * o: 2 * o + p_len].unsqueeze(0).to(dtype), pt, pff, p_len)
            o += int(f.shape[1])
        start = end
    return items


def vc_device(self, model, net_g, sid, audio0, pitch, pitchf, times, index, index_rate, version, protect) -> torch.Tensor:
    """``Pipeline.vc`` up to (not including) its final ``.data.cpu().float().numpy()``: returns the converted segment as a
    1-D device tensor.  ``audio0``: numpy or tensor (16 kHz segment, padded); ``index``: an ``IVFFlatHIP`` or None."""
    from time import time

    dev = torch.device(self.device)
    feats, pitch, pitchf, p_len = features_device(self, model, audio0, pitch, pitchf, times, index, index_rate, version, protect)
    t1 = time()
    plen_t = torch.tensor([p_len], device=dev).long()
    with torch.no_grad():
        audio1 = net_g.infer(feats, plen_t, sid, pitch=pitch, pitchf=pitchf)[0, 0] if pitch is not None else net_g.infer(feats, plen_t, sid)[0, 0]
    times[2] += time() - t1
    return audio1.data


# ---- all segments of a file in ONE ``net_g.infer`` call ------------------------------------------------------------------------------
# The reference converts the segments of a long input one ``vc`` call after the other (pipeline.py:301-343); they are independent
# once f0 is known.  With the ragged-batch entry of the generator (include/rvcmi.h rvcmi_nsf_forward ``lengths``: every item computed
# exactly as a separate call of its own length) they go through the front and the generator as one batch.  The noise of item b is
# drawn as the b-th sequential call would have drawn it (randn(1, 192, T_b); rand(1, 1, 1); randn(1, T_b * upp, 1)), so a seeded run
# consumes the generator exactly like the sequential pipeline.  Padded frames per call (items x longest item) are bounded (``MAX_BATCH_FRAMES``) so that
# the workspace of an hour-long file stays a few GB; segments beyond the bound go into further calls.
MAX_BATCH_FRAMES = 32768


def _ragged_capable(net_g) -> bool:
    from .front import infer_hip

    from .nsf import GeneratorHIP, NSFGeneratorHIP

    inf = getattr(net_g, "infer", None)
    routed = bool(getattr(inf, "_rvcmi_ragged", False)) or getattr(inf, "func", None) is infer_hip
    # ... and the generator behind it must be the HIP one: infer_hip cannot tell a foreign dec the lengths (it raises), and
    # infer_segments reads dec.upp / dec.cfg
    return routed and isinstance(getattr(net_g, "dec", None), (NSFGeneratorHIP, GeneratorHIP))


def infer_segments(net_g, sid, items, times=None):
    """``items``: list of (feats [1, T_b, d], pitch [1, T_b] or None, pitchf [1, T_b] or None, T_b) as ``features_device`` returns them.
    -> list of 1-D device tensors (the waveform of every item, ``T_b * upp`` samples), from as few ``net_g.infer`` calls as
    ``MAX_BATCH_FRAMES`` allows.  Bit-identical to one call per item with the kernel family pinned; the launcher's own per-shape choices
    may differ between a batch and a single clip by operand rounding."""
    from time import time

    t0 = time()
    outs = [None] * len(items)
    dev = items[0][0].device
    use_f0 = items[0][1] is not None
    upp = int(getattr(net_g.dec, "upp"))
    IC = int(net_g.dec.cfg["inter_channels"])
    start = 0
    while start < len(items):
        # the workspace of a call is B x T_max frames (padded), so THAT is what the bound applies to, not the sum of the lengths
        end, tmax = start, 0
        while end < len(items) and (end == start or (end - start + 1) * max(tmax, items[end][3]) <= MAX_BATCH_FRAMES):
            tmax = max(tmax, items[end][3])
            end += 1
        grp = items[start:end]
        B, Tm = len(grp), max(it[3] for it in grp)
        d = int(grp[0][0].shape[2])
        phone = torch.zeros(B, Tm, d, device=dev, dtype=grp[0][0].dtype)
        pitch = torch.ones(B, Tm, device=dev, dtype=torch.long) if use_f0 else None
        pitchf = torch.zeros(B, Tm, device=dev, dtype=grp[0][2].dtype) if use_f0 else None
        nzp = torch.zeros(B, IC, Tm, device=dev, dtype=grp[0][0].dtype)
        ndec = torch.zeros(B, Tm * upp, device=dev, dtype=grp[0][2].dtype) if use_f0 else None
        for b, (f, pt, pf, Tb) in enumerate(grp):
            phone[b, :Tb] = f[0]
            nzp[b, :, :Tb] = torch.randn(1, IC, Tb, device=dev, dtype=f.dtype)[0]       # randn_like(m_p)        synthesizers.py:182
            if use_f0:
                pitch[b, :Tb], pitchf[b, :Tb] = pt[0], pf[0]
                torch.rand(1, 1, 1, device=dev)                                          # rand_ini               generators.py:164
                ndec[b, :Tb * upp] = torch.randn(1, Tb * upp, 1, device=dev, dtype=pf.dtype)[0, :, 0]  # generators.py:192
        lens = torch.tensor([it[3] for it in grp], device=dev).long()
        sidb = sid.reshape(-1)[:1].expand(B).contiguous()
        with torch.no_grad():
            if use_f0:
                o = net_g.infer(phone, lens, sidb, pitch=pitch, pitchf=pitchf, noise_zp=nzp, noise_dec=ndec, ragged=True)
            else:
                o = net_g.infer(phone, lens, sidb, noise_zp=nzp, ragged=True)
        for b, it in enumerate(grp):
            outs[start + b] = o[b, 0, : it[3] * upp].data
        start = end
    if times is not None:
        times[2] += time() - t0
    return outs


def vc_hip(self, model, net_g, sid, audio0, pitch, pitchf, times, index, big_npy, index_rate, version, protect):
    """Drop-in ``Pipeline.vc`` (same arguments, same numpy return).  An index object that is not ours (a real faiss index
    the HIP reader could not serve) is handed to the reference's own ``vc``."""
    if index is not None and not _is_hip_index(index):
        orig = getattr(vc_hip, "_rvcmi_original", None)
        if orig is None:
            raise TypeError("Pipeline.vc: index is a %s, not an IVFFlatHIP, and no reference vc is bound" % type(index).__name__)
        return orig(self, model, net_g, sid, audio0, pitch, pitchf, times, index, big_npy, index_rate, version, protect)
    use_index = index is not None and big_npy is not None and index_rate != 0  # the reference's guard, pipeline.py:113-117
    out = vc_device(self, model, net_g, sid, audio0, pitch, pitchf, times, index if use_index else None, index_rate, version, protect)
    return out.cpu().float().numpy()


def _cut_points(self, audio, audio_pad_w):
    """pipeline.py:219-232: where a long input is cut -- the quietest sample (|x| summed over one window) within
    +-t_query of every multiple of t_center.  numpy float64 like the reference (same sums, same first-minimum rule)."""
    import numpy as np

    opt_ts = []
    if audio_pad_w.shape[0] > self.t_max:
        audio_sum = np.zeros_like(audio)
        for i in range(self.window):
            audio_sum += np.abs(audio_pad_w[i: i - self.window])
        for t in range(self.t_center, audio.shape[0], self.t_center):
            seg = audio_sum[t - self.t_query: t + self.t_query]
            opt_ts.append(t - self.t_query + int(np.where(seg == seg.min())[0][0]))
    return opt_ts


def _device_cuts(self, audio, dev):
    """The cut positions of ``_cut_points`` from the device search, or None when the host loop has to run (no GPU, a signal that is
    not float64, ``t_query > t_center`` -- numpy's negative slice start wraps there, the kernel refuses it --, a window the kernel
    does not stage, ``RVCMI_DEVICE_CUTS=0``).  -> (list of ints, the filtered signal as a float64 device tensor).  One upload, one
    synchronising read-back of ``len(opt_ts)`` integers."""
    import os

    import numpy as np

    from . import glue

    w = int(self.window)
    on_device = isinstance(audio, torch.Tensor)  # the device preparation's signal: searched where it lies, no upload
    f64 = torch.float64 if on_device else np.float64
    if (dev.type != "cuda" or os.environ.get("RVCMI_DEVICE_CUTS", "1") == "0" or audio.dtype != f64 or audio.ndim != 1
            or self.t_query > self.t_center or self.t_query < 1 or w % 2 or not 2 <= w <= 1024 or audio.shape[0] <= w
            or (on_device and audio.device.type != "cuda")):
        return None
    a64 = audio.contiguous() if on_device else torch.from_numpy(np.ascontiguousarray(audio)).to(dev)
    return glue.cut_points(a64, w, int(self.t_center), int(self.t_query)).tolist(), a64


def _file_cuts(self, audio, dev):
    """pipeline.py:222-236 for one filtered input (numpy, or the float64 device tensor of the device preparation): -> (opt_ts, its
    float64 device copy or None).  The search runs when the input,
    padded by half a window at each end, is longer than ``t_max`` (the reference's condition): on the device where that is
    possible, else by the host loop, which also answers ``[]`` for a short numpy input; a short device tensor is answered ``[]``
    where it lies (no copy, no synchronisation)."""
    import numpy as np

    on_device = isinstance(audio, torch.Tensor)
    if audio.shape[0] + 2 * (self.window // 2) > self.t_max:
        got = _device_cuts(self, audio, dev)
        if got is not None:
            return got
    elif on_device:
        return [], audio  # not searched at all (the common case: a clip under t_max): nothing to compute, and nothing leaves the device
    a64 = None
    if on_device:  # a device-prepared LONG input the device search does not serve (RVCMI_DEVICE_CUTS=0, t_query > t_center): host loop on a copy
        a64, audio = audio, audio.cpu().numpy()
    return _cut_points(self, audio, np.pad(audio, (self.window // 2, self.window // 2), mode="reflect")), a64


DEVICE_PREP = False  # install(device_prep=True) sets it; RVCMI_DEVICE_PREP=1 / =0 overrides it per call
# The device filter is used for the shapes where it was measured faster than the host's (tools/prep_time.py, profiles/prep_time.json).
# Its time hardly depends on the amount of audio -- every thread runs warm-up + 1024 samples of the recurrence, about 1.8 ms per call from
# 10 s to 64 x 10 s -- while scipy's grows by 0.23-0.33 ms per second of audio: 70 s, 305 s and a group of 64 x 10 s are faster on the
# device (10x, 27x, 18x with the uploads); for a single 10 s clip the device median is lower but the ranges of the two overlap, which
# counts as a tie.  Below 24 s of audio in one call (a file alone, or all files of a convert_files group together), where the gap is
# not yet a clear factor of two, the host prepares the input.
DEVICE_PREP_MIN_SAMPLES = 24 * 16000


_device_prep_on = _lib.Switch("RVCMI_DEVICE_PREP", globals(), "DEVICE_PREP").on


def _device_prep(self, audios, dev):
    """The input preparation of pipeline.py:221,241 for SEVERAL inputs on the device: one upload of the raw samples (float32 or
    float64 as they come; anything else is widened to float64 on the host, as scipy would), ONE ``glue.filtfilt_flat`` call (per
    sample type) that also writes the ``t_pad`` reflection pad.  -> per input (filtered float64 device tensor, its padded twin), or None for an input
    the device path does not serve (CPU device, not 1-D, not longer than ``t_pad`` / the filter's padlen: np.pad reflects such a
    signal several times over; or less than ``DEVICE_PREP_MIN_SAMPLES`` of audio in the whole call, where the host is faster): the
    caller prepares that one on the host."""
    import numpy as np

    from . import glue

    res = [None] * len(audios)
    if dev.type != "cuda" or not _device_prep_on():
        return res
    ref = _ref_module(self)
    padlen = 3 * max(len(ref.ah), len(ref.bh))
    arrs = [np.asarray(a) for a in audios]
    pick = [i for i, a in enumerate(arrs) if a.ndim == 1 and a.shape[0] > max(int(self.t_pad), padlen)]
    if not pick or sum(arrs[i].shape[0] for i in pick) < DEVICE_PREP_MIN_SAMPLES:
        return res
    # one call per sample type (a folder is one type in practice): a float32 input's odd extension is rounded in float32, as scipy
    # does it, so widening it to share a call with float64 files would not be "exactly as a call with that item alone"
    for dt in (np.float32, np.float64):
        grp = [i for i in pick if (arrs[i].dtype == np.float32) == (dt is np.float32)]
        if not grp:
            continue
        flat = np.concatenate([arrs[i].astype(dt, copy=False) for i in grp]) if len(grp) > 1 else np.ascontiguousarray(arrs[grp[0]], dtype=dt)
        outs, pads = glue.filtfilt_flat(torch.from_numpy(flat).to(dev), [arrs[i].shape[0] for i in grp], ref.bh, ref.ah, int(self.t_pad))
        for j, i in enumerate(grp):
            res[i] = (outs[j], pads[j])
    return res


RMVPE_THRED = 0.03  # rvc/f0/gen.py:113: Generator.calculate hard-codes compute_f0(..., filter_radius=0.03) for rmvpe


def _torch_rmvpe(self):
    """This f0_gen's torch RMVPE object (loaded on first use, as ``Generator`` does), or None when there is none the device path can read:
    no checkpoint, an onnx-only build, the onnx session of a ``privateuseone`` device."""
    gen = self.f0_gen
    if not hasattr(gen, "rmvpe"):
        try:
            from rvc.f0.rmvpe import RMVPE

            gen.rmvpe = RMVPE("%s/rmvpe.pt" % gen.rmvpe_root, is_half=gen.is_half, device=gen.device)
        except Exception:  # noqa  (no checkpoint / onnx-only build: the reference path decides what to do)
            return None
    r = gen.rmvpe
    if not (hasattr(r, "mel_extractor") and hasattr(r, "_mel2hidden")) or "privateuseone" in str(getattr(r, "device", "")):
        return None
    return r


def _rmvpe_on_device(self, audio_pad, p_len, f0_up_key):
    """RMVPE salience on PyTorch-ROCm (the reference's own mel extractor + network), decoded by ``rvcmi_glue_rmvpe_f0``
    (rvc/f0/rmvpe.py:119-164, f0.py:31-78, gen.py:10-41) without visiting the host.  None when this f0_gen has no torch RMVPE.

    The caller's ``filter_radius`` is NOT the voicing threshold: it is harvest's median radius (the UI slider 0..7, web.py:794)
    that ``vc_single`` forwards to every estimator; ``Generator.calculate`` ignores it for rmvpe and passes the constant 0.03
    (rvc/f0/gen.py:113), and so does this function."""
    from . import glue

    gen = self.f0_gen
    r = _torch_rmvpe(self)
    if r is None:
        return None
    # opt-in (RVCMI_RMVPE_HIP=1 / install(rmvpe_hip=True), default off): the whole estimator on this project's kernels (rmvpe.py) -- mel front end
    # and head included, no torch op but one cast between the waveform and (pitch, pitchf) -- and a key that may be fractional.  A model the
    # kernels do not serve keeps the path below.
    from . import rmvpe as _rm

    on = _rm.rmvpe_on()
    if on:
        hip = _rm.for_generator(gen, r)
        if hip is not None:
            return hip.f0(torch.as_tensor(audio_pad).float().to(hip.device), p_len, f0_up_key, RMVPE_THRED)
    # (beyond SURVEY.md section 8) the network's bidirectional GRU -- 75-90 % of a conversion as MIOpen runs it, bench.py --e2e -- on the
    # persistent HIP kernel, once per RMVPE object; everything else of RMVPE stays on PyTorch-ROCm.  RVCMI_RMVPE_GRU=0 keeps torch's GRU.
    from .gru import accelerate_f0_rmvpe

    accelerate_f0_rmvpe(r)
    wav = torch.as_tensor(audio_pad)
    with torch.no_grad():
        mel = r.mel_extractor(wav.float().to(r.device).unsqueeze(0), center=True)
        hidden = r._mel2hidden(mel)
    return glue.rmvpe_f0(hidden.squeeze(0).float(), p_len, f0_up_key if on else int(f0_up_key), RMVPE_THRED)


def _rmvpe_batch_f0(self, pads, p_lens, f0_up_key):
    """The f0 of SEVERAL padded inputs in ONE ``RMVPEHIP.f0_batch`` call (a ragged batch: every file comes out as its own ``hip.f0`` call
    gives it, to operand rounding).  None -- nothing computed -- when this f0_gen's RMVPE is not one the kernels serve: the caller keeps the
    per-file calls.  (Whether a group takes this path at all is ``convert_files``' decision.)"""
    from . import rmvpe as _rm

    r = _torch_rmvpe(self)
    hip = _rm.for_generator(self.f0_gen, r) if r is not None else None
    if hip is None:
        return None
    return hip.f0_batch([torch.as_tensor(a).float().to(hip.device) for a in pads], list(p_lens), f0_up_key, RMVPE_THRED)


INDEX_CACHE_ENTRIES = 2  # index files kept resident (a WebUI session alternates between very few voices)
_INDEX_CACHE = {}
_INDEX_CACHE_LOCK = __import__("threading").Lock()  # (the WebUI serves requests from worker threads)


def _open_index(self, file_index, index_rate):
    """pipeline.py:205-218.  -> (IVFFlatHIP or None, needs_reference): ``needs_reference`` = an index kind only real faiss reads
    (not IVF-Flat / L2 ...) while the reference's own pipeline and the real faiss module are bound: the caller hands the whole
    file to that pipeline (retrieval included; its vc calls come back through vc_hip, which passes a non-HIP index on)."""
    import os
    import traceback

    from . import _lib, ivf

    if not (file_index != "" and os.path.exists(file_index) and index_rate != 0):
        return None, False
    try:
        # on THIS pipeline's device (config.device), not the process's current GPU; big_npy is never materialised.
        # The reference re-reads the file on every call (pipeline.py:205-218: faiss.read_index + reconstruct_n); here the parsed index stays
        # resident on the GPU between calls, keyed by (path, size, mtime, device) -- a 10000 x 768 index is 31 MB of file read + upload per
        # call otherwise (round 6, bench.py --e2e: the largest single item around the hot path at one file per call).  RVCMI_INDEX_CACHE=0 turns it off.
        dev = torch.device(self.device)
        st = os.stat(file_index)
        key = (os.path.abspath(file_index), st.st_size, st.st_mtime_ns, str(dev))
        cached = os.environ.get("RVCMI_INDEX_CACHE", "1") != "0"
        if cached:
            with _INDEX_CACHE_LOCK:
                hit = _INDEX_CACHE.get(key)
            if hit is not None:
                return hit, False
        index = ivf.read_index(file_index, device=dev)
        if cached:
            with _INDEX_CACHE_LOCK:
                while len(_INDEX_CACHE) >= INDEX_CACHE_ENTRIES:
                    _INDEX_CACHE.pop(next(iter(_INDEX_CACHE)))  # oldest entry out (dicts keep insertion order)
                _INDEX_CACHE[key] = index
        return index, False
    except _lib.RvcmiError as e:
        orig = getattr(pipeline_hip, "_rvcmi_original", None)
        real = getattr(getattr(_ref_module(self), "faiss", None), "_rvcmi_real", None)
        if e.code == _lib.ERR_IO and orig is not None and real is not None:
            return None, True
        traceback.print_exc()  # the reference prints and converts without an index (pipeline.py:216-218)
        return None, False


def _host_prep(self, audio):
    """pipeline.py:221,241 on the host: -> (the high-passed signal, its ``t_pad`` reflection pad)."""
    import numpy as np

    ref = _ref_module(self)
    audio = ref.signal.filtfilt(ref.bh, ref.ah, audio)
    return audio, np.pad(audio, (self.t_pad, self.t_pad), mode="reflect")


def _prepare_file(self, model, sid, audio, times, f0_up_key, f0_method, if_f0, filter_radius, version, f0_file, collect, prepped=None,
                  host_prepped=None, f0_pair=None):
    """``Pipeline.pipeline`` from its input to the point where a segment would enter ``vc`` (pipeline.py:219-300): high-pass,
    cut points, reflection pad, f0 (RMVPE decoded on the device), then ``collect(audio_segment, pitch_slice, pitchf_slice)`` for
    every segment in order.  -> (the filtered 16 kHz input (``change_rms`` needs it), the number of cuts, its float64 device copy
    when the cut search uploaded one, else None).  ``prepped``: this input's ``_device_prep`` result when the caller prepared a whole
    group in one call; with the device preparation the segments are device slices and the first return value is None.  ``host_prepped``:
    this input's ``_host_prep`` result and ``f0_pair``: its precomputed (pitch, pitchf) when the caller estimated a whole group's f0 in one
    call (``convert_files``); the RMVPE step is then skipped."""
    import traceback
    from time import time

    import numpy as np

    ref = _ref_module(self)
    dev = torch.device(self.device)
    if prepped is None:
        prepped = _device_prep(self, [audio], dev)[0]
    if prepped is not None:
        audio_dev, audio_pad = prepped  # float64 device tensors: the filtered signal and np.pad(.., t_pad, "reflect") of it
        opt_ts, a64 = _file_cuts(self, audio_dev, dev)
        audio, a64 = None, audio_dev
        t1 = time()
    elif host_prepped is not None:
        audio, audio_pad = host_prepped
        opt_ts, a64 = _file_cuts(self, audio, dev)
        t1 = time()
    else:
        audio = ref.signal.filtfilt(ref.bh, ref.ah, audio)
        opt_ts, a64 = _file_cuts(self, audio, dev)
        t1 = time()
        audio_pad = np.pad(audio, (self.t_pad, self.t_pad), mode="reflect")
    p_len = audio_pad.shape[0] // self.window
    inp_f0 = None
    if hasattr(f0_file, "name"):
        try:
            with open(f0_file.name, "r") as f:
                lines = f.read().strip("\n").split("\n")
            if lines and lines[0]:
                inp_f0 = np.array([[float(v) for v in ln.split(",")] for ln in lines], dtype="float32")
        except Exception:  # noqa
            traceback.print_exc()
    pitch = pitchf = None
    if if_f0:
        got = f0_pair
        if got is None and if_f0 == 1 and f0_method == "rmvpe" and inp_f0 is None:
            got = _rmvpe_on_device(self, audio_pad, p_len, f0_up_key)
        if got is not None:
            pitch, pitchf = got[0][:, :p_len].long(), got[1][:, :p_len].float()
        else:
            if if_f0 == 1:
                # a host estimator: the device-prepared signal comes down once (the same signal the segments are cut from)
                pad_np = audio_pad.cpu().numpy() if isinstance(audio_pad, torch.Tensor) else audio_pad
                pitch, pitchf = self.f0_gen.calculate(pad_np, p_len, f0_up_key, f0_method, filter_radius, inp_f0)
            else:
                pitch, pitchf = f0_method  # pipeline.py:268-269: a precomputed (coarse, Hz) pair
            pitch = torch.as_tensor(np.asarray(pitch)[:p_len], device=dev).unsqueeze(0).long()
            pitchf = torch.as_tensor(np.asarray(pitchf)[:p_len].astype(np.float32), device=dev).unsqueeze(0).float()
    times[1] += time() - t1
    w = self.window
    s, t = 0, None
    for t in opt_ts:
        t = t // w * w
        collect(audio_pad[s: t + self.t_pad2 + w], pitch[:, s // w: (t + self.t_pad2) // w] if if_f0 else None,
                pitchf[:, s // w: (t + self.t_pad2) // w] if if_f0 else None)
        s = t
    lo = (t // w) if t is not None else 0
    collect(audio_pad[t:], pitch[:, lo:] if if_f0 else None, pitchf[:, lo:] if if_f0 else None)
    return audio, len(opt_ts), a64


def _finish_file(self, segs, audio, tgt_sr, resample_sr, rms_mix_rate, audio_dev=None):
    """pipeline.py:344-360 on the device: concatenate the trimmed segments, ``change_rms``, (``resample_sr``: host, like the
    reference), int16-range scaling, ONE copy to the host.  ``audio_dev``: the float64 device copy of ``audio`` the cut search
    made, if any; its ``.float()`` is the same single rounding as numpy's ``astype(float32)``, so it is not uploaded again."""
    import numpy as np

    from . import glue

    dev = torch.device(self.device)
    audio_opt = torch.cat([o[self.t_pad_tgt: o.shape[0] - self.t_pad_tgt].float() for o in segs]).contiguous()
    if rms_mix_rate != 1:
        if audio_dev is not None:
            a16 = audio_dev.float()
        else:
            a16 = torch.as_tensor(np.ascontiguousarray(audio, dtype=np.float32), device=dev)
        audio_opt = glue.change_rms(a16, 16000, audio_opt, int(tgt_sr), float(rms_mix_rate))
    if tgt_sr != resample_sr >= 16000:
        # librosa's soxr resampler has no device twin (and no offline oracle): this one option goes through the host like the
        # reference (pipeline.py:351-354) and comes back for the scaling
        host = _ref_module(self).librosa.resample(audio_opt.cpu().numpy(), orig_sr=tgt_sr, target_sr=resample_sr)
        audio_opt = torch.as_tensor(host, device=dev).float().contiguous()
    glue.scale_int16_range(audio_opt)
    return audio_opt.cpu().numpy()


def pipeline_hip(self, model, net_g, sid, audio, times, f0_up_key, f0_method, file_index, index_rate, if_f0, filter_radius, tgt_sr,
                 resample_sr, rms_mix_rate, version, protect, f0_file=None):
    """Drop-in ``Pipeline.pipeline``: same arguments, same numpy return (float array scaled to the int16 range)."""
    import os

    index, needs_ref = _open_index(self, file_index, index_rate)
    if needs_ref:
        return pipeline_hip._rvcmi_original(self, model, net_g, sid, audio, times, f0_up_key, f0_method, file_index, index_rate, if_f0,
                                            filter_radius, tgt_sr, resample_sr, rms_mix_rate, version, protect, f0_file)
    dev = torch.device(self.device)
    sid = torch.tensor(sid, device=dev).unsqueeze(0).long()
    # segments of a long input: one net_g.infer call for all of them when the synthesizer is the HIP one (infer_segments above);
    # RVCMI_PIPELINE_BATCH=0 (or a foreign net_g) keeps the reference's call-per-segment order
    can_batch = _ragged_capable(net_g) and os.environ.get("RVCMI_PIPELINE_BATCH", "1") != "0"
    pending, segs = [], []

    def collect(a0, pt, pf):
        pending.append((a0, pt, pf))

    audio, ncuts, a64 = _prepare_file(self, model, sid, audio, times, f0_up_key, f0_method, if_f0, filter_radius, version, f0_file, collect)
    if can_batch and ncuts > 0:
        from time import time

        t0 = time()
        # (RVCMI_HUBERT_FE + RVCMI_HUBERT_BATCH, opt-in: HuBERT once per group of segments; otherwise the per-segment calls, in this order)
        items = blend_segments(hubert_device_many(self, model, pending, version), index, index_rate, protect)
        times[0] += time() - t0
        segs = infer_segments(net_g, sid, items, times)
    else:
        segs = [vc_device(self, model, net_g, sid, a0, pt, pf, times, index, index_rate, version, protect) for a0, pt, pf in pending]
    return _finish_file(self, segs, audio, tgt_sr, resample_sr, rms_mix_rate, a64)


def convert_files(self, model, net_g, sid, audios, times, f0_up_key, f0_method, file_index, index_rate, if_f0, filter_radius, tgt_sr,
                  resample_sr, rms_mix_rate, version, protect, f0_files=None):
    """``Pipeline.pipeline`` for SEVERAL inputs in one go -- the body of ``VC.vc_multi``'s loop (infer/modules/vc/modules.py:201-266:
    ``load_audio`` + ``vc_single`` -> ``pipeline`` per file of a folder) with the files batched on the GPU:

      1. per file, as ``pipeline`` does it: high-pass (with ``RVCMI_DEVICE_PREP=1``: all files in one device call), cut points (a long
         file's on the device, its own call), f0 (RMVPE on the device), HuBERT per segment.  With the HIP estimator switched on
         (``RVCMI_RMVPE_HIP=1``, off by default), its group switch on (``RVCMI_RMVPE_BATCH=1``; ``rmvpe.RMVPE_BATCH``, off until measured)
         and at least ``rmvpe.RMVPE_BATCH_MIN_FILES`` files without an ``f0_file``, the f0 of those files is ONE ``RMVPEHIP.f0_batch``
         call on the ragged batch of their padded signals, made before the per-file loop;
      2. ONE retrieval call for the HuBERT frames of every segment of every file (``blend_segments``: one coarse pass and one
         list-major scan per ``MAX_BATCH_QUERIES`` frames instead of one per segment);
      3. the segments of all files through ``net_g.infer`` as ragged batches (``infer_segments``, at most ``MAX_BATCH_FRAMES`` padded
         frames per call): a 10 s clip alone fills the chip only in part of the generator (stage 0: 355 tiles on 256 CUs), a batch of
         them does throughout (BASELINE configs[2]);
      4. per file: trim + concatenate, ``change_rms``, scaling, one copy to the host.

    ``audios``: list of 16 kHz float waveforms (``load_audio`` output); the other arguments are ``Pipeline.pipeline``'s, shared by all
    files (``vc_multi`` passes the same sid / f0 method / index / rates for the whole folder); ``f0_files``: None or one entry per
    input.  -> list of numpy arrays in input order.  Every item is computed exactly as its own call would compute it (same noise
    draws in the same order, ragged batch items = separate calls; bit-equal with the shape-dependent kernel choices pinned --
    generator ``RB_STREAM`` / ``NO_RB_SPLIT``, front ``FR_NJ`` / ``FR_FFN_SPLIT`` -- and equal to operand rounding otherwise), so the result does not depend on how the files are grouped.
    One exception, with the device preparation switched on (``RVCMI_DEVICE_PREP=1``, off by default): ``DEVICE_PREP_MIN_SAMPLES`` is judged on the
    audio of the whole call, so a 10 s file is high-passed on the device inside a group and on the host through ``pipeline`` alone; the two
    filters agree to fp64 rounding noise only, which moves about half of the fp32 input samples by one ulp (bit-equal again with the threshold at 0).
    A second one, with the HIP estimator switched on: a file's f0 inside a group equals that of its lone call to operand rounding, not bit for
    bit -- no sequence reads another's frames, but the U-Net layers that split their K loop choose the split from the launch size, which is
    the group's (bit-equal with the group switch off).  A third one, with the HIP feature extractor and its group switch on
    (``RVCMI_HUBERT_FE=1`` and ``RVCMI_HUBERT_BATCH=1``, both off by default) and a model that honours ``padding_mask``
    (``hubert.batch_capable``): the HuBERT features of a segment inside a group equal those of its lone call to operand rounding, not bit for
    bit -- the extractor's rows are bit-equal and no segment attends to another or to padding, but the transformer's GEMMs on torch see
    another M (bit-equal with the group switch off).  A synthesizer that is not the HIP one, or an
    index only real faiss reads, or ``RVCMI_PIPELINE_BATCH=0``, takes the plain per-file loop over ``self.pipeline``."""
    audios = list(audios)
    f0_files = list(f0_files) if f0_files is not None else [None] * len(audios)
    if len(f0_files) != len(audios):
        raise ValueError("f0_files must hold one entry per input")
    if if_f0 == 2 and len(audios) > 1:
        raise ValueError("if_f0 == 2 hands ONE precomputed (pitch, pitchf) pair to the pipeline (pipeline.py:268-269); convert such inputs one by one")
    import os

    index, needs_ref = _open_index(self, file_index, index_rate)
    # RVCMI_PIPELINE_BATCH=0 (the switch pipeline_hip honours for a file's segments) turns cross-file batching off too
    if needs_ref or not _ragged_capable(net_g) or os.environ.get("RVCMI_PIPELINE_BATCH", "1") == "0":
        return [self.pipeline(model, net_g, sid, a, times, f0_up_key, f0_method, file_index, index_rate, if_f0, filter_radius, tgt_sr,
                              resample_sr, rms_mix_rate, version, protect, f) for a, f in zip(audios, f0_files)]
    if len(audios) > MAX_FILES_PER_GROUP:  # bound what is resident at once (HuBERT frames and waveforms of a group); same order, same draws
        res = []
        for lo in range(0, len(audios), MAX_FILES_PER_GROUP):
            res += convert_files(self, model, net_g, sid, audios[lo: lo + MAX_FILES_PER_GROUP], times, f0_up_key, f0_method, file_index, index_rate,
                                 if_f0, filter_radius, tgt_sr, resample_sr, rms_mix_rate, version, protect, f0_files[lo: lo + MAX_FILES_PER_GROUP])
        return res
    from time import time

    dev = torch.device(self.device)
    sid = torch.tensor(sid, device=dev).unsqueeze(0).long()
    raw, owner, filtered = [], [], []
    prepped = _device_prep(self, audios, dev)  # RVCMI_DEVICE_PREP: every file of the group filtered in ONE call (else all None)
    # RVCMI_RMVPE_HIP + RVCMI_RMVPE_BATCH (opt-in): the f0 of every file without an f0_file in ONE ragged RMVPEHIP.f0_batch call instead of one call per file.  It
    # needs each file's padded signal first, so the host preparation of those files moves in front of the loop (same calls, same order).
    host_prepped, f0_pairs = [None] * len(audios), [None] * len(audios)
    if if_f0 == 1 and f0_method == "rmvpe":
        from . import rmvpe as _rm

        todo = [i for i, f in enumerate(f0_files) if not hasattr(f, "name")]
        if _rm.rmvpe_batch_on() and len(todo) >= _rm.RMVPE_BATCH_MIN_FILES:
            for i in todo:
                if prepped[i] is None:
                    host_prepped[i] = _host_prep(self, audios[i])
            pads = [prepped[i][1] if prepped[i] is not None else host_prepped[i][1] for i in todo]
            t1 = time()
            pairs = _rmvpe_batch_f0(self, pads, [p.shape[0] // self.window for p in pads], f0_up_key)
            times[1] += time() - t1
            for i, pair in zip(todo, pairs or ()):
                f0_pairs[i] = pair
    # RVCMI_HUBERT_FE + RVCMI_HUBERT_BATCH (opt-in): the segments are only gathered in the loop and HuBERT runs once per planned group of them behind it
    batch_hubert = hubert_batched(model)
    pending = []
    for i, (a, f0f) in enumerate(zip(audios, f0_files)):
        def collect(a0, pt, pf, i=i):
            t0 = time()
            if batch_hubert:
                pending.append((a0, pt, pf))
            else:
                raw.append(hubert_device(self, model, a0, pt, pf, version))
            owner.append(i)
            times[0] += time() - t0

        got = _prepare_file(self, model, sid, a, times, f0_up_key, f0_method, if_f0, filter_radius, version, f0f, collect, prepped[i],
                            host_prepped[i], f0_pairs[i])
        # (of the device copy only what change_rms reads is kept while the group's other files are prepared)
        filtered.append((got[0], got[2].float() if got[2] is not None and rms_mix_rate != 1 else None))
    t0 = time()
    if batch_hubert:
        raw = hubert_device_many(self, model, pending, version)  # same tuples, same order as the per-segment calls
    items = blend_segments(raw, index, index_rate, protect)
    times[0] += time() - t0
    outs = infer_segments(net_g, sid, items, times)
    res = []
    for i in range(len(audios)):
        res.append(_finish_file(self, [o for o, w in zip(outs, owner) if w == i], filtered[i][0], tgt_sr, resample_sr, rms_mix_rate,
                                filtered[i][1]))
    return res
