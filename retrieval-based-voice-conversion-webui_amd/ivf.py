"""The faiss index object as the reference uses it, backed by the HIP IVF-Flat kernels.

Mirrors exactly the surface the reference touches:

    index = faiss.read_index(path)                 -> read_index(path)            pipeline.py:214
    big_npy = index.reconstruct_n(0, index.ntotal) -> index.reconstruct_n(0, n)   pipeline.py:215
    score, ix = index.search(npy, k=8)             -> index.search(npy, k=8)      pipeline.py:126
    faiss.extract_index_ivf(index).nprobe = 1      -> index.nprobe = 1            web.py:551-552
    faiss.write_index(index, path)                 -> write_index(index, path)    web.py:571
    index = faiss.index_factory(d, "IVF%s,Flat")   -> index_factory(d, "IVF<n>,Flat") web.py:547
    index.train(big_npy); index.add(big_npy[i:j])  -> index.train(x); index.add(x)    web.py:553,561-563

plus the device-resident fast path ``search_blend`` that fuses pipeline.py:126-138 and removes the
two D2H + two H2D hops around retrieval.  numpy in -> numpy out (drop-in); torch.cuda in -> torch.cuda out.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import List, Tuple, Union

import numpy as np
import torch

from . import _lib

ArrayLike = Union[np.ndarray, torch.Tensor]


class IVFFlatHIP:
    def __init__(self, handle: C.c_void_p, device: torch.device, keepalive=None):
        self._h = handle
        self.device = device
        self._keepalive = keepalive  # e.g. the torch tensor that owns a broadcast blob

    # -- construction ----------------------------------------------------------------------------
    @classmethod
    def from_arrays(cls, centroids: np.ndarray, list_offsets: np.ndarray, ids: np.ndarray, vecs: np.ndarray,
                    nprobe: int = 1, device="cuda:0") -> "IVFFlatHIP":
        """What ``index.train(); index.add()`` leave behind (web.py:553-563): centroids [nlist,d],
        list_offsets [nlist+1], and ids [n] / vecs [n,d] in list-major order."""
        dev = _cuda(device)
        cent = np.ascontiguousarray(centroids, dtype=np.float32)
        off = np.ascontiguousarray(list_offsets, dtype=np.int64)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        vecs = np.ascontiguousarray(vecs, dtype=np.float32)
        nlist, d = cent.shape
        n = ids.shape[0]
        if off.shape != (nlist + 1,) or vecs.shape != (n, d):
            raise ValueError("inconsistent IVF arrays")
        h = C.c_void_p(None)
        _lib.check(_lib.lib().rvcmi_ivf_create(d, n, nlist, int(nprobe), cent.ctypes.data_as(C.c_void_p),
                                               off.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p),
                                               vecs.ctypes.data_as(C.c_void_p), _idx(dev), C.byref(h)))
        return cls(h, dev)

    @classmethod
    def train(cls, big_npy: np.ndarray, nlist: int = None, niter: int = 10, seed: int = 1234, device="cuda:0",
              return_objective: bool = False):
        """``index = faiss.index_factory(d, "IVF%s,Flat" % n_ivf); index.train(big_npy); index.add(big_npy)`` (web.py:544-563)
        on the GPU.  ``nlist`` defaults to the reference's ``min(int(16 * sqrt(N)), N // 39)``; ``nprobe`` is 1 (web.py:552).
        ids are the row numbers of ``big_npy`` (sequential ``add``)."""
        dev = _cuda(device)
        x = np.ascontiguousarray(big_npy, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("big_npy must be [N, d]")
        n, d = x.shape
        if nlist is None:
            nlist = max(1, min(int(16 * np.sqrt(n)), n // 39))
        obj = np.zeros(int(niter) + 1, dtype=np.float64)
        h = C.c_void_p(None)
        _lib.check(_lib.lib().rvcmi_ivf_build(d, n, x.ctypes.data_as(C.c_void_p), int(nlist), int(niter), int(seed), _idx(dev),
                                              obj.ctypes.data_as(C.c_void_p) if return_objective else C.c_void_p(None), C.byref(h)))
        idx = cls(h, dev)
        return (idx, obj) if return_objective else idx

    @classmethod
    def trained(cls, big_npy: np.ndarray, nlist: int = None, niter: int = 10, seed: int = 1234, device="cuda:0",
                return_objective: bool = False):
        """``index.train(big_npy)`` alone (web.py:553): the k-means of :meth:`train`, returned as a trained, EMPTY index (what the
        reference writes as ``trained_IVF*.index``); rows come in with :meth:`add`.  Same ``nlist`` default as :meth:`train`;
        ``trained(x, ...)`` followed by ``add(x)`` is :meth:`train`, bit for bit.  The objective has ``niter`` entries (``kmeans``)."""
        dev = _cuda(device)
        x = np.ascontiguousarray(big_npy, dtype=np.float32)
        if x.ndim != 2:
            raise ValueError("big_npy must be [N, d]")
        n, d = x.shape
        if nlist is None:
            nlist = max(1, min(int(16 * np.sqrt(n)), n // 39))
        obj = np.zeros(int(niter), dtype=np.float64)
        h = C.c_void_p(None)
        _lib.check(_lib.lib().rvcmi_ivf_train(d, n, x.ctypes.data_as(C.c_void_p), int(nlist), int(niter), int(seed), _idx(dev),
                                              obj.ctypes.data_as(C.c_void_p) if return_objective else C.c_void_p(None), C.byref(h)))
        idx = IVFFlatHIP(h, dev)
        return (idx, obj) if return_objective else idx

    def add(self, x: ArrayLike) -> None:
        """``index.add(x)`` (web.py:561-563): appends the rows ``x`` [n, d] with ids ``ntotal .. ntotal + n - 1``, each to the list of
        its exact nearest centroid, on the device (``rvcmi_ivf_add``).  A numpy array of any float dtype is converted to fp32 and
        copied up once; a CUDA tensor must be contiguous fp32 on the index's device and is read in place.  Adding in batches gives
        the same index as adding at once.  The index moves to a new blob (``blob()`` copies; an adopted ``from_blob`` tensor is left
        as it was).  Not for use under stream capture."""
        h = self._h
        d = self.d
        if isinstance(x, torch.Tensor):
            if x.device.type != "cuda" or _idx(x.device) != _idx(self.device):
                raise ValueError("add: a tensor must live on the index's device %s (got %s); pass host rows as a numpy array" % (self.device, x.device))
            if x.dtype != torch.float32 or not x.is_contiguous():
                raise ValueError("add: a CUDA tensor must be contiguous float32 (it is read in place)")
            ptr, on_device, keep = x.data_ptr(), 1, x
        else:
            keep = np.ascontiguousarray(x, dtype=np.float32)
            ptr, on_device = keep.ctypes.data, 0
        if keep.ndim != 2 or keep.shape[1] != d:
            raise ValueError("add: rows must be [n, %d], got %s" % (d, tuple(keep.shape)))  # faiss: assert d == self.d
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rvcmi_ivf_add(h, int(keep.shape[0]), C.c_void_p(ptr), on_device, _lib.stream_ptr(self.device)))

    @classmethod
    def from_blob(cls, blob: torch.Tensor) -> "IVFFlatHIP":
        """Adopt a device blob (uint8 CUDA tensor), e.g. one received by an RCCL broadcast."""
        if blob.dtype != torch.uint8 or blob.device.type != "cuda" or not blob.is_contiguous():
            raise ValueError("blob must be a contiguous uint8 CUDA tensor")
        h = C.c_void_p(None)
        _lib.check(_lib.lib().rvcmi_ivf_create_from_blob(_lib.ptr(blob), blob.numel(), _idx(blob.device), 0,
                                                         C.byref(h)))
        return cls(h, blob.device, keepalive=blob)

    def blob(self) -> torch.Tensor:
        """A uint8 CUDA tensor holding a COPY of the whole index (header+centroids+lists)."""
        p, n = C.c_void_p(None), C.c_size_t(0)
        _lib.check(_lib.lib().rvcmi_ivf_blob(self._h, C.byref(p), C.byref(n)))
        out = torch.empty(n.value, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rvcmi_ivf_blob_copy(self._h, _lib.ptr(out), n.value, _lib.stream_ptr(self.device)))
        return out

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                _lib.lib().rvcmi_ivf_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # -- faiss attribute surface -------------------------------------------------------------------
    @property
    def is_trained(self) -> bool:
        return True  # every handle holds centroids (the untrained state exists only in index_factory's object)

    @property
    def ntotal(self) -> int:
        return int(_lib.lib().rvcmi_ivf_ntotal(self._h))

    @property
    def d(self) -> int:
        return int(_lib.lib().rvcmi_ivf_d(self._h))

    @property
    def nlist(self) -> int:
        return int(_lib.lib().rvcmi_ivf_nlist(self._h))

    @property
    def nprobe(self) -> int:
        return int(_lib.lib().rvcmi_ivf_nprobe(self._h))

    @nprobe.setter
    def nprobe(self, v: int) -> None:
        _lib.check(_lib.lib().rvcmi_ivf_set_nprobe(self._h, int(v)))

    def reserve(self, max_nq: int) -> "IVFFlatHIP":
        _lib.check(_lib.lib().rvcmi_ivf_reserve(self._h, int(max_nq)))
        return self

    def centroids(self) -> np.ndarray:
        """The coarse quantizer's centres [nlist, d] (``faiss.extract_index_ivf(index).quantizer.reconstruct_n(0, nlist)``)."""
        out = np.empty((self.nlist, self.d), dtype=np.float32)
        _lib.check(_lib.lib().rvcmi_ivf_centroids(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def reconstruct_n(self, i0: int = 0, n: int = None) -> np.ndarray:
        n = self.ntotal - i0 if n is None else int(n)
        out = np.empty((n, self.d), dtype=np.float32)
        _lib.check(_lib.lib().rvcmi_ivf_reconstruct_n(self._h, int(i0), n, out.ctypes.data_as(C.c_void_p)))
        return out

    def search(self, x: ArrayLike, k: int = 8) -> Tuple[ArrayLike, ArrayLike]:
        """``index.search(x, k)`` -> (D squared-L2 ascending, I int64, -1/FLT_MAX padded)."""
        self._h  # (an untrained index_factory object raises here, before anything is copied)
        is_np = isinstance(x, np.ndarray)
        if is_np:
            if x.dtype != np.float32:
                raise TypeError("queries must be float32 (faiss raises on anything else)")
            xt = torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
        else:
            xt = x.to(self.device, torch.float32).contiguous()
        if xt.dim() != 2 or xt.shape[1] != self.d:
            raise ValueError("queries must be [nq, %d], got %s" % (self.d, tuple(xt.shape)))  # faiss: assert d == self.d
        nq = xt.shape[0]
        D = torch.empty(nq, k, dtype=torch.float32, device=self.device)
        I = torch.empty(nq, k, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rvcmi_ivf_search(self._h, nq, _lib.ptr(xt), int(k), _lib.ptr(D), _lib.ptr(I), _lib.stream_ptr(self.device)))
        if is_np:
            return D.cpu().numpy(), I.cpu().numpy()
        return D, I

    def search_blend(self, feats: torch.Tensor, index_rate: float, k: int = 8, skip_if_short: bool = False) -> torch.Tensor:
        """pipeline.py:126-138 fused on the device; ``feats`` [nq,d] fp32 CUDA is updated IN PLACE and returned.
        ``skip_if_short`` reproduces the realtime guard ``if (ix >= 0).all()`` of rtrvc.py:173."""
        if feats.device.type != "cuda" or feats.dtype != torch.float32 or not feats.is_contiguous():
            raise ValueError("feats must be a contiguous float32 CUDA tensor")
        if feats.dim() != 2 or feats.shape[1] != self.d:
            raise ValueError("feats must be [nq, %d]" % self.d)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().rvcmi_ivf_search_blend(self._h, feats.shape[0], _lib.ptr(feats), float(index_rate), int(k), 1 if skip_if_short else 0,
                                                         _lib.stream_ptr(self.device)))
        return feats

    def set_option(self, key: str, value=None) -> None:
        """Dev / test option of this index (``rvcmi_ivf_set_option``: ``IVF_COARSE_F64``, ``IVF_GENERIC``, ``IVF_LM`` 0 = never the list-major
        kernels, ``IVF_LM_MIN`` their routing threshold in queries (default 16), ``IVF_SORT``); ``None`` = default; an unknown key is an error."""
        _lib.set_option(_lib.lib().rvcmi_ivf_set_option, self._h, key, value)

    def profile(self, enable: bool) -> None:
        _lib.check(_lib.lib().rvcmi_ivf_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self, reset: bool = True) -> List[dict]:
        return _lib.read_stats(_lib.lib().rvcmi_ivf_profile_read, self._h, reset)


def read_index(path: str, device="cuda:0") -> IVFFlatHIP:
    """``faiss.read_index(path)`` for IVF-Flat/L2 files (IwFl)."""
    dev = _cuda(device)
    h = C.c_void_p(None)
    _lib.check(_lib.lib().rvcmi_ivf_create_from_file(str(path).encode(), _idx(dev), C.byref(h)))
    return IVFFlatHIP(h, dev)


def write_index(index: IVFFlatHIP, path: str) -> None:
    """``faiss.write_index(index, path)``."""
    _lib.check(_lib.lib().rvcmi_ivf_write_file(index._h, str(path).encode()))


_SERVED = 'only "IVF<nlist>,Flat" (faiss IndexIVFFlat, METRIC_L2: every index the reference builds, web.py:547) is served'


def parse_description(description: str) -> int:
    """``nlist`` of an ``"IVF<nlist>,Flat"`` factory string; anything else (``"IVF%s,PQ128x4fs,RFlat"`` ...) is a ValueError."""
    m = re.fullmatch(r"IVF([0-9]+),Flat", description) if isinstance(description, str) else None
    if m is None or int(m.group(1)) < 1:
        raise ValueError("index_factory(%r): %s" % (description, _SERVED))
    return int(m.group(1))


class FactoryIVFFlatHIP(IVFFlatHIP):
    """What ``faiss.index_factory(d, "IVF<nlist>,Flat")`` returns: untrained until ``train(x)`` (an instance method here, faiss'
    meaning, unlike the classmethod it shadows), afterwards an ordinary :class:`IVFFlatHIP`.  Untrained, ``is_trained`` is False,
    ``ntotal`` 0, ``d`` / ``nlist`` / ``nprobe`` readable and ``nprobe`` settable (web.py:551-552; carried into the trained index);
    everything that needs centroids raises ``RvcmiError`` ("not trained"), as faiss asserts."""

    def __init__(self, d: int, nlist: int, device="cuda:0", niter: int = 10, seed: int = 1234):
        self._handle = None
        self._d, self._nlist, self._nprobe = int(d), int(nlist), 1
        self.niter, self.seed = int(niter), int(seed)
        super().__init__(None, _cuda(device))

    @property
    def _h(self):
        if self._handle is None:
            raise _lib.RvcmiError("the index is not trained: call index.train(x) first (faiss: 'is_trained' assertion)")
        return self._handle

    @_h.setter
    def _h(self, v):
        self._handle = v

    @property
    def is_trained(self) -> bool:
        return self._handle is not None

    @property
    def ntotal(self) -> int:
        return IVFFlatHIP.ntotal.fget(self) if self.is_trained else 0

    @property
    def d(self) -> int:
        return self._d

    @property
    def nlist(self) -> int:
        return self._nlist

    @property
    def nprobe(self) -> int:
        return IVFFlatHIP.nprobe.fget(self) if self.is_trained else self._nprobe

    @nprobe.setter
    def nprobe(self, v: int) -> None:
        if int(v) < 1:
            raise _lib.RvcmiError("bad nprobe", code=_lib.ERR_INVALID)
        if self.is_trained:
            IVFFlatHIP.nprobe.fset(self, v)
        self._nprobe = int(v)

    def train(self, x: np.ndarray) -> None:  # noqa  (faiss' instance method; IVFFlatHIP.train is the one-shot classmethod)
        """``index.train(x)``: k-means for the ``nlist`` centroids (``rvcmi_ivf_train``); needs at least ``nlist`` rows.  A second call
        is a no-op, as in faiss."""
        if self.is_trained:
            return
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self._d:
            raise ValueError("train: rows must be [n, %d], got %s" % (self._d, tuple(x.shape)))
        if x.shape[0] < self._nlist:
            raise _lib.RvcmiError("train: need at least nlist=%d training vectors, got %d" % (self._nlist, x.shape[0]), code=_lib.ERR_INVALID)
        h = C.c_void_p(None)
        _lib.check(_lib.lib().rvcmi_ivf_train(self._d, x.shape[0], x.ctypes.data_as(C.c_void_p), self._nlist, self.niter, self.seed,
                                              _idx(self.device), C.c_void_p(None), C.byref(h)))
        self._handle = h
        if self._nprobe != 1:
            IVFFlatHIP.nprobe.fset(self, self._nprobe)


def index_factory(d: int, description: str, device="cuda:0") -> FactoryIVFFlatHIP:
    """``faiss.index_factory(d, "IVF%s,Flat" % n_ivf)`` (web.py:547, tools/cmd/train-index{,-v2}.py): an untrained IVF-Flat / L2 index."""
    nlist = parse_description(description)
    if int(d) < 4 or int(d) % 4:
        raise ValueError("index_factory: dimension %s must be a positive multiple of 4" % (d,))
    return FactoryIVFFlatHIP(int(d), nlist, device=device)


def extract_index_ivf(index: IVFFlatHIP) -> IVFFlatHIP:
    """``faiss.extract_index_ivf(index)``: the index itself (the reference only sets ``.nprobe`` on it, web.py:551-552)."""
    if not isinstance(index, IVFFlatHIP):
        raise TypeError("extract_index_ivf: not an rvc_amd index: %r" % (type(index),))
    return index


def _cuda(device) -> torch.device:
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.RvcmiError("the HIP IVF index needs a GPU device (got %s); there is no CPU fallback" % device)
    return dev


def _idx(dev: torch.device) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def reduce_features(big_npy: np.ndarray, n_clusters: int = 10000, threshold: float = 2e5, niter: int = 10, seed: int = 1234,
                    device="cuda:0") -> np.ndarray:
    """The training-set reduction of web.py:522-536: more than 2e5 feature rows are replaced by ``n_clusters`` k-means
    centres before the index is trained.  The reference runs sklearn's ``MiniBatchKMeans(init="random")`` on the host
    (stochastic mini-batches, its own RNG: not reproducible elsewhere); this runs full-batch Lloyd iterations on the GPU with
    the exact coarse-assignment kernels of the search path (same objective, lower final inertia).  Smaller sets are returned
    unchanged, like the reference's ``if big_npy.shape[0] > 2e5``."""
    x = np.ascontiguousarray(big_npy, dtype=np.float32)
    if x.shape[0] <= threshold:
        return x
    return kmeans(x, int(n_clusters), niter=niter, seed=seed, device=device)


def kmeans(x: np.ndarray, k: int, niter: int = 10, seed: int = 1234, device="cuda:0") -> np.ndarray:
    """``k`` k-means centres of the rows of ``x`` (``rvcmi_kmeans``): the Lloyd iterations of :meth:`IVFFlatHIP.train` without the
    index -- no ``add`` pass over the N rows, no list-major copy in HBM.  A cluster that loses all its points is re-seeded by
    splitting the largest one, so all ``k`` rows returned are usable centres (not necessarily distinct: an all-zero centre cannot be split)."""
    dev = _cuda(device)
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("x must be [N, d]")
    n, d = x.shape
    out = np.empty((int(k), d), dtype=np.float32)
    _lib.check(_lib.lib().rvcmi_kmeans(d, n, x.ctypes.data_as(C.c_void_p), int(k), int(niter), int(seed), _idx(dev), C.c_void_p(None),
                                       out.ctypes.data_as(C.c_void_p)))
    return out


def train_index(big_npy: np.ndarray, path: str = None, nlist: int = None, niter: int = 10, seed: int = 1234, device="cuda:0") -> IVFFlatHIP:
    """The index recipe of web.py:544-571 (``train`` + ``add`` + optional ``write_index``) on the GPU."""
    idx = IVFFlatHIP.train(big_npy, nlist=nlist, niter=niter, seed=seed, device=device)
    if path is not None:
        write_index(idx, path)
    return idx
