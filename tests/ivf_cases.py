"""Small IndexIVFFlat files for the reader tests: well-formed indices with chosen list sizes, and crafted files whose counts lie."""
import struct

import numpy as np


def make_index(n, d, nlist, empty=(), seed=0):
    """An index dict (oracle/ivf_oracle.py layout) of n random rows spread over the lists not named in ``empty``."""
    rng = np.random.default_rng(seed)
    live = np.array([l for l in range(nlist) if l not in empty], dtype=np.int64)
    assign = live[rng.integers(0, len(live), n)] if n else np.zeros(0, np.int64)
    if n >= len(live):
        assign[:len(live)] = live  # every other list holds at least one row
    order = np.argsort(assign, kind="stable")
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(assign, minlength=nlist), out=off[1:])
    xb = rng.standard_normal((n, d)).astype(np.float32)
    return dict(d=d, ntotal=n, nlist=nlist, nprobe=1, centroids=rng.standard_normal((nlist, d)).astype(np.float32), list_offsets=off,
                ids=order.astype(np.int64), vecs=xb[order])


def crafted(d=4, nlist=2, ntotal=3, nlist_stated=None, dm_n=0, tag=b"full", words=(), payload=0):
    """The bytes of an IwFl file with ``nlist`` real centroids whose header fields are free: ``nlist_stated`` (main header, quantizer
    and inverted lists), the direct-map length, the size vector (``tag`` + ``words``) and ``payload`` zero bytes of list data."""
    ns = nlist if nlist_stated is None else nlist_stated
    hdr = lambda nt: struct.pack("<iqqqBi", d, nt, 1 << 20, 1 << 20, 1, 1)
    u64 = lambda v: v % (1 << 64)
    b = b"IwFl" + hdr(ntotal) + struct.pack("<QQ", ns, 1)
    b += b"IxF2" + hdr(ns) + struct.pack("<Q", u64(ns * d)) + bytes(4 * nlist * d)
    b += struct.pack("<bQ", 1 if dm_n else 0, dm_n)
    b += b"ilar" + struct.pack("<QQ", ns, 4 * d)
    b += tag + struct.pack("<Q", len(words)) + b"".join(struct.pack("<Q", u64(w)) for w in words)
    return b + bytes(payload)


# list sizes that sum to ntotal = 3 modulo 2^64: the reader before the size checks allocated 3 rows and read 1600 bytes into them
WRAPPED_SIZES = dict(words=(2 ** 60 + 100, 2 ** 64 - 2 ** 60 - 97), payload=4000)

CRAFTED = {
    "sizes_sum_to_ntotal_mod_2_64": WRAPPED_SIZES,
    "nlist_2_61": dict(nlist_stated=2 ** 61, words=(3, 0), payload=120),
    "list_size_2_63": dict(words=(2 ** 63, 3), payload=120),
    "direct_map_2_61": dict(dm_n=2 ** 61, words=(3, 0), payload=120),
    "odd_sprs_count": dict(tag=b"sprs", words=(0, 3, 1), payload=120),
    "sprs_list_id_is_nlist": dict(tag=b"sprs", words=(2, 3), payload=120),
    "ntotal_minus_1": dict(ntotal=-1, words=(3, 0), payload=120),
}
