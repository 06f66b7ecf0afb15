"""Cases for the nprobe > 1 path of the IVF search (k_coarse_dist + k_coarse_select, then the query-major scan with its probe loop) on
the three scan kernels, shared by tests/test_cpu_ivf_probe.py (the cases on the oracle alone) and tests/test_gpu_ivf_probe.py.

One index per kernel, oracle/ivf_oracle.py layout, with CHOSEN list sizes around the row-loop step of that kernel (G row groups x RU
rows in flight):

    d = 256   k_scan_v<4,16,2>   32 rows per pipeline step
    d = 768   k_scan_v<6,32,2>   16
    d =  64   k_scan (generic)   16

Unlike ``_tiny_index`` of test_gpu_ivf.py the centroids are close (scale 1.5, row spread 1.0), so the 2nd to 9th nearest lists
supply results.  Every index carries one row planted three times, bit for bit (inside its own list and in a second list, under
different ids), and query 0 equals it: distance 0 and a tie, the lowest id first.

Everything is seeded, built without a GPU, cached and handed out read-only."""
import functools

import numpy as np

from oracle import ivf_oracle

STEP = {256: 32, 768: 16, 64: 16}  # rows per pipeline step of the scan kernel that serves d
DIMS = (256, 768, 64)
KS = (8, 5, 1)
NQ = 48
SMALL = (0, 0, 2, 3, 4, 5, 6, 7, 9, 11)  # two empty lists and a handful of short ones: the 9 shortest lists still hold 28 rows >= k
SEED = {256: 256, 768: 768, 64: 1}  # (64: with seed 64 the planted row's second nearest list is an empty one; test_cpu_ivf_probe.py checks)


def margin(d):
    """Four times the standard relative bound (d + 2) u on a d-term fp64 sum of squared fp32 differences, u = 2^-53: two fp64 values
    closer than this could legitimately be ranked, or rounded to fp32, differently by another summation order."""
    return 4.0 * (d + 2) * 2.0 ** -53


def list_sizes(d):
    s = STEP[d]
    return (1, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, 3 * s + 1, 4 * s, 4 * s + 1) + SMALL


def nprobes(nlist):
    return (1, 2, 9, nlist, nlist + 3)


def _freeze(idx):
    for v in idx.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return idx


def _layout(sizes, d, rng, scale=1.5, spread=1.0):
    sizes = np.asarray(sizes, np.int64)
    nlist = len(sizes)
    cent = (scale * rng.standard_normal((nlist, d))).astype(np.float32)
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    n = int(off[-1])
    lab = np.repeat(np.arange(nlist), sizes)
    vecs = (cent[lab] + spread * rng.standard_normal((n, d))).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    return dict(d=d, ntotal=n, nlist=nlist, nprobe=1, centroids=cent, list_offsets=off, ids=ids, vecs=vecs)


@functools.lru_cache(maxsize=None)
def probe_case(d):
    """-> (index, queries [NQ, d], planted): ``planted`` = dict(list_a, list_b, pos (the three row positions), ids (ascending))."""
    rng = np.random.default_rng(SEED[d])
    sizes = np.asarray(list_sizes(d), np.int64)[rng.permutation(len(list_sizes(d)))]  # the size classes in a seeded list order
    idx = _layout(sizes, d, rng)
    cent, off, vecs, ids = idx["centroids"], idx["list_offsets"], idx["vecs"], idx["ids"]
    nlist = idx["nlist"]
    # the planted row: the LAST row of the longest list (4 step + 1 rows: alone in the fifth pipeline step), copied into the first
    # step of its own list and over the last row of the list whose centroid is its second nearest (a different, non-empty list)
    a = int(np.argmax(sizes))
    pa = int(off[a + 1]) - 1
    x = vecs[pa].copy()
    order = ivf_oracle.coarse_assign(idx, x[None], nlist)[0]
    b = int([l for l in order if l != a and sizes[l] >= 2][0])
    pb, pc = int(off[b + 1]) - 1, int(off[a]) + 3
    vecs[pb] = x
    vecs[pc] = x
    # ids against the scan order: the copy a scan meets first carries the highest id of the three
    lo, mid, hi = sorted(int(ids[p]) for p in (pa, pb, pc))
    ids[pb], ids[pa], ids[pc] = lo, mid, hi
    # 40 queries next to the centroids, two per list (every size class, the empty lists included), and 8 between a long list and
    # another one, so that two probed lists supply a result in alternation
    pick = np.arange(40) % nlist
    q = cent[pick] + 0.7 * rng.standard_normal((40, d))
    longs = np.argsort(-sizes)[:8]
    other = (longs + 1 + rng.integers(0, nlist - 1, 8)) % nlist
    q2 = 0.5 * (cent[longs] + cent[other]) + 0.7 * rng.standard_normal((8, d))
    q = np.concatenate([q, q2]).astype(np.float32)
    q[0] = x
    q.setflags(write=False)
    return _freeze(idx), q, dict(list_a=a, list_b=b, pos=(pa, pb, pc), ids=(lo, mid, hi))


def with_nprobe(idx, nprobe):
    """The same arrays under another stored nprobe (``ivf_oracle.search_blend`` reads it from the dict)."""
    out = dict(idx)
    out["nprobe"] = int(nprobe)
    return out


@functools.lru_cache(maxsize=None)
def expected(d, nprobe):
    """The oracle's (D, I) at k = 8 for the 48 queries; a smaller k is the leading columns."""
    idx, q, _ = probe_case(d)
    D, I = ivf_oracle.search(idx, q, 8, nprobe=nprobe)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


# ---- the coarse cut: two bit-identical centroids at rank nprobe and nprobe + 1 of query 0 -------------------------------------------
CUT_STRADDLE, CUT_INSIDE = 3, 4  # nprobe: the tie straddles the cut / both lists are probed


@functools.lru_cache(maxsize=None)
def cut_case(d):
    """-> (index, queries [6, d], info): centroids ``a < b`` are the same bits and sit at ranks 3 and 4 of query 0; list ``b`` holds the
    row nearest to query 0 (id ``near_id``).  At nprobe 3 list a is probed and b is not; at nprobe 4 both are."""
    rng = np.random.default_rng(1000 + d)
    s = STEP[d]
    idx = _layout((9, s + 1, 12, 2 * s + 1, 10, 17, 8, s, 11, 13, 3 * s + 1, 15), d, rng)
    cent, off, vecs, ids = idx["centroids"], idx["list_offsets"], idx["vecs"], idx["ids"]
    nlist = idx["nlist"]
    pick = rng.permutation(nlist)[:6]
    q = (cent[pick] + 0.7 * rng.standard_normal((6, d))).astype(np.float32)
    order = ivf_oracle.coarse_assign(idx, q[:1], nlist)[0]
    x, y = int(order[CUT_STRADDLE - 1]), int(order[CUT_STRADDLE])
    cent[y] = cent[x]  # y moves in to x's distance: still behind ranks 1-2 and ahead of rank 5
    a, b = min(x, y), max(x, y)
    pn = int(off[b]) + 1
    vecs[pn] = (q[0] + 0.05 * rng.standard_normal(d)).astype(np.float32)
    q.setflags(write=False)
    return _freeze(idx), q, dict(a=a, b=b, near_pos=pn, near_id=int(ids[pn]))


# ---- nprobe changing on a handle that has searched (the 256-d index) ---------------------------------------------------------------
# (nprobe, nq) in order; "reserve" = one reserve(1000) with the NEXT step's nprobe already set
TRANSITIONS = ((1, 128), (9, 20), (1, 128), (3, 300), (9, 300), (1, 10), "reserve", (2, 600), (1, 600))
RESERVE_NQ = 1000


@functools.lru_cache(maxsize=None)
def transition_queries():
    """600 queries next to the centroids of the 256-d index; step (nprobe, nq) searches the first nq of them."""
    idx, _, _ = probe_case(256)
    rng = np.random.default_rng(600)
    pick = rng.integers(0, idx["nlist"], 600)
    q = (idx["centroids"][pick] + 0.7 * rng.standard_normal((600, 256))).astype(np.float32)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def transition_expected(nprobe):
    """The oracle's (D, I) at k = 8 for all 600 queries (results are per query: a step takes the leading rows)."""
    idx, _, _ = probe_case(256)
    D, I, _ = ivf_oracle.search_c(idx, transition_queries(), 8, nprobe=nprobe)
    D.setflags(write=False)
    I.setflags(write=False)
    return D, I


# ---- the conditions under which exact equality with the oracle is the right bar ----------------------------------------------------

def merged_candidates(idx, qrow, nprobe):
    """All rows of the ``nprobe`` nearest lists of one query -> (fp64 distances, ids), ascending (distance, id)."""
    lists = ivf_oracle.coarse_assign(idx, qrow[None], min(nprobe, idx["nlist"]))[0]
    off = idx["list_offsets"]
    pos = np.concatenate([np.arange(off[l], off[l + 1]) for l in lists] + [np.zeros(0, np.int64)]).astype(np.int64)
    diff = idx["vecs"][pos].astype(np.float64) - qrow.astype(np.float64)[None, :]
    dist = np.einsum("ij,ij->i", diff, diff)
    o = np.lexsort((idx["ids"][pos], dist))
    return dist[o], idx["ids"][pos][o]


def centroid_distances(idx, qrow):
    """fp64 distances of one query to every centroid, ascending (distance, id)."""
    diff = idx["centroids"].astype(np.float64) - qrow.astype(np.float64)[None, :]
    dist = np.einsum("ij,ij->i", diff, diff)
    return dist[np.lexsort((np.arange(len(dist)), dist))]


def midpoint_margin(x):
    """Relative distance of the positive fp64 values ``x`` to the nearest fp32 rounding boundary (the midpoint of two neighbouring fp32)."""
    x = np.asarray(x, np.float64)
    f = x.astype(np.float32)
    lo = (f.astype(np.float64) + np.nextafter(f, np.float32(-np.inf)).astype(np.float64)) / 2
    hi = (f.astype(np.float64) + np.nextafter(f, np.float32(np.inf)).astype(np.float64)) / 2
    return np.minimum(np.abs(x - lo), np.abs(x - hi)) / x


def exactness_report(idx, q, nprobe, k=8):
    """What the conditions of tests/test_cpu_ivf_probe.py are checked on, over all queries: the smallest relative gap between
    neighbouring UNEQUAL distances among the first k + 1 merged candidates, the smallest midpoint margin of the first k, the smallest
    relative gap between UNEQUAL centroid distances at the cut (inf when every list is probed), and how many neighbouring pairs /
    cuts are exact ties."""
    gap = mid = cut = np.inf
    ties = cut_ties = 0
    for i in range(q.shape[0]):
        dist, _ = merged_candidates(idx, q[i], nprobe)
        head = dist[:k + 1]
        if len(head) > 1:
            lo, hi = head[:-1], head[1:]
            ne = hi != lo
            ties += int((~ne).sum())
            if ne.any():
                gap = min(gap, float(((hi - lo)[ne] / hi[ne]).min()))
        pos = dist[:k][dist[:k] > 0]
        if len(pos):
            mid = min(mid, float(midpoint_margin(pos).min()))
        if nprobe < idx["nlist"]:
            cd = centroid_distances(idx, q[i])
            if cd[nprobe] == cd[nprobe - 1]:
                cut_ties += 1
            else:
                cut = min(cut, float((cd[nprobe] - cd[nprobe - 1]) / cd[nprobe]))
    return dict(gap=gap, mid=mid, cut=cut, ties=ties, cut_ties=cut_ties)
