"""TEST INFRASTRUCTURE ONLY -- the index build (csrc/ivf_kmeans.hpp + the loop of ``ivf_build_impl`` in csrc/ivf.hip) step by step in
numpy fp64: which function of (x, nlist, niter, seed) the built index is.

One function per published step, and ``build`` that strings them together the way the device loop does.  What is bit-exact and what is not:

* Centroids have no liberty.  A mean is the fp64 sum of the list's rows in ascending id order (strictly sequential), one division, one
  rounding to fp32; a split centre is an fp32 product; a relocated centre is a copy of a training row.  They are compared bit for bit.
* Distances are NOT imitated (the device sums lane-strided partials through an xor butterfly, with a contractible multiply-add).  Every
  decision that hangs on a distance instead reports its relative margin, and a case is admissible only when each margin is exactly 0 (an
  exact tie of two sums with equal terms, resolved by id) or at least ``MARGIN`` = 1e-9, seven orders above fp64 summation noise.
  ``admissible(report)`` is that condition; it is a condition on the inputs, asserted on the CPU for every case of tests/ivf_build_cases.py.

``variant`` names one deliberately wrong restatement (``VARIANTS``): the tests require each of them to change the final centroids of at
least one case of the table, so that the table cannot go blind to that kind of device bug.
"""
from __future__ import annotations

import math

import numpy as np

MARGIN = 1e-9
M64 = (1 << 64) - 1
VARIANTS = ("mean_drops_last_row", "mean_in_fp32", "assign_ties_high", "split_keeps_sizes", "no_moved_rule", "relocate_one_more",
            "relocation_inputs_nudged", "nearest_ties_high")


# ---- seed rows: xorshift64* partial Fisher-Yates, python integers mod 2^64 ----
def seed_rows(n: int, nlist: int, seed: int) -> list:
    perm = list(range(n))
    sd = (seed * 6364136223846793005 + 1442695040888963407) & M64
    for i in range(nlist):
        sd ^= sd >> 12
        sd ^= (sd << 25) & M64
        sd ^= sd >> 27
        r = ((sd * 2685821657736338717) & M64) % (n - i)
        perm[i], perm[i + r] = perm[i + r], perm[i]
    return perm[:nlist]


def _rel(a: float, b: float) -> float:
    """relative distance of two non-negative numbers; 0 = equal (inf == inf included)"""
    if a == b:
        return 0.0
    return abs(a - b) / max(abs(a), abs(b))


def _direct(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    t = a.astype(np.float64) - b.astype(np.float64)
    return np.einsum("ij,ij->i", t, t)


# ---- assignment: exact fp64 argmin of sum((x - c)^2), ties -> lowest list ----
def assign(x: np.ndarray, cent: np.ndarray, ties_high: bool = False, rows_per_chunk: int = 2048):
    """-> (assign [n] int64, dist [n] fp64 to the winner, facts).  The fp64 expansion |x|^2 + |c|^2 - 2xc only prefilters: every centre
    within 1e-6 relative (plus 1e-11 of |x|^2 + max|c|^2, far above the expansion's own error) of the best is evaluated again by direct
    differences, and the winner, the tie count and the margin come from those.  facts: ties = rows whose two best distances are exactly
    equal, ties_unequal = those among them whose two sums differ in some term, |x_e - c_e| (never admissible: such a tie is an accident of
    the summation order; with equal terms every order gives equal sums -- bit-identical centres, or the two halves of a split around a
    row that equals the split centre), margin = the smallest relative gap (d2 - d1) / d2 of the other rows."""
    n, k = x.shape[0], cent.shape[0]
    x64, c64 = x.astype(np.float64), cent.astype(np.float64)
    cn = np.einsum("ij,ij->i", c64, c64)
    cnmax = float(cn.max())
    out = np.empty(n, np.int64)
    dist = np.empty(n, np.float64)
    ties = ties_unequal = 0
    margin = math.inf
    for s in range(0, n, rows_per_chunk):
        xs = x64[s:s + rows_per_chunk]
        m = xs.shape[0]
        xn = np.einsum("ij,ij->i", xs, xs)
        E = xn[:, None] + cn[None, :] - 2.0 * (xs @ c64.T)
        emin = E.min(axis=1)
        thr = emin + 1e-6 * np.abs(emin) + 1e-11 * (xn + cnmax)
        ri, ci = np.nonzero(E <= thr[:, None])
        dd = _direct(xs[ri], c64[ci])
        order = np.lexsort((-ci if ties_high else ci, dd, ri))
        ri, ci, dd = ri[order], ci[order], dd[order]
        first = np.flatnonzero(np.r_[True, ri[1:] != ri[:-1]])
        assert first.shape[0] == m
        out[s:s + m] = ci[first]
        dist[s:s + m] = dd[first]
        if k < 2:
            continue
        cnt = np.diff(np.r_[first, ri.shape[0]])
        multi = first[cnt > 1]
        d1, d2 = dd[multi], dd[multi + 1]
        tie = d1 == d2
        ties += int(tie.sum())
        tr, ta, tb = ri[multi[tie]], ci[multi[tie]], ci[multi[tie] + 1]
        ties_unequal += int((np.abs(xs[tr] - c64[ta]) != np.abs(xs[tr] - c64[tb])).any(axis=1).sum())
        if (~tie).any():
            margin = min(margin, float(((d2[~tie] - d1[~tie]) / d2[~tie]).min()))
        single = np.flatnonzero(cnt == 1)  # (the runner-up lies outside the verified band: its gap is the expansion's, >= 1e-6)
        if single.size:
            e2 = np.partition(E[single], 1, axis=1)[:, 1]
            margin = min(margin, float(((e2 - emin[single]) / np.maximum(e2, 1e-300)).min()))
    return out, dist, dict(ties=ties, ties_unequal=ties_unequal, margin=margin)


# ---- lists: stable counting sort ----
def lists(assign_: np.ndarray, nlist: int):
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.bincount(assign_, minlength=nlist), out=off[1:])
    order = np.argsort(assign_, kind="stable").astype(np.int64)
    return off, order


# ---- mean: fp64, ascending ids, strictly sequential; one division; one rounding to fp32.  Empty lists keep ``prev`` ----
def means(x: np.ndarray, off: np.ndarray, order: np.ndarray, prev: np.ndarray, variant: str = None) -> np.ndarray:
    nlist, d = prev.shape
    size = np.diff(off)
    acc_t = np.float32 if variant == "mean_in_fp32" else np.float64
    xs = x.astype(acc_t)
    acc = np.zeros((nlist, d), acc_t)
    last = size - 1 if variant == "mean_drops_last_row" else size
    for t in range(int(last.max(initial=0))):  # step t adds the t-th row of every list that has one: sequential inside each list
        sel = np.flatnonzero(last > t)
        acc[sel] += xs[order[off[sel] + t]]
    cent = prev.copy()
    ne = size > 0
    cent[ne] = (acc[ne] / size[ne, None].astype(acc_t)).astype(np.float32)
    return cent


# ---- split of empty lists: the largest list's centre, nudged apart by fp32 products v * (1 +- 2^-10) in alternating coordinates ----
def split_empty(cent: np.ndarray, off: np.ndarray, variant: str = None):
    """-> (cent after the split, the (empty list, list it was split from) pairs).  The running sizes follow the header: the new list takes
    half of the split one's rows (rounded down), so the next empty list splits what is largest THEN."""
    cent = cent.copy()
    sz = np.diff(off).copy()
    eps = np.float32(1.0 / 1024.0)
    up, dn = np.float32(1.0) + eps, np.float32(1.0) - eps
    odd = (np.arange(cent.shape[1]) & 1).astype(bool)
    pairs = []
    for l in range(sz.shape[0]):
        if sz[l]:
            continue
        big = int(np.argmax(sz))  # first maximum, as std::max_element
        v = cent[big].copy()
        cent[l] = np.where(odd, v * dn, v * up)
        cent[big] = np.where(odd, v * up, v * dn)
        pairs.append((l, big))
        if variant != "split_keeps_sizes":
            sz[l] = sz[big] // 2
            sz[big] -= sz[l]
    return cent, pairs


# ---- relocation inputs ----
def assigned_dist(x: np.ndarray, cent: np.ndarray, assign_: np.ndarray) -> np.ndarray:
    return _direct(x, cent[assign_])


def nearest_two(cent: np.ndarray, ties_high: bool = False):
    """-> (nn2 [nlist, 2]: the two nearest centres of every centre, itself among them, ascending (distance, id); the smallest relative gap
    between the second and the third that is not an exact tie; the count of exact ties whose two sums differ in some term)"""
    k = cent.shape[0]
    c64 = cent.astype(np.float64)
    nn2 = np.empty((k, 2), np.int64)
    margin, unequal = math.inf, 0
    ids = np.arange(k)
    for l in range(k):
        dd = _direct(c64, c64[l:l + 1])
        o = np.lexsort((-ids if ties_high else ids, dd))
        nn2[l] = o[:2]
        if k > 2:
            a, b = float(dd[o[1]]), float(dd[o[2]])
            if a != b:
                margin = min(margin, (b - a) / b)
            elif (np.abs(c64[l] - c64[o[1]]) != np.abs(c64[l] - c64[o[2]])).any():
                unequal += 1
    return nn2, margin, unequal


# ---- relocation (kmeans_relocate) ----
def relocate(x: np.ndarray, dist: np.ndarray, nn2: np.ndarray, off: np.ndarray, order: np.ndarray, cent: np.ndarray, variant: str = None):
    """-> (cent with the moved centres overwritten, report).  ``dist`` and ``nn2`` are the caller's (the build hands in those of the
    un-nudged means); the costs are computed here from ``cent`` (the build hands in the nudged host centres)."""
    nlist, d = cent.shape
    cent = cent.copy()
    c64 = cent.astype(np.float64)
    size = np.diff(off)
    S = np.zeros(nlist)
    cost = np.full(nlist, math.inf)
    nn = np.full(nlist, -1, np.int64)
    for l in range(nlist):
        for p in range(off[l], off[l + 1]):
            S[l] += dist[order[p]]
        if not size[l]:
            continue
        o = int(nn2[l, 1] if nn2[l, 0] == l else nn2[l, 0])
        if o < 0 or o == l or not size[o]:
            continue
        t = c64[l] - c64[o]
        nn[l] = o
        cost[l] = float(size[l]) * float(np.dot(t, t))
    ids = np.arange(nlist)
    by_cost = np.lexsort((ids, cost))
    by_S = np.lexsort((ids, -S))
    used = np.zeros(nlist, bool)
    moved = np.zeros(nlist, bool)
    maxmoves = max(1, nlist // 20)
    rep = dict(moves=[], skip_used=0, skip_moved=0, skip_other=0, cursor_diff=0, brk="end", maxmoves=maxmoves,
               margin_far=math.inf, margin_gain=math.inf, margin_sort=math.inf)
    si = 0
    last_ci, last_sj = -1, -1
    for ci in range(nlist):
        if len(rep["moves"]) >= maxmoves:
            rep["brk"] = "cap"
            break
        last_ci = ci
        j = int(by_cost[ci])
        if used[j]:
            rep["skip_used"] += 1
            continue
        if nn[j] < 0 or not cost[j] < math.inf:
            rep["skip_other"] += 1
            continue
        if moved[nn[j]] and variant != "no_moved_rule":
            rep["skip_moved"] += 1
            continue
        while si < nlist and (used[by_S[si]] or size[by_S[si]] < 2):
            si += 1
        sj = si
        while sj < nlist and (used[by_S[sj]] or by_S[sj] == j or by_S[sj] == nn[j] or size[by_S[sj]] < 2):
            sj += 1
        if sj >= nlist:
            rep["brk"] = "sj"
            break
        rep["cursor_diff"] += int(sj != si)
        last_sj = max(last_sj, sj)
        o = int(by_S[sj])
        rows = order[off[o]:off[o + 1]]
        dr = dist[rows]
        far = int(rows[int(np.argmax(dr))])  # first maximum: the lowest id among equals
        top = np.unique(dr)
        if top.shape[0] > 1:
            rep["margin_far"] = min(rep["margin_far"], _rel(float(top[-1]), float(top[-2])))
        gain = 0.0
        for g in np.maximum(0.0, dr - _direct(x[rows], x[far:far + 1])):
            gain += float(g)
        if gain != cost[j]:
            rep["margin_gain"] = min(rep["margin_gain"], _rel(gain, float(cost[j])))
        if not gain > cost[j]:
            rep["brk"] = "gain"
            break
        cent[j] = x[far]
        used[j] = used[o] = used[nn[j]] = True
        moved[j] = True
        rep["moves"].append((j, far))
    else:
        if len(rep["moves"]) >= maxmoves:
            rep["brk"] = "cap"
    # neighbouring entries of the two orders, as far as the loop consulted them (one past the last entry it read)
    for a in range(min(last_ci + 1, nlist - 1)):
        m = _rel(float(cost[by_cost[a]]), float(cost[by_cost[a + 1]]))
        if m:
            rep["margin_sort"] = min(rep["margin_sort"], m)
    for a in range(min(last_sj + 1, nlist - 1)):
        m = _rel(float(S[by_S[a]]), float(S[by_S[a + 1]]))
        if m:
            rep["margin_sort"] = min(rep["margin_sort"], m)
    return cent, rep


def update(x: np.ndarray, cent: np.ndarray, assign_: np.ndarray, relocating: bool, variant: str = None):
    """One pass of the loop body after the assignment: lists -> means -> split -> relocation.  -> (new centres, report).

    The relocation's inputs are NOT taken from one set of centres, and this restates what ``ivf_build_impl`` does today: the distances of
    the rows and the two nearest centres come from the device's copy of the new means, which the host's split has not touched (an empty list
    still holds its previous centre there), while the costs inside the relocation come from the host centres after the split."""
    nlist = cent.shape[0]
    off, order = lists(assign_, nlist)
    mean = means(x, off, order, cent, variant)
    host, pairs = split_empty(mean, off, variant)
    rep = dict(splits=len(pairs), split_pairs=pairs, sizes=np.diff(off))
    if relocating:
        src = host if variant == "relocation_inputs_nudged" else mean
        dist = assigned_dist(x, src, assign_)
        nn2, m_nn, uneq = nearest_two(src, ties_high=variant == "nearest_ties_high")
        host, r = relocate(x, dist, nn2, off, order, host, variant)
        rep.update(r, margin_nn=m_nn, nn_ties_unequal=uneq)
    else:
        rep.update(moves=[], skip_used=0, skip_moved=0, skip_other=0, cursor_diff=0, brk=None)
    return host, rep


def build(x: np.ndarray, nlist: int, niter: int, seed: int, centres_only: bool = False, variant: str = None) -> dict:
    """``rvcmi_ivf_build`` (``centres_only``: ``rvcmi_kmeans`` / ``rvcmi_ivf_train`` -- niter updates, no final assignment).
    -> centroids [nlist, d] fp32, objective (niter + 1 entries, niter when centres_only), list_offsets / ids (None when centres_only),
    report: one dict per iteration."""
    assert variant is None or variant in VARIANTS, variant
    x = np.ascontiguousarray(x, np.float32)
    n, d = x.shape
    seeds = seed_rows(n, nlist, seed)
    cent = x[seeds].copy()
    objective, report = [], []
    a = None
    for it in range(niter + 1):
        if centres_only and it == niter:
            break
        a, dist, facts = assign(x, cent, ties_high=variant == "assign_ties_high")
        objective.append(math.fsum(dist.tolist()))
        if it == niter:
            report.append(dict(final=True, **facts))
            break
        lim = 2 if variant == "relocate_one_more" else 3
        cent, rep = update(x, cent, a, relocating=it + lim < niter and nlist >= 2, variant=variant)
        rep.update(facts, final=False)
        report.append(rep)
    out = dict(centroids=cent, objective=np.array(objective), seeds=seeds, report=report, list_offsets=None, ids=None)
    if not centres_only:
        out["list_offsets"], out["ids"] = lists(a, nlist)
    return out


def margins(rep: dict) -> dict:
    return {k: v for k, v in rep.items() if k.startswith("margin")}


def smallest_margin(report: list) -> float:
    return min([v for r in report for v in margins(r).values()] + [math.inf])


def admissible(report: list) -> bool:
    """every distance-dependent decision of the run is an exact tie between identical operands or at least MARGIN clear"""
    return all(r.get("ties_unequal", 0) == 0 and r.get("nn_ties_unequal", 0) == 0 for r in report) and smallest_margin(report) >= MARGIN
