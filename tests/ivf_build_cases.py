"""The table of index builds that tests/test_cpu_ivf_build.py (admissibility, non-vacuity, wrong variants) and tests/test_gpu_ivf_build.py
(device against oracle/ivf_build_oracle.py, bit for bit) share, and what each case is there for.

Every case names the facts of the oracle's report it must show (``must``): the CPU suite asserts them, so no case can go vacuous when
someone changes a shape or a seed.  Seeds marked "searched" were found by running the oracle over seeds on the CPU until the fact held.
"Blobs" = centres sep * N(0, 1) plus unit Gaussian noise, rows drawn with numpy's default_rng.
"""
from functools import lru_cache

import numpy as np

from oracle import ivf_build_oracle as bo


def blobs(nb, d, n, sep, rs):
    rng = np.random.default_rng(rs)
    c = sep * rng.standard_normal((nb, d))
    return (c[rng.integers(0, nb, n)] + rng.standard_normal((n, d))).astype(np.float32)


def repeated(distinct, times, d, rs):
    return np.repeat(np.random.default_rng(rs).standard_normal((distinct, d)).astype(np.float32), times, axis=0)


def zeros_and_others(rs):
    rng = np.random.default_rng(rs)
    x = np.zeros((200, 8), np.float32)
    x[150:] = (5.0 + rng.standard_normal((50, 8))).astype(np.float32)
    return x[rng.permutation(200)]


def zeros_near_and_far(rs):
    """150 zero rows, 8 rows close to them, 60 rows in three far blobs: lists empty out and are split while centres still move"""
    rng = np.random.default_rng(rs)
    x = np.zeros((218, 8), np.float32)
    x[150:158] = 0.3 * rng.standard_normal((8, 8))
    c = 8.0 * rng.standard_normal((3, 8))
    x[158:] = c[rng.integers(0, 3, 60)] + rng.standard_normal((60, 8))
    return x[rng.permutation(218)]


def nearest_tie(seed):
    """Two of the five seed rows are zero rows, so lists 0 and 2 start as bit-identical centres: every zero row goes to list 0, list 2 stays
    empty and cannot be split apart (it is re-seeded from the zero list, the largest).  The small list 1 next to them has both at exactly
    the same distance: with the tie to the lower id its nearest other centre is list 0, which has rows, so list 1 may be deleted, and it
    moves into the two-part list 3; with the tie to the higher id it would be list 2, which is empty, and list 1 would stay."""
    rng = np.random.default_rng(21)
    near = (np.array([0.6, 0, 0, 0]) + 0.05 * rng.standard_normal((6, 4))).astype(np.float32)
    wide = np.concatenate([np.array([20.0, 0, 0, 0]) + rng.standard_normal((10, 4)), np.array([20.0, 12.0, 0, 0]) + rng.standard_normal((10, 4))])
    far = np.array([-25.0, 5.0, 0, 0]) + rng.standard_normal((12, 4))
    groups = [np.zeros((30, 4)), near, wide, far]
    n = sum(g.shape[0] for g in groups)
    first = [0, 30, 1, 36, 56]  # the rows the seeds must draw, in list order: zero, near, zero, wide (its first part), far
    rest = [i for i in range(n) if i not in first]
    at = bo.seed_rows(n, 5, seed)
    free = [i for i in range(n) if i not in at]
    src = np.concatenate(groups).astype(np.float32)
    x = np.empty_like(src)
    x[at] = src[first]
    x[free] = src[rest]
    return x


# name -> (rows: (factory, args), nlist, niter, seed)
CASES = {
    # several moves per iteration: maxmoves = 60 // 20 = 3 is reached; the same rows at the niter values around the relocation's gate
    "moves_niter8": ((blobs, (60, 16, 2400, 4.0, 11)), 60, 8, 5),
    "moves_niter0": ((blobs, (60, 16, 2400, 4.0, 11)), 60, 0, 5),  # the seeds alone
    "moves_niter1": ((blobs, (60, 16, 2400, 4.0, 11)), 60, 1, 5),
    "moves_niter3": ((blobs, (60, 16, 2400, 4.0, 11)), 60, 3, 5),  # the last value without relocation
    "moves_niter4": ((blobs, (60, 16, 2400, 4.0, 11)), 60, 4, 5),  # the first value with relocation
    # a split and moves in one iteration, a `used` skip; d = 36 leaves k_assigned_dist a 64-lane tail
    # (seeds searched over 1..39: seed 2 splits, moves and skips a `used` centre in iteration 2; seed 35 skips a `moved` one there)
    "split_moves_d36": ((blobs, (80, 36, 3000, 3.0, 12)), 80, 8, 2),
    "split_moved_d36": ((blobs, (80, 36, 3000, 3.0, 12)), 80, 8, 35),
    # d above 256: k_list_mean's strided loop over the dimension
    "d768": ((blobs, (12, 768, 700, 3.0, 13)), 17, 6, 5),
    # more lists than distinct rows: splits every iteration, exact ties, an objective that rises from 0
    "dup_nlist40": ((repeated, (12, 25, 20, 14)), 40, 6, 5),
    "dup_nlist14": ((repeated, (12, 25, 20, 14)), 14, 6, 5),
    # an all-zero centre cannot be split: v * (1 +- 2^-10) is 0
    "zero_rows": ((zeros_and_others, (15,)), 6, 5, 5),
    # splits in the iterations that relocate (seed searched over 1..29: the first for which inputs taken from the nudged centres end elsewhere)
    "zeros_near_far": ((zeros_near_and_far, (2,)), 8, 6, 9),
    # a tie between the two nearest other centres decides a move (rows laid out around the seeds' draw, see nearest_tie)
    "nearest_tie": ((nearest_tie, (5,)), 5, 4, 5),
    # n == nlist: no list has two rows, so nothing can move or split
    "n_eq_nlist": ((blobs, (6, 12, 48, 3.0, 16)), 48, 5, 5),
    "nlist1_d4": ((blobs, (3, 4, 37, 3.0, 17)), 1, 3, 5),
    "d4_nlist5": ((blobs, (5, 4, 203, 4.0, 18)), 5, 6, 5),
    # coarse_assign_exact takes k_coarse_gemm<2, 4> from 512 tiles of 128 lists x 64 rows on: 8 x 64 tiles at n = 4096, and at n = 4095 too
    # (ceil(4095 / 64) = 64; its last tile is one row short); n = 4032 is the largest n that stays on k_coarse_gemm<1, 1> (8 x 63 = 504)
    "grid_n4096": ((blobs, (64, 8, 4096, 3.0, 19)), 1024, 2, 5),
    "grid_n4095": ((blobs, (64, 8, 4095, 3.0, 19)), 1024, 2, 5),
    "grid_n4032": ((blobs, (64, 8, 4032, 3.0, 19)), 1024, 2, 5),
    # coarse_chunk = 512 MiB / (4 * 8192) = 16384 rows < n: the assignment runs in two chunks, the second of 3616 rows
    "two_chunks": ((blobs, (200, 4, 20000, 4.0, 20)), 8192, 1, 5),
}


@lru_cache(maxsize=None)
def rows(name):
    (fn, args), _, _, _ = CASES[name]
    x = fn(*args)
    x.setflags(write=False)
    return x


def params(name):
    _, nlist, niter, seed = CASES[name]
    return dict(nlist=nlist, niter=niter, seed=seed)


@lru_cache(maxsize=None)
def oracle(name, centres_only=False, variant=None):
    """The oracle's build of a case, computed once per process and shared: callers leave it unchanged."""
    return bo.build(rows(name), centres_only=centres_only, variant=variant, **params(name))


# ---- hand-made single updates for the host program (tests/host/ivf_format_main.cpp `steps`): rules of kmeans_relocate that a random
# build reaches rarely or never.  Rows lie along coordinate 0 (the k-th row of a group at pos + step * k (k + 1) / 2: uneven, so that no two
# rows of a list are equally far from its mean), the other three coordinates carry a small jitter.  The assignment is hand-made, not the nearest centre.
def _tight(l):
    """a list nothing wants to move or split: three rows, 100 + 2l apart from the previous one (distinct costs), spread growing with l
    (distinct distortions)"""
    return (l, 3000.0 + 100.0 * l + l * l, 3, 0.1 * (1.0 + l / 40.0))


def _crafted(nlist, groups):
    """groups: (list, pos, rows, step) -> (x [n, 4], assign [n], prev [nlist, 4])"""
    pos, a = [], []
    for l, p, cnt, step in groups:
        pos += [p + step * k * (k + 1) / 2 for k in range(cnt)]
        a += [l] * cnt
    n = len(pos)
    x = np.zeros((n, 4), np.float32)
    x[:, 0] = pos
    for i in range(n):
        for e in range(1, 4):
            x[i, e] = 0.01 * ((i * 7 + e * 3) % 5 - 2)
    prev = np.zeros((nlist, 4), np.float32)
    prev[:, 0] = 9000.0 + 10.0 * np.arange(nlist)  # (only an empty list keeps its previous centre)
    return x, np.array(a, np.int64), prev


def _wide(l, p, gap, extra=0):
    return [(l, p, 4 + extra, 0.1), (l, p + gap, 4, 0.1)]


# name -> (nlist, groups, the facts of the oracle's report the input must show)
CRAFTED = {
    # B, A, C in one blob: A (cheapest) moves into the wide list 5 and takes its receiver B along (`used`); C's nearest centre is A, which
    # is gone (`moved`); then D moves into the wide list 6 and the cap 40 // 20 = 2 ends the loop.  List 39 is empty: the largest list, 5,
    # is split first, so the costs are taken on nudged centres while the distances are those of the means.
    "skips_cap40": (40, [(0, -1.0, 5, 0.1), (1, 0.0, 4, 0.1), (2, 1.5, 4, 0.1), (3, 500.0, 4, 0.1), (4, 503.0, 5, 0.1)]
                    + _wide(5, 1000.0, 40.0, extra=1) + _wide(6, 2000.0, 30.0) + [_tight(l) for l in range(7, 39)],
                    dict(splits=1, moves=[1, 3], skip_used=1, skip_moved=1, brk="cap")),
    # list 1 sits next to the mean of the wide list 0, the list with the largest distortion: that list is its receiver, so the local cursor
    # steps over it (the global one stays) and list 1 moves into the runner-up, list 2; the next candidates no longer pay: `gain <= cost`
    "cursor_gain40": (40, _wide(0, 1000.0, 30.0) + [(1, 1014.0, 2, 0.1)] + _wide(2, 2000.0, 20.0) + [_tight(l) for l in range(3, 40)],
                      dict(splits=0, moves=[1], skip_used=1, cursor_diff=1, brk="gain")),
    # two close pairs of rows, every other list a single row: nothing can be split, the local cursor runs off the end
    "sj_break40": (40, [(0, 0.0, 2, 0.1), (1, 2.0, 2, 0.3)] + [(l, 3000.0 + 100.0 * l + l * l, 1, 0.0) for l in range(2, 40)],
                   dict(splits=0, moves=[], brk="sj")),
    # nlist 19: max(1, 19 // 20) = 1 move, although a second one (list 3 into list 5) would pay
    "cap19": (19, [(0, 0.0, 4, 0.1), (1, 1.5, 5, 0.1)] + _wide(2, 1000.0, 30.0) + [(3, 500.0, 4, 0.1), (4, 503.0, 5, 0.1)] + _wide(5, 2000.0, 20.0)
              + [_tight(l) for l in range(6, 19)], dict(splits=0, moves=[0], brk="cap")),
}


def crafted(name):
    nlist, groups, must = CRAFTED[name]
    return _crafted(nlist, groups) + (nlist, must)


def _both(f):
    """iterations that split an empty list AND moved a centre"""
    return [i for i, (s, m) in enumerate(zip(f["splits"], f["moves"])) if s and m]


def _tiles(name):
    n, nlist = rows(name).shape[0], params(name)["nlist"]
    return ((nlist + 127) // 128) * ((n + 63) // 64)


# name -> what the oracle's report of the case must show: (statement, predicate(facts(name), oracle(name)))
MUST = {
    "moves_niter8": [("the cap of 3 moves is reached", lambda f, o: f["maxmoves"] == 3 and max(f["moves"]) == 3),
                     ("no list empties", lambda f, o: sum(f["splits"]) == 0)],
    "moves_niter0": [("the centroids are the seed rows", lambda f, o: np.array_equal(o["centroids"], rows("moves_niter0")[o["seeds"]])
                      and len(o["objective"]) == 1)],
    "moves_niter1": [("one update, no relocation", lambda f, o: f["brk"] == [None])],
    "moves_niter3": [("three updates, no relocation", lambda f, o: f["brk"] == [None] * 3)],
    "moves_niter4": [("only the first update relocates, and it moves", lambda f, o: f["brk"][1:] == [None] * 3 and f["moves"][0] > 0)],
    "split_moves_d36": [("one iteration splits, moves and skips a used centre",
                         lambda f, o: any(o["report"][i]["skip_used"] for i in _both(f))),
                        ("d is not a multiple of 64", lambda f, o: o["centroids"].shape[1] % 64 == 36)],
    "split_moved_d36": [("one iteration splits, moves and skips a candidate whose nearest centre was moved",
                         lambda f, o: any(o["report"][i]["skip_moved"] for i in _both(f)))],
    "d768": [("d above 256, and a centre moves", lambda f, o: o["centroids"].shape[1] == 768 and sum(f["moves"]) > 0)],
    "dup_nlist40": [("28 splits in every iteration", lambda f, o: f["splits"] == [28] * 6),
                    ("hundreds of exact ties", lambda f, o: sum(f["ties"]) >= 200),
                    ("the objective rises from 0", lambda f, o: o["objective"][0] == 0.0 and o["objective"][1] > 0.0)],
    "dup_nlist14": [("splits in every iteration", lambda f, o: all(f["splits"])),
                    ("hundreds of exact ties", lambda f, o: sum(f["ties"]) >= 200)],
    "zero_rows": [("splits in every iteration, none of which can part the zero centre", lambda f, o: all(f["splits"])),
                  ("duplicate final centroids", lambda f, o: len(np.unique(o["centroids"], axis=0)) < 6),
                  ("empty final lists", lambda f, o: int((np.diff(o["list_offsets"]) == 0).sum()) > 0)],
    "zeros_near_far": [("an iteration splits and moves", lambda f, o: len(_both(f)) > 0)],
    "nearest_tie": [("the first update re-seeds the empty twin of the zero list and moves list 1",
                     lambda f, o: f["splits"][0] == 1 and [j for j, _ in o["report"][0]["moves"]] == [1] and f["ties"][0] >= 30)],
    "n_eq_nlist": [("n == nlist: nothing splits, nothing moves, no list can be split (the `sj` break)",
                    lambda f, o: rows("n_eq_nlist").shape[0] == 48 and not sum(f["splits"]) and not sum(f["moves"]) and f["brk"][:2] == ["sj", "sj"])],
    "nlist1_d4": [("one list, the smallest dimension", lambda f, o: o["centroids"].shape == (1, 4))],
    "d4_nlist5": [("the smallest dimension, and a centre moves", lambda f, o: o["centroids"].shape[1] == 4 and sum(f["moves"]) > 0)],
    "grid_n4096": [("512 tiles: the first grid on k_coarse_gemm<2, 4>", lambda f, o: _tiles("grid_n4096") == 512)],
    "grid_n4095": [("512 tiles, the last row tile one row short", lambda f, o: _tiles("grid_n4095") == 512 and 4095 % 64 == 63)],
    "grid_n4032": [("504 tiles: the last grid on k_coarse_gemm<1, 1>", lambda f, o: _tiles("grid_n4032") == 504 and _tiles("grid_n4032") + 8 == 512)],
    "two_chunks": [("the assignment needs two chunks", lambda f, o: (512 << 20) // (4 * 8192) == 16384 < rows("two_chunks").shape[0] <= 2 * 16384)],
}


def facts(name):
    """the report of a case in one dict: per-iteration lists and the totals the tests and the summary quote"""
    rep = oracle(name)["report"]
    its = [r for r in rep if not r["final"]]
    return dict(
        splits=[r["splits"] for r in its],
        moves=[len(r["moves"]) for r in its],
        skip_used=sum(r["skip_used"] for r in its),
        skip_moved=sum(r["skip_moved"] for r in its),
        cursor_diff=sum(r["cursor_diff"] for r in its),
        brk=[r["brk"] for r in its],
        ties=[r["ties"] for r in rep],
        margin=bo.smallest_margin(rep),
        maxmoves=max(1, params(name)["nlist"] // 20),
    )
