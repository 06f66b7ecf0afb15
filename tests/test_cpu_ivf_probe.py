"""The cases of tests/ivf_probe_cases.py on the oracle alone: the conditions under which tests/test_gpu_ivf_probe.py may ask the
device for the oracle's bits (ids AND fp32 distances) without hiding or inventing a failure.

The device adds the d squared differences of a row in another order than either restatement (lane partials, fma).  Two fp64 sums of
the same d terms differ by at most ~(d + 2) 2^-53 relative; ``margin(d)`` is four times that.  So the answer is order-independent when
neighbouring candidates, the centroid distances at the nprobe cut and every returned distance keep further than ``margin(d)`` from,
respectively, each other and the nearest fp32 rounding boundary -- or are EXACTLY equal, as the planted bit-identical rows and
centroids are (the same bits give the same sum in any fixed order; the tie then goes to the lowest id)."""
import numpy as np
import pytest

import ivf_probe_cases as cases
from oracle import ivf_oracle

CASES = [(d, np_) for d in cases.DIMS for np_ in cases.nprobes(20)]


def _check_report(rep, d, what, cut_ties_allowed=0):
    m = cases.margin(d)
    print("%s: neighbour gap %.3g, midpoint margin %.3g, cut gap %.3g (margin %.3g); %d exact neighbour ties, %d exact cut ties"
          % (what, rep["gap"], rep["mid"], rep["cut"], m, rep["ties"], rep["cut_ties"]))
    assert rep["gap"] > m, "%s: two unequal neighbouring distances within the summation-order margin" % what
    assert rep["mid"] > m, "%s: a returned distance within the margin of an fp32 rounding midpoint" % what
    assert rep["cut"] > m, "%s: unequal centroid distances at the nprobe cut within the margin" % what
    assert rep["cut_ties"] <= cut_ties_allowed, "%s: an exact centroid tie at the cut that no case planted" % what


def test_layout_is_the_one_the_kernels_need():
    for d in cases.DIMS:
        idx, q, planted = cases.probe_case(d)
        s = cases.STEP[d]
        sizes = np.diff(idx["list_offsets"])
        assert idx["nlist"] == 20 and q.shape == (cases.NQ, d) and q.dtype == np.float32
        for want in (1, s - 1, s, s + 1, 2 * s - 1, 2 * s, 2 * s + 1, 3 * s + 1, 4 * s, 4 * s + 1):
            assert want in sizes, (d, want)
        assert int((sizes == 0).sum()) == 2 and int(np.sort(sizes)[:9].sum()) >= 8
        assert sorted(idx["ids"].tolist()) == list(range(idx["ntotal"]))
        # the planted row: three positions, the same bits, two lists, ids against the scan order, query 0 equal to it
        pa, pb, pc = planted["pos"]
        off = idx["list_offsets"]
        a, b = planted["list_a"], planted["list_b"]
        assert a != b and off[a] <= pc < pa == off[a + 1] - 1 and pb == off[b + 1] - 1 and off[b] <= pb
        assert pa - off[a] == 4 * s and pc - off[a] < s  # alone in the fifth pipeline step / in the first
        for p in (pb, pc):
            assert idx["vecs"][p].tobytes() == idx["vecs"][pa].tobytes()
        assert q[0].tobytes() == idx["vecs"][pa].tobytes()
        assert (int(idx["ids"][pb]), int(idx["ids"][pa]), int(idx["ids"][pc])) == planted["ids"] and planted["ids"][0] < planted["ids"][1] < planted["ids"][2]
        # both lists are the two nearest of query 0: nprobe 1 sees the two copies of list a, nprobe >= 2 all three
        assert list(ivf_oracle.coarse_assign(idx, q[:1], 2)[0]) == [a, b]
        D1, I1 = cases.expected(d, 1)
        D2, I2 = cases.expected(d, 2)
        assert list(I1[0, :2]) == [planted["ids"][1], planted["ids"][2]] and D1[0, 0] == 0 and D1[0, 1] == 0 and D1[0, 2] > 0
        assert list(I2[0, :3]) == list(planted["ids"]) and np.all(D2[0, :3] == 0) and D2[0, 3] > 0


@pytest.mark.parametrize("d,nprobe", CASES)
def test_both_restatements_agree_bit_for_bit(d, nprobe):
    """einsum order (``search``) against element order (``search_c``): every I and every D, every k."""
    idx, q, _ = cases.probe_case(d)
    D, I = cases.expected(d, nprobe)
    for k in cases.KS:
        Dc, Ic, _ = ivf_oracle.search_c(idx, q, k, nprobe=nprobe)
        assert np.array_equal(Ic, I[:, :k]) and np.array_equal(Dc, D[:, :k]), (d, nprobe, k)
    assert np.all(np.diff(D.astype(np.float64), axis=1) >= 0)


@pytest.mark.parametrize("d,nprobe", CASES)
def test_no_near_tie_no_rounding_boundary_no_near_cut(d, nprobe):
    idx, q, _ = cases.probe_case(d)
    rep = cases.exactness_report(idx, q, nprobe)
    _check_report(rep, d, "d %d nprobe %d" % (d, nprobe))
    assert rep["ties"] >= 1  # the planted copies: an exact tie is there to be ordered by id


@pytest.mark.parametrize("d", cases.DIMS)
def test_padding_is_what_the_cases_intend(d):
    """nprobe 1 and 2 leave padded results (so the realtime guard has something to see), nprobe 9 and beyond leave none."""
    padded = {np_: int((cases.expected(d, np_)[1] < 0).any(axis=1).sum()) for np_ in cases.nprobes(20)}
    print("d %d: padded queries per nprobe %s" % (d, padded))
    assert padded[1] >= 1 and padded[2] >= 1, padded
    assert padded[9] == 0 and padded[20] == 0 and padded[23] == 0, padded
    for np_ in cases.nprobes(20):
        D, I = cases.expected(d, np_)
        assert np.all(D[I < 0] == ivf_oracle.FLT_MAX) and np.all(D[I >= 0] < ivf_oracle.FLT_MAX)
    # results really come from several lists: some query's top-8 at nprobe 9 is not its top-8 at nprobe 1 plus padding
    I1, I9 = cases.expected(d, 1)[1], cases.expected(d, 9)[1]
    full = (I1 >= 0).all(axis=1)
    assert (I1[full] != I9[full]).any(), "no query with a full first list takes a result from a later list"


@pytest.mark.parametrize("d", cases.DIMS)
def test_coarse_cut_case(d):
    """Two bit-identical centroids at ranks 3 and 4 of query 0: the lower list id is probed at nprobe 3, the higher is not -- and the
    higher one holds the nearest row of the whole index, so the difference shows in the result."""
    idx, q, info = cases.cut_case(d)
    a, b = info["a"], info["b"]
    assert a < b and idx["centroids"][a].tobytes() == idx["centroids"][b].tobytes()
    order = ivf_oracle.coarse_assign(idx, q[:1], idx["nlist"])[0]
    assert (int(order[2]), int(order[3])) == (a, b)
    cd = cases.centroid_distances(idx, q[0])
    assert cd[1] < cd[2] == cd[3] < cd[4]
    # the nearest row of all (fp64 brute force) lies in list b
    diff = idx["vecs"].astype(np.float64) - q[0].astype(np.float64)[None, :]
    near = int(np.argmin(np.einsum("ij,ij->i", diff, diff)))
    assert near == info["near_pos"] and idx["list_offsets"][b] <= near < idx["list_offsets"][b + 1]
    assert int((np.diff(idx["list_offsets"]) < 8).sum()) == 0  # no padding in this case
    for nprobe, inside in ((cases.CUT_STRADDLE, False), (cases.CUT_INSIDE, True)):
        D, I = ivf_oracle.search(idx, q, 8, nprobe=nprobe)
        Dc, Ic, _ = ivf_oracle.search_c(idx, q, 8, nprobe=nprobe)
        assert np.array_equal(I, Ic) and np.array_equal(D, Dc)
        assert (I[0, 0] == info["near_id"]) == inside and (info["near_id"] in I[0]) == inside
        # every cut of the case is clear of the margin or is the planted pair (query 0 meets it at nprobe 3; another query may, at either)
        rep = cases.exactness_report(idx, q, nprobe)
        _check_report(rep, d, "cut case d %d nprobe %d" % (d, nprobe), cut_ties_allowed=q.shape[0])
        if not inside:
            assert rep["cut_ties"] >= 1


@pytest.mark.parametrize("d", cases.DIMS)
def test_wrong_scans_would_show(d):
    """The cases can tell a wrong scan from a right one.  Restated on the oracle: (a) a row loop without its ``rr < end`` guard inserts
    the clamped last row of a list once per idle row slot of the last pipeline step; (b) a probe loop that stops one list early;
    (c) ties resolved to the HIGHEST id.  Each changes the expected result at every nprobe it applies to."""
    idx, q, planted = cases.probe_case(d)
    s = cases.STEP[d]
    off = idx["list_offsets"]
    sizes = np.diff(off)
    padded_sizes = np.where(sizes > 0, -(-sizes // s) * s, 0)
    pos = np.concatenate([np.minimum(np.arange(off[l], off[l] + padded_sizes[l]), off[l + 1] - 1) for l in range(idx["nlist"])]).astype(np.int64)
    off2 = np.zeros_like(off)
    np.cumsum(padded_sizes, out=off2[1:])
    unguarded = dict(idx, list_offsets=off2, ids=idx["ids"][pos], vecs=idx["vecs"][pos], ntotal=len(pos))
    for nprobe in cases.nprobes(20):
        D, I = cases.expected(d, nprobe)
        assert not np.array_equal(ivf_oracle.search(unguarded, q, 8, nprobe=nprobe)[1], I), (d, nprobe, "unguarded tail rows")
        if nprobe in (2, 9):  # (the farthest of all 20 lists supplies no result: nothing to see at nprobe = nlist)
            assert not np.array_equal(ivf_oracle.search(idx, q, 8, nprobe=nprobe - 1)[1], I), (d, nprobe, "one list short")
    flipped = dict(idx, ids=(idx["ntotal"] - 1 - idx["ids"]))  # the same search with the id order reversed = ties to the highest id
    for nprobe in (1, 2, 9):
        I = cases.expected(d, nprobe)[1]
        If = ivf_oracle.search(flipped, q, 8, nprobe=nprobe)[1]
        assert not np.array_equal(np.where(If >= 0, idx["ntotal"] - 1 - If, -1), I), (d, nprobe, "ties to the highest id")


def test_transition_queries_meet_the_same_conditions():
    """The 600 queries of the nprobe-transition script, at every nprobe the script sets."""
    idx, _, _ = cases.probe_case(256)
    q = cases.transition_queries()
    steps = [s for s in cases.TRANSITIONS if s != "reserve"]
    assert steps == [(1, 128), (9, 20), (1, 128), (3, 300), (9, 300), (1, 10), (2, 600), (1, 600)]
    assert cases.TRANSITIONS.index("reserve") == 6 and cases.RESERVE_NQ == 1000
    for nprobe in sorted({s[0] for s in steps}):
        nq = max(s[1] for s in steps if s[0] == nprobe)
        _check_report(cases.exactness_report(idx, q[:nq], nprobe), 256, "transition nprobe %d, %d queries" % (nprobe, nq))
        D, I = ivf_oracle.search(idx, q[:nq], 8, nprobe=nprobe)
        Dc, Ic = cases.transition_expected(nprobe)
        assert np.array_equal(I, Ic[:nq]) and np.array_equal(D, Dc[:nq])


def test_search_c_refuses_more_probes_than_the_c_loop_holds():
    """oracle/ivf_scan.c keeps ``lists[64]`` per query and would silently probe 64 lists: above that the wrapper raises."""
    from ivf_cases import make_index

    idx = make_index(200, 8, 70, seed=1)
    q = np.random.default_rng(0).standard_normal((3, 8), dtype=np.float32)
    D, I, _ = ivf_oracle.search_c(idx, q, 8, nprobe=64)
    Dn, In = ivf_oracle.search(idx, q, 8, nprobe=64)
    assert np.array_equal(I, In) and np.allclose(D, Dn, rtol=1e-6, atol=0)
    for nprobe in (65, 70, 1000):
        with pytest.raises(ValueError, match="at most 64"):
            ivf_oracle.search_c(idx, q, 8, nprobe=nprobe)
    small = make_index(100, 8, 20, seed=2)
    ivf_oracle.search_c(small, q, 8, nprobe=1000)  # min(nprobe, nlist) = 20: fine
    assert max(min(np_, 20) for np_ in cases.nprobes(20)) <= ivf_oracle.C_MAX_PROBES
