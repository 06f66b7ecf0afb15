"""GPU parity of the HIP IVF-Flat retrieval (C ABI via the faiss-like Python object) against the CPU oracle:
bit-exact ids, distances to fp32 rounding, the blend to 1e-5 RMS; the reference's edge semantics; file and blob
round trips; and ranking properties at BASELINE's stress size."""
import numpy as np
import pytest
import torch

from oracle import ivf_oracle, synth

pytestmark = pytest.mark.gpu


def make(idx, gpu, nprobe=1):
    import rvc_amd

    return rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], nprobe=nprobe, device=gpu)


@pytest.mark.parametrize("n,d,nq", [(10000, 768, 599), (5000, 256, 301), (2000, 64, 33)])
def test_search_ids_bit_exact_and_distances(n, d, nq, gpu):
    idx = synth.make_ivf(n, d, seed=n, dup=9)
    q = synth.make_phone(1, nq, d, seed=n)[0].numpy()
    q[:5] = idx["xb"][:5]  # exact hits
    h = make(idx, gpu)
    assert (h.ntotal, h.d, h.nlist, h.nprobe) == (n, d, idx["nlist"], 1)
    D, I = h.search(q, 8)
    Dr, Ir = ivf_oracle.search(idx, q, 8)
    assert I.dtype == np.int64 and D.dtype == np.float32
    assert np.array_equal(I, Ir), "%d id mismatches" % int((I != Ir).sum())
    assert np.array_equal(D, Dr)
    for k in (1, 3):  # top-1 (legacy tools/cmd/infer-pm-index256.py:161) = column 0 of top-8
        Dk, Ik = h.search(q, k)
        assert np.array_equal(Ik, Ir[:, :k]) and np.array_equal(Dk, Dr[:, :k])
    # torch in -> torch out, device resident
    Dt, It = h.search(torch.from_numpy(q).to(gpu), 8)
    assert Dt.is_cuda and np.array_equal(It.cpu().numpy(), Ir)
    # queries scanned in the list-sorted, XCD-contiguous order (k_qsort_*, opt-in) instead of arrival order: identical results
    h.set_option("IVF_LM", 0)  # (the list-sorted order is an option of the query-major kernel)
    h.set_option("IVF_SORT", 1)
    D0, I0 = h.search(q, 8)
    h.set_option("IVF_SORT", None)
    assert np.array_equal(I0, Ir) and np.array_equal(D0, Dr)
    # query-major kernel (round 3, IVF_LM=0) and list-major path (default from 16 queries on): the same bits, and the profiler
    # names say which one ran
    for lm in (0, None):
        h.set_option("IVF_LM", lm)
        h.profile(True)
        D1, I1 = h.search(q, 8)
        names = {st["name"] for st in h.profile_read()}
        h.profile(False)
        assert np.array_equal(I1, Ir) and np.array_equal(D1, Dr)
        assert ("ivf_select" in names) == (lm is None and nq >= 16 and d % 32 == 0), names


@pytest.mark.parametrize("nprobe", [2, 9])
def test_nprobe_greater_than_one(nprobe, gpu):
    """Legacy indices carry nprobe=9 (tools/cmd/train-index.py:26-29)."""
    idx = synth.make_ivf(4000, 64, nlist=50, seed=5)
    q = np.random.default_rng(3).standard_normal((77, 64), dtype=np.float32)
    h = make(idx, gpu, nprobe=nprobe)
    D, I = h.search(q, 8)
    Dr, Ir = ivf_oracle.search(idx, q, 8, nprobe=nprobe)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    h.nprobe = 1  # web.py:551-552
    D1, I1 = h.search(q, 8)
    Dr1, Ir1 = ivf_oracle.search(idx, q, 8, nprobe=1)
    assert h.nprobe == 1 and np.array_equal(I1, Ir1)


def test_short_lists_empty_lists_empty_queries_and_ties(gpu):
    idx = synth.make_ivf(60, 16, nlist=20, seed=8)  # ~3 rows per list: shorter than k
    # plus one EMPTY list whose centroid sits far away: a query next to it gets nothing but -1 / FLT_MAX padding
    far = np.full((1, 16), 50.0, np.float32)
    idx["centroids"] = np.concatenate([idx["centroids"][:5], far, idx["centroids"][5:]])
    idx["list_offsets"] = np.concatenate([idx["list_offsets"][:6], idx["list_offsets"][5:]])
    idx["nlist"] = 21
    assert (np.diff(idx["list_offsets"]) == 0).sum() == 1
    q = np.random.default_rng(2).standard_normal((40, 16), dtype=np.float32)
    q[7] = far[0] + 0.01
    h = make(idx, gpu)
    D, I = h.search(q, 8)
    Dr, Ir = ivf_oracle.search(idx, q, 8)
    assert np.array_equal(I, Ir) and (I == -1).any() and (I[7] == -1).all()
    assert np.all(D[I == -1] == np.float32(3.4028234663852886e38)) and np.array_equal(D, Dr)
    D0, I0 = h.search(q[:0], 8)
    assert D0.shape == (0, 8) and I0.shape == (0, 8)
    # duplicates: ties resolve to the lowest id
    idx2 = synth.make_ivf(300, 16, nlist=4, seed=9)
    idx2["vecs"][1] = idx2["vecs"][0]
    h2 = make(idx2, gpu, nprobe=4)
    D2, I2 = h2.search(idx2["vecs"][:1].copy(), 2)
    assert D2[0, 0] == 0 and D2[0, 1] == 0 and list(I2[0]) == sorted([int(idx2["ids"][0]), int(idx2["ids"][1])])
    with pytest.raises(ValueError):
        h.search(np.zeros((3, 17), np.float32), 8)  # dimension mismatch (the reference raises "index mistatch")
    with pytest.raises(TypeError):
        h.search(np.zeros((3, 16), np.float64), 8)
    import rvc_amd

    with pytest.raises(rvc_amd.RvcmiError):
        h.search(q, 9)  # k > 8


def test_list_major_scan_edge_cases(gpu):
    """The list-major path (ivf_lm_kernels.hpp: plan -> fp32 MFMA score tiles -> fp64 verification of everything inside the
    rigorous margin) on the cases the tile logic can get wrong: lists shorter than k (padding -1 / FLT_MAX), an EMPTY probed list,
    lists of exactly 32 / 33 / 65 rows (tile edges), more than 32 queries on one list (several query tiles), exact duplicate rows
    (distance ties -> lowest id) and an exact hit; against the oracle and against the query-major kernel, fused blend included."""
    rng = np.random.default_rng(31)
    d = 32
    sizes = np.array([3, 0, 32, 33, 65, 1, 8, 9, 200, 7], dtype=np.int64)
    nlist, n = len(sizes), int(sizes.sum())
    cent = (rng.standard_normal((nlist, d)) * 6).astype(np.float32)
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    vecs = np.concatenate([cent[l] + rng.standard_normal((int(sizes[l]), d)).astype(np.float32) for l in range(nlist)]).astype(np.float32)
    vecs[off[8] + 5] = vecs[off[8] + 4]        # duplicate rows inside the 200-row list
    vecs[off[8] + 150] = vecs[off[8] + 4]
    ids = rng.permutation(n).astype(np.int64)
    idx = dict(d=d, ntotal=n, nlist=nlist, nprobe=1, centroids=cent, list_offsets=off, ids=ids, vecs=vecs)
    pos = np.empty(n, np.int64)
    pos[ids] = np.arange(n)
    idx["xb"] = vecs[pos]
    per = [5, 4, 10, 40, 70, 3, 9, 33, 90, 6]  # queries aimed at every list (the empty one included), two lists get > 32
    q = np.concatenate([cent[l] + 0.7 * rng.standard_normal((per[l], d)).astype(np.float32) for l in range(nlist)]).astype(np.float32)
    q[-1] = vecs[off[8] + 4]                   # an exact hit on the triplicated row
    q = q[rng.permutation(len(q))]
    assert len(q) >= 64
    h = make(idx, gpu)
    Dr, Ir = ivf_oracle.search(idx, q, 8)
    assert (Ir == -1).any() and (Ir[:, 0] == -1).any()
    for lm in (None, 0):
        h.set_option("IVF_LM", lm)
        h.profile(True)
        D, I = h.search(q, 8)
        names = {st["name"] for st in h.profile_read()}
        h.profile(False)
        assert ("ivf_select" in names) == (lm is None)
        assert np.array_equal(I, Ir), "IVF_LM=%s: %d id mismatches" % (lm, int((I != Ir).sum()))
        assert np.array_equal(D, Dr)
        for k in (1, 5):
            Dk, Ik = h.search(q, k)
            assert np.array_equal(Ik, Ir[:, :k]) and np.array_equal(Dk, Dr[:, :k])
        got = h.search_blend(torch.from_numpy(q).to(gpu), 0.75).cpu().numpy()
        exp = ivf_oracle.search_blend(idx, q, 0.75)
        ok = ~np.isnan(exp).any(1)
        assert np.array_equal(np.isnan(got).any(1), ~ok) and np.abs(got[ok] - exp[ok]).max() <= 1e-5
        kept = h.search_blend(torch.from_numpy(q).to(gpu), 0.75, skip_if_short=True).cpu().numpy()
        assert np.array_equal(kept, q)  # some list is shorter than k: the realtime guard skips the whole call
    h.set_option("IVF_LM", None)


def test_search_blend_matches_pipeline_arithmetic(gpu):
    """pipeline.py:129-138 fused on the device, incl. its edge cases: id -1 -> big_npy[-1] with zero weight,
    exact hit -> NaN row, and the realtime guard of rtrvc.py:173."""
    idx = synth.make_ivf(10000, 768, seed=4321)
    h = make(idx, gpu)
    q = synth.make_phone(1, 599, 768)[0].numpy()
    exp = ivf_oracle.search_blend(idx, q, 0.75)
    got = h.search_blend(torch.from_numpy(q).to(gpu), 0.75).cpu().numpy()
    assert np.sqrt(np.mean((got - exp) ** 2)) <= 1e-5 and np.abs(got - exp).max() <= 1e-5
    big = h.reconstruct_n(0, h.ntotal)
    assert np.array_equal(big, idx["xb"])
    assert np.array_equal(h.reconstruct_n(17, 5), idx["xb"][17:22])
    # exact hit -> inf/inf = NaN for that row, exactly as numpy gives the reference
    q2 = q[:8].copy()
    q2[3] = idx["xb"][123]
    got2 = h.search_blend(torch.from_numpy(q2).to(gpu), 0.5).cpu().numpy()
    exp2 = ivf_oracle.search_blend(idx, q2, 0.5)
    assert np.isnan(got2[3]).all() and np.isnan(exp2[3]).all()
    assert np.abs(np.delete(got2, 3, 0) - np.delete(exp2, 3, 0)).max() <= 1e-5
    # short lists: offline path blends with big_npy[-1]*0, realtime path skips the whole call
    idx3 = synth.make_ivf(60, 16, nlist=20, seed=8)
    h3 = make(idx3, gpu)
    q3 = np.random.default_rng(2).standard_normal((40, 16), dtype=np.float32)
    exp3 = ivf_oracle.search_blend(idx3, q3, 0.75)
    got3 = h3.search_blend(torch.from_numpy(q3).to(gpu), 0.75).cpu().numpy()
    assert np.abs(got3 - exp3).max() <= 1e-5
    kept = h3.search_blend(torch.from_numpy(q3).to(gpu), 0.75, skip_if_short=True).cpu().numpy()
    assert np.array_equal(kept, q3)
    # retrieve_blend: the Pipeline.vc glue (keeps dtype/shape, index_rate 0 or index None = untouched)
    import rvc_amd

    f = torch.from_numpy(q).to(gpu).half().unsqueeze(0)
    out = rvc_amd.retrieve_blend(f, h, 0.75)
    assert out.shape == f.shape and out.dtype == torch.float16
    assert rvc_amd.retrieve_blend(f, None, 0.75) is f and rvc_amd.retrieve_blend(f, h, 0) is f


def test_faiss_file_and_blob_roundtrips(tmp_path, gpu):
    import rvc_amd

    idx = synth.make_ivf(3000, 256, seed=77)
    q = np.random.default_rng(1).standard_normal((50, 256), dtype=np.float32)
    h = make(idx, gpu)
    _, I = h.search(q, 8)
    p = str(tmp_path / "added_IVF76_Flat_nprobe_1.index")
    rvc_amd.write_index(h, p)  # C++ writer -> independent python reader
    r = ivf_oracle.read_index(p)
    for k in ("centroids", "list_offsets", "ids", "vecs"):
        assert np.array_equal(r[k], idx[k]), k
    for sparse in (False, True):  # python writer -> C++ reader
        p2 = str(tmp_path / ("py%d.index" % sparse))
        ivf_oracle.write_index(idx, p2, sparse=sparse)
        h2 = rvc_amd.read_index(p2, gpu)
        assert np.array_equal(h2.search(q, 8)[1], I)
    blob = h.blob()  # what one RCCL broadcast ships
    h3 = rvc_amd.IVFFlatHIP.from_blob(blob.clone())
    assert np.array_equal(h3.search(q, 8)[1], I) and h3.ntotal == h.ntotal
    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.IVFFlatHIP.from_blob(torch.zeros(4096, dtype=torch.uint8, device=gpu))
    trunc = tmp_path / "trunc.index"
    trunc.write_bytes(open(p, "rb").read()[:5000])
    with pytest.raises(rvc_amd.RvcmiError, match="truncated"):
        rvc_amd.read_index(str(trunc), gpu)


def test_coarse_prefilter_is_exact_on_adversarial_near_ties(gpu):
    """The nprobe=1 coarse pass scores centroids in fp32 (MFMA) and re-checks every centroid inside a rigorous error
    margin in fp64.  Centroids that differ by ~1e-6 relative (far below fp32 dot-product resolution at d=768) make
    nearly ALL of them candidates; the chosen list must still be the exact fp64 argmin with ties to the lowest id."""
    rng = np.random.default_rng(77)
    d, nlist, per = 768, 300, 4
    base = rng.standard_normal(d).astype(np.float32) * 3
    cent = (base[None, :] + 1e-5 * rng.standard_normal((nlist, d))).astype(np.float32)
    cent[17] = cent[5]  # an exact duplicate centroid: the lower id must win
    n = nlist * per
    vecs = rng.standard_normal((n, d), dtype=np.float32)
    off = np.arange(0, n + 1, per, dtype=np.int64)
    ids = rng.permutation(n).astype(np.int64)
    idx = dict(d=d, ntotal=n, nlist=nlist, nprobe=1, centroids=cent, list_offsets=off, ids=ids, vecs=vecs)
    q = (base[None, :] + 1e-5 * rng.standard_normal((200, d))).astype(np.float32)
    q[:3] = cent[[5, 100, 299]]
    import rvc_amd

    h = rvc_amd.IVFFlatHIP.from_arrays(cent, off, ids, vecs, device=gpu)
    D, I = h.search(q, 4)
    Dr, Ir = ivf_oracle.search(idx, q, 4)
    assert np.array_equal(I, Ir), "%d mismatches" % int((I != Ir).sum())
    assert np.array_equal(D, Dr)
    lists = ivf_oracle.coarse_assign(idx, q, 1)[:, 0]
    assert lists[0] == 5 and 17 not in lists  # duplicate centroid: lowest id


def test_stress_size_ranking_properties(gpu):
    """BASELINE's stress shape (1M x 256, nlist 16000, nprobe 1) through size-independent properties:
    results ascending, every hit comes from the probed list, top-1 == brute force over that list in fp64, and a
    query equal to a stored row finds it at distance 0 when its list is probed."""
    n, d, nlist = 1_000_000, 256, 16000
    rng = np.random.default_rng(4321)
    vecs = rng.standard_normal((n, d), dtype=np.float32)
    cent = vecs[rng.choice(n, nlist, replace=False)].copy()
    sizes = np.full(nlist, n // nlist, dtype=np.int64)
    sizes[: n - sizes.sum()] += 1
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    ids = rng.permutation(n).astype(np.int64)
    import rvc_amd

    h = rvc_amd.IVFFlatHIP.from_arrays(cent, off, ids, vecs, device=gpu)
    q = rng.standard_normal((599, d), dtype=np.float32)
    D, I = h.search(q, 8)
    assert np.all(np.diff(D.astype(np.float64), axis=1) >= 0) and (I >= 0).all()
    pos_of_id = np.empty(n, np.int64)
    pos_of_id[ids] = np.arange(n)
    lists = np.searchsorted(off, pos_of_id[I], side="right") - 1
    assert np.all(lists == lists[:, :1])  # one probed list per query
    c64 = cent.astype(np.float64)
    for i in range(0, 599, 37):  # brute force on a sample of queries
        dist = ((c64 - q[i].astype(np.float64)) ** 2).sum(1)
        l = int(np.argmin(dist))
        assert lists[i, 0] == l
        rows = vecs[off[l]:off[l + 1]].astype(np.float64)
        dd = ((rows - q[i].astype(np.float64)) ** 2).sum(1)
        order = np.lexsort((ids[off[l]:off[l + 1]], dd))[:8]
        assert np.array_equal(I[i], ids[off[l]:off[l + 1]][order])
        assert np.array_equal(D[i], dd[order].astype(np.float32))


def _path_names(h, fn):
    """Runs fn() with the handle's profiler on -> (result, set of launch names): 'ivf_plan' / 'ivf_select' = the list-major kernels."""
    h.profile(True)
    r = fn()
    names = {st["name"] for st in h.profile_read()}
    h.profile(False)
    return r, names


def _assert_equal_to_c_oracle(idx, h, q, gpu, what, blend_rate=0.75):
    """ids bit-equal on every query; distances bit-equal after the fp64 -> fp32 rounding except where the two fp64 summation orders
    (the C loop adds in element order, the wave adds 64 lane partials) straddle an fp32 rounding boundary: at most a handful of
    1-ulp cases in 300 000 distances; fused search + blend <= 1e-5 RMS against the C blend of the oracle's own (D, P)."""
    Dr, Ir, Pr = ivf_oracle.search_c(idx, q, 8)
    (D, I), names = _path_names(h, lambda: h.search(q, 8))
    assert {"ivf_plan", "ivf_select"} <= names, "%s: the list-major kernels did not run (%s)" % (what, names)
    bad = int((I != Ir).sum())
    assert bad == 0, "%s: %d of %d ids differ from the fp64 oracle (first query %d)" % (what, bad, I.size, int(np.argwhere(I != Ir)[0][0]))
    neq = D != Dr
    if neq.any():
        ulp = np.abs(D.view(np.int32).astype(np.int64) - Dr.view(np.int32).astype(np.int64))
        assert int(neq.sum()) <= 8 and int(ulp.max()) <= 1, "%s: %d distances differ, up to %d ulp" % (what, int(neq.sum()), int(ulp.max()))
    feats = torch.from_numpy(q).to(gpu).contiguous()
    _, names = _path_names(h, lambda: h.search_blend(feats, blend_rate, 8))
    assert {"ivf_plan", "ivf_select"} <= names, names
    exp = ivf_oracle.blend_c(idx, q, Dr, Pr, blend_rate)
    got = feats.cpu().numpy()
    fin = np.isfinite(exp).all(1)  # (an exact hit -> distance 0 -> weight inf -> NaN row, in numpy as on the device)
    assert np.array_equal(np.isfinite(got).all(1), fin)
    e = float(np.sqrt(np.mean((got[fin].astype(np.float64) - exp[fin]) ** 2)))
    assert e <= 1e-5, "%s: blend RMS %.2e" % (what, e)
    return int(neq.sum())


def test_batch_scale_on_the_bench_index_equals_the_oracle(gpu):
    """BASELINE configs[2]: 64 clips x 599 queries = 38 336 queries in ONE call against the 10000 x 768 index of bench.py -- the
    list-major path with many 32-query tiles per list (fp32 near-ties become expected at this scale; the fp64
    verification margin of k_lm_select is what keeps the answer exact).  Checked on EVERY query against the OpenMP C oracle."""
    idx = synth.make_ivf(10000, 768, seed=4321, kmeans_iters=1)  # bench.py's index
    q = synth.make_phone(64, 599, 768, seed=1234).reshape(-1, 768).numpy()  # bench.py's queries (rank 0)
    q[7] = idx["xb"][123]  # one exact hit
    h = make(idx, gpu)
    _assert_equal_to_c_oracle(idx, h, q, gpu, "10000 x 768, 38336 queries")
    # the same queries in the query-major kernel (IVF_LM=0): the same bits
    D1, I1 = h.search(q[:4096], 8)
    h.set_option("IVF_LM", 0)
    (D0, I0), names = _path_names(h, lambda: h.search(q[:4096], 8))
    assert "ivf_plan" not in names and np.array_equal(I0, I1) and np.array_equal(D0, D1)


def test_batch_scale_on_the_config3_index_equals_the_oracle(gpu, tmp_path):
    """BASELINE configs[3] exactly as ``bench.py --config 3`` builds it: 1 000 000 x 256 clustered rows, nlist 16000 (of the
    planner's 16 384), trained on the GPU (``rvcmi_ivf_build``, 2 iterations, seed 4321), one rank's 64 x 599 = 38 336 queries."""
    import rvc_amd

    n, d = 1_000_000, 256
    nlist = synth.ivf_nlist(n)
    assert nlist == 16000
    rows = synth.make_clustered_rows(n, d, nlist, seed=4321)
    h = rvc_amd.IVFFlatHIP.train(rows, nlist=nlist, niter=2, seed=4321, device=gpu)
    del rows
    path = str(tmp_path / "config3.index")
    rvc_amd.write_index(h, path)
    idx = ivf_oracle.read_index(path)  # the host copy of what the GPU built: the oracle searches THAT index
    assert idx["ntotal"] == n and idx["nlist"] == nlist and int(np.diff(idx["list_offsets"]).max()) <= 2048
    q = synth.make_phone(64, 599, d, seed=1234).reshape(-1, d).numpy()
    _assert_equal_to_c_oracle(idx, h, q, gpu, "1M x 256 (GPU-trained), 38336 queries")


def _tiny_index(sizes, d, seed=0, spread=0.05):
    """An IVF layout with GIVEN list sizes: centroid c far from the others, its rows a tight cloud around it."""
    rng = np.random.default_rng(seed)
    nlist = len(sizes)
    cent = (rng.standard_normal((nlist, d)) * 4.0).astype(np.float32)
    off = np.zeros(nlist + 1, np.int64)
    np.cumsum(np.asarray(sizes, np.int64), out=off[1:])
    n = int(off[-1])
    lab = np.repeat(np.arange(nlist), sizes)
    vecs = (cent[lab] + spread * rng.standard_normal((n, d))).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64)
    return dict(d=d, ntotal=n, nlist=nlist, nprobe=1, centroids=cent, list_offsets=off, ids=ids, vecs=vecs)


@pytest.mark.parametrize("case", ["nlist_16384", "nlist_16385", "list_2048", "list_2049", "list_9000", "d_64", "d_48", "nq_16", "nq_15"])
def test_list_major_boundaries_pin_the_path_and_both_paths_agree(case, gpu, capfd):
    """The limits of the list-major kernels (ivf.hip ``lm_unusable_reason``): the planner counts at most 16 384 lists in LDS, the MFMA K
    chunk wants d % 32 == 0, and below 16 queries the one-launch query-major kernel is kept.  (Round 5: a list longer than the 2048
    entries the selector stages in LDS is no longer a limit -- its score row is worked on in place in the global scratch: cases
    list_2049 / list_9000, e.g. the one list all silence frames of a training set fall into.)  On each side of each limit: WHICH path ran (profiler names), that its answer equals the fp64 oracle, and -- a
    call of 64 queries or more that has to fall back says so ONCE on stderr instead of silently re-reading every list per query."""
    rng = np.random.default_rng(7)
    nq, d = 128, 32
    if case.startswith("nlist"):
        nlist = int(case.split("_")[1])
        idx = _tiny_index([2] * nlist, d, seed=1)
    elif case.startswith("list"):
        idx = _tiny_index([int(case.split("_")[1]), 5, 0, 40, 9], d, seed=2)
    elif case.startswith("d_"):
        d = int(case.split("_")[1])
        idx = _tiny_index([40, 3, 70, 0, 12, 33], d, seed=3)
    else:
        nq = int(case.split("_")[1])
        idx = _tiny_index([40, 3, 70, 0, 12, 33], d, seed=4)
    lm = case in ("nlist_16384", "list_2048", "list_2049", "list_9000", "d_64", "nq_16")
    # queries near the centroids of a few lists (the long list first), one of them an exact stored row
    pick = rng.integers(0, min(idx["nlist"], 64), size=nq)
    pick[: nq // 2] = 0
    q = (idx["centroids"][pick] + 0.05 * rng.standard_normal((nq, d))).astype(np.float32)
    q[1] = idx["vecs"][0]
    h = make(idx, gpu)
    capfd.readouterr()
    (D, I), names = _path_names(h, lambda: h.search(q, 8))
    err = capfd.readouterr().err
    assert ("ivf_plan" in names) == lm and ("ivf_select" in names) == lm, (case, names)
    if lm or nq < 64:
        assert "query-major scan" not in err, err
    else:
        assert err.count("query-major scan") == 1 and {"nlist_16385": "16384 lists", "d_48": "multiple of 32"}[case] in err, err
        h.search(q, 8)
        assert "query-major scan" not in capfd.readouterr().err  # once per index
    Dr, Ir, _ = ivf_oracle.search_c(idx, q, 8)
    assert np.array_equal(I, Ir), "%s: %d ids differ" % (case, int((I != Ir).sum()))
    assert np.array_equal(D, Dr)
    # the other path on the same call (forced): identical bits
    if lm:
        h.set_option("IVF_LM", 0)
        (D2, I2), names2 = _path_names(h, lambda: h.search(q, 8))
        assert "ivf_plan" not in names2 and np.array_equal(I2, I) and np.array_equal(D2, D)


def test_calls_beyond_the_one_gib_score_scratch_run_in_passes(gpu):
    """The list-major kernels keep their fp32 score scratch (queries x longest list) at or below 1 GiB.  Round 4 fell back to the
    query-major scan beyond that -- and (ADVICE) a ``reserve`` above the bound left the buffers at an earlier, smaller size while raising
    the handle's capacity, so that a later call under the bound overran them.  Now a call of any size runs in PASSES of the queries one
    scratch holds (``lm_buf_nq``): a 200 000-query call against a 1500-row list (1.2 GB of scores) = two passes, every result equal to the
    oracle, before and after smaller calls on the same handle."""
    idx = _tiny_index([1500, 40, 7, 0, 300], 32, seed=5)
    h = make(idx, gpu)
    rng = np.random.default_rng(1)
    pick = np.where(rng.random(200_000) < 0.5, 0, rng.integers(0, 5, 200_000))
    q = (idx["centroids"][pick] + 0.05 * rng.standard_normal((200_000, 32))).astype(np.float32)
    (_, I0), names = _path_names(h, lambda: h.search(q[:128], 8))  # scratch sized for 128 queries
    assert "ivf_plan" in names
    Dr, Ir, _ = ivf_oracle.search_c(idx, q, 8)
    h.profile(True)
    D, I = h.search(q, 8)  # 200000 x 1504 x 4 B = 1.2 GB > 1 GiB: two passes
    st = {s_["name"]: s_["launches"] for s_ in h.profile_read()}
    h.profile(False)
    assert st.get("ivf_plan") == 2 and st.get("ivf_select") == 2, st
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    (D2, I2), names = _path_names(h, lambda: h.search(q[:4096], 8))  # and a single pass again on the same (larger) buffers
    assert "ivf_plan" in names and np.array_equal(I2, Ir[:4096]) and np.array_equal(D2, Dr[:4096]) and np.array_equal(I2[:128], I0)
    feats = torch.from_numpy(q).to(gpu).contiguous()
    h.search_blend(feats, 0.75, 8)  # the fused blend follows its pass
    exp = ivf_oracle.blend_c(idx, q, Dr, ivf_oracle.search_c(idx, q, 8)[2], 0.75)
    fin = np.isfinite(exp).all(1)
    assert float(np.sqrt(np.mean((feats.cpu().numpy()[fin].astype(np.float64) - exp[fin]) ** 2))) <= 1e-5


def test_index_build_kmeans_lists_and_roundtrip(gpu, tmp_path):
    """web.py:544-571 on the GPU: k-means objective never increases, every vector sits in the list of its exact (fp64) nearest
    centroid with ids ascending inside a list, every centroid is the mean of its list after convergence steps, a vector
    queried against the built index finds itself, and the written file reads back identically."""
    import rvc_amd

    rng = np.random.default_rng(3)
    blobs = rng.standard_normal((40, 256)).astype(np.float32) * 3.0
    x = (blobs[rng.integers(0, 40, 6000)] + rng.standard_normal((6000, 256)).astype(np.float32)).astype(np.float32)
    index, obj = rvc_amd.IVFFlatHIP.train(x, niter=8, seed=7, device=gpu, return_objective=True)
    assert index.ntotal == 6000 and index.d == 256 and index.nprobe == 1
    assert index.nlist == synth.ivf_nlist(6000)
    assert np.all(np.diff(obj) <= 1e-6 * obj[:-1]), "k-means objective increased: %s" % obj
    assert obj[-1] < 0.8 * obj[0]
    path = str(tmp_path / "built.index")
    rvc_amd.write_index(index, path)
    d = ivf_oracle.read_index(path)
    off, ids, vecs, cent = d["list_offsets"], d["ids"], d["vecs"], d["centroids"]
    assert sorted(ids.tolist()) == list(range(6000))
    assert np.array_equal(vecs, x[ids])
    want = synth.assign_nearest(x, cent)  # exact fp64 argmin, ties -> lowest id
    got = np.repeat(np.arange(index.nlist), np.diff(off))
    assert np.array_equal(want[ids], got)
    for l in range(index.nlist):
        seg = ids[off[l]:off[l + 1]]
        assert np.all(np.diff(seg) > 0)
    D, I = index.search(x[:500], 1)
    assert np.array_equal(I[:, 0], np.arange(500)) and np.all(D[:, 0] == 0)
    again = rvc_amd.read_index(path, device=gpu)
    D2, I2 = again.search(x[100:164], 8)
    D1, I1 = index.search(x[100:164], 8)
    assert np.array_equal(I1, I2) and np.array_equal(D1, D2)


def test_index_build_handles_empty_lists_and_is_deterministic(gpu):
    """Two builds of rows with few distinct values give the same bytes, and every distinct row finds itself.  Despite the name, seed 1 draws
    rows of 15 distinct points for the 15 lists (oracle/ivf_build_oracle.py: no iteration splits anything), so no list ever empties here:
    empty lists and kmeans_split_empty are tested by tests/ivf_build_cases.py (dup_nlist40, dup_nlist14, zero_rows, ...) in
    tests/test_gpu_ivf_build.py."""
    import rvc_amd

    rng = np.random.default_rng(4)
    x = np.repeat(rng.standard_normal((30, 64)).astype(np.float32), 20, axis=0)  # 600 rows, only 30 distinct: most seeds collide
    a = rvc_amd.IVFFlatHIP.train(x, nlist=15, niter=5, seed=1, device=gpu)
    b = rvc_amd.IVFFlatHIP.train(x, nlist=15, niter=5, seed=1, device=gpu)
    assert torch.equal(a.blob(), b.blob())
    D, I = a.search(x[::20], 8)
    assert np.all(D[:, 0] == 0)


@pytest.mark.parametrize("dim", [768, 256])
def test_real_hubert_distribution_with_exact_duplicates(dim, gpu):
    """Index and queries drawn from the only REAL HuBERT features of the reference checkout (logs/mute/3_feature*/mute.npy,
    fixture mute_hubert): near-collinear rows, exact duplicate rows and an exact second copy of every row -- distance ties
    between different ids everywhere.  ids must still be bit-exact (ties -> lowest id), trained index included."""
    import rvc_amd
    from conftest import load_golden

    feats = load_golden("mute_hubert")["f%d" % dim]
    x = synth.make_mute_rows(feats)
    idx = synth.make_ivf_from_rows(x)
    h = make(idx, gpu)
    q = np.concatenate([feats, (feats[:60] + np.float32(1e-3)).astype(np.float32)])  # exact hits (score 0) and near hits
    D, I = h.search(q, 8)
    Dr, Ir = ivf_oracle.search(idx, q, 8)
    assert np.array_equal(I, Ir), "%d id mismatches on the real-feature index" % int((I != Ir).sum())
    assert np.array_equal(D, Dr)
    assert (D[:149, 0] == 0).all() and (D[:149, 1] == 0).all()  # every row has its exact second copy: a tie at distance 0
    # the GPU-built index (k-means on the same rows) answers its own oracle the same way
    built = rvc_amd.IVFFlatHIP.train(x, niter=4, device=gpu)
    assert np.array_equal(built.reconstruct_n(0, built.ntotal), x)
    Db, Ib = built.search(feats, 8)
    assert (Db[:, 0] == 0).all() and np.array_equal(x[Ib[:, 0]], feats)  # an exact hit is found in its own cell, lowest id first
    assert (Ib[:, 0] < Ib[:, 1]).all() and (Db[:, 1] == 0).all()


def test_reader_and_object_reject_what_they_do_not_support_with_a_clear_message(tmp_path, gpu):
    import struct

    import rvc_amd

    idx = synth.make_ivf(600, 64, seed=2)
    good = str(tmp_path / "ok.index")
    ivf_oracle.write_index(idx, good)
    buf = bytearray(open(good, "rb").read())
    pos_dm = 4 + 33 + 16 + 4 + 33 + 8 + 4 * idx["nlist"] * 64  # fourcc, header, nlist/nprobe, quantizer fourcc + header, count, centroids
    assert buf[pos_dm] == 0
    bad = bytearray(buf)
    bad[pos_dm] = 2  # DirectMap::Hashtable
    p = str(tmp_path / "hash.index")
    open(p, "wb").write(bad)
    with pytest.raises(rvc_amd.RvcmiError, match="direct map type 2"):
        rvc_amd.read_index(p, device=gpu)
    bad = bytearray(buf)
    struct.pack_into("<i", bad, 4 + 33 + 16 + 4 + 29, 0)  # quantizer metric_type -> METRIC_INNER_PRODUCT
    p = str(tmp_path / "ip.index")
    open(p, "wb").write(bad)
    with pytest.raises(rvc_amd.RvcmiError, match="quantizer"):
        rvc_amd.read_index(p, device=gpu)
    # list sizes that sum to ntotal modulo 2^64 (tests/test_cpu_ivf_format.py has the other crafted files): refused on the host
    import ivf_cases

    p = str(tmp_path / "wrapped.index")
    open(p, "wb").write(ivf_cases.crafted(**ivf_cases.WRAPPED_SIZES))
    with pytest.raises(rvc_amd.RvcmiError) as ei:
        rvc_amd.read_index(p, device=gpu)
    assert ei.value.code == rvc_amd._lib.ERR_IO
    h = rvc_amd.read_index(good, device=gpu)
    with pytest.raises(rvc_amd.RvcmiError, match="at most 8"):
        h.search(np.zeros((2, 64), np.float32), 9)
    ids = idx["ids"].copy()
    ids[ids == 5] = 10 ** 6  # add_with_ids-style gap: id 5 does not exist
    h2 = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], ids, idx["vecs"], device=gpu)
    with pytest.raises(rvc_amd.RvcmiError, match="id 5 is not in the index"):
        h2.reconstruct_n(0, 600)
    assert np.array_equal(h2.reconstruct_n(6, 100), idx["xb"][6:106])


def test_reduce_features_is_the_large_set_branch_of_the_index_recipe(gpu):
    """web.py:522-536: > 2e5 rows -> 10k k-means centres (here scaled down: threshold 3000 -> 64 centres).  The centres must
    be a valid k-means solution: every centre is the mean of the rows nearest to it, and the objective beats random rows."""
    import rvc_amd

    rng = np.random.default_rng(8)
    blobs = rng.standard_normal((64, 32)).astype(np.float32) * 4
    x = (blobs[rng.integers(0, 64, 6000)] + rng.standard_normal((6000, 32)).astype(np.float32)).astype(np.float32)
    assert rvc_amd.reduce_features(x[:2000], 64, threshold=3000, device=gpu) is not None and rvc_amd.reduce_features(x[:2000], 64, threshold=3000, device=gpu).shape == (2000, 32)
    c = rvc_amd.reduce_features(x, 64, threshold=3000, niter=15, device=gpu)
    assert c.shape == (64, 32) and c.dtype == np.float32 and np.isfinite(c).all()
    a = synth.assign_nearest(x, c)
    means = np.stack([x[a == j].astype(np.float64).mean(0) if (a == j).any() else c[j] for j in range(64)])
    assert np.abs(means - c).max() <= 5e-2  # a Lloyd fixed point up to the last iteration's movement
    obj = ((x - c[a]) ** 2).sum()
    c0 = x[rng.choice(6000, 64, replace=False)]
    assert obj < 0.8 * ((x - c0[synth.assign_nearest(x, c0)]) ** 2).sum()
    # the centres-only entry (rvcmi_kmeans) runs the SAME Lloyd iterations as the index build, without the add pass
    assert np.array_equal(c, rvc_amd.IVFFlatHIP.train(x, nlist=64, niter=15, device=gpu).centroids())


def test_reduce_features_quality_against_the_reference_minibatch_kmeans_call(gpu):
    """web.py:522-536 reduces a training set of more than 2e5 rows to 10k centres with
    ``MiniBatchKMeans(n_clusters=10000, batch_size=256 * n_cpu, compute_labels=False, init="random").fit(big_npy).cluster_centers_``.
    sklearn IS installable here, so this one library call of the index recipe can be held against the real thing (scaled down: 30000 x 64
    rows, 200 centres).  Its stochastic mini-batch trajectory is not reproducible bit for bit and nothing downstream depends on the
    individual centres, so what is measured is the quantity the reduction exists for: the k-means objective (fp64, every row to its
    nearest centre) on the same rows.

    What it found (round 5): on WELL-SEPARATED blobs -- the adversarial case for a random initialisation: some blobs start without a
    centre, others with two, and plain Lloyd iterations never repair that -- ``rvc_amd.reduce_features`` ended 1.43x ABOVE the reference call
    (4.15e6 vs 2.90e6; the optimum is 1.92e6): sklearn re-seeds low-count centres every batch, ours re-seeded only EMPTY ones.  The build now
    relocates centres (ivf_kmeans.hpp ``kmeans_relocate``: the centre that is cheapest to delete moves to the farthest point of the cluster with
    the largest distortion whenever the exact gain exceeds the deletion cost -- the objective cannot go up): **0.66x** the reference call's
    objective, i.e. the optimum.  On rows without such structure (second case: one broad Gaussian, the regime of real HuBERT features) no
    move passes the gain test and the result is the plain iterations': 0.98x."""
    sk = pytest.importorskip("sklearn.cluster")
    import rvc_amd

    rng = np.random.default_rng(0)
    cent = (rng.standard_normal((200, 64)) * 3).astype(np.float32)
    blobs = (cent[rng.integers(0, 200, 30000)] + rng.standard_normal((30000, 64))).astype(np.float32)
    broad = rng.standard_normal((30000, 64)).astype(np.float32)
    ratios = []
    for x, bound in ((blobs, 1.0), (broad, 1.02)):
        def objective(c):
            a = synth.assign_nearest(x, np.ascontiguousarray(c, np.float32))
            return float(((x.astype(np.float64) - np.asarray(c, np.float64)[a]) ** 2).sum())

        ref = sk.MiniBatchKMeans(n_clusters=200, verbose=False, batch_size=256 * 8, compute_labels=False, init="random", random_state=0).fit(x).cluster_centers_
        ours = rvc_amd.reduce_features(x, 200, threshold=1000, niter=10, device=gpu)
        assert ours.shape == ref.shape == (200, 64)
        o_ref, o_ours = objective(ref), objective(ours)
        ratios.append(o_ours / o_ref)
        assert o_ours <= bound * o_ref, "k-means objective %.4g vs the reference MiniBatchKMeans call's %.4g (x %.2f)" % (o_ours, o_ref, o_ours / o_ref)
    print("reduce_features / MiniBatchKMeans objective: blobs x%.3f, broad Gaussian x%.3f" % tuple(ratios))
