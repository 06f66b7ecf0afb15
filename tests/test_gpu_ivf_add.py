"""``index.add`` on the device and the faiss-style ``index_factory`` / ``train`` / ``add`` recipe (web.py:547-571) against the CPU
oracle: ``synth.make_ivf_from_rows(x, nlist, kmeans_iters=0, init=C)`` is the layout sequential adds leave for fixed centroids C
(exact fp64 assignment, ties to the lowest list, ids ascending inside a list).  Files are compared byte for byte where two routes
must give the same index, array for array against the oracle's reader otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ivf_oracle, synth

pytestmark = pytest.mark.gpu
SKEL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "skeleton")
FLT_MAX = np.float32(3.4028234663852886e38)


def empty(C, gpu, nprobe=1):
    """A trained, empty index with the fixed centroids C."""
    import rvc_amd

    nlist, d = C.shape
    return rvc_amd.IVFFlatHIP.from_arrays(C, np.zeros(nlist + 1, np.int64), np.zeros(0, np.int64), np.zeros((0, d), np.float32),
                                          nprobe=nprobe, device=gpu)


def file_of(h, tmp_path, name):
    import rvc_amd

    path = str(tmp_path / name)
    rvc_amd.write_index(h, path)
    return open(path, "rb").read(), ivf_oracle.read_index(path)


def layout(x, C):
    return synth.make_ivf_from_rows(x, C.shape[0], kmeans_iters=0, init=C)


def assert_layout(got, exp):
    assert got["ntotal"] == exp["ntotal"] and got["nlist"] == exp["nlist"] and got["d"] == exp["d"]
    assert np.array_equal(got["centroids"], exp["centroids"])
    assert np.array_equal(got["list_offsets"], exp["list_offsets"])
    assert np.array_equal(got["ids"], exp["ids"])
    assert np.array_equal(got["vecs"], exp["vecs"])


def rows_and_centroids(n, d, nlist, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=np.float32)
    C = x[rng.choice(n, size=nlist, replace=False)] + 0.25 * rng.standard_normal((nlist, d), dtype=np.float32)
    return x, np.ascontiguousarray(C, dtype=np.float32)


@pytest.mark.parametrize("n,d,nlist", [(300, 16, 7), (600, 768, 16), (500, 256, 11)])
def test_layout_of_an_add_into_an_empty_index_equals_the_oracle(n, d, nlist, gpu, tmp_path):
    x, C = rows_and_centroids(n, d, nlist, seed=n + d)
    # no planted tie here: best and second-best centroid are apart, so only the exact rule itself is compared
    diff = x.astype(np.float64)[:, None, :] - C.astype(np.float64)[None, :, :]
    two = np.sort(np.einsum("ijk,ijk->ij", diff, diff), axis=1)[:, :2]
    assert np.all(two[:, 1] - two[:, 0] > 1e-9 * two[:, 1])
    h = empty(C, gpu)
    assert h.is_trained and h.ntotal == 0
    assert h.add(x) is None
    assert (h.ntotal, h.d, h.nlist, h.nprobe) == (n, d, nlist, 1)
    _, got = file_of(h, tmp_path, "a.index")
    assert_layout(got, layout(x, C))


def test_batches_equal_one_shot_and_runs_are_deterministic(gpu, tmp_path):
    x, C = rows_and_centroids(300, 16, 7, seed=11)

    def run(cuts, name):
        h = empty(C, gpu)
        for a, b in zip(cuts[:-1], cuts[1:]):
            h.add(x[a:b])
        return file_of(h, tmp_path, name)[0]

    one = run([0, 300], "one.index")
    assert run([0, 1, 8, 108, 300], "batched.index") == one  # batches of 1, 7, 100 and the rest
    assert run([0, 1, 8, 108, 300], "again.index") == one
    assert run([0, 300], "one2.index") == one


@pytest.mark.parametrize("n,d,nlist", [(2000, 16, 20), (1500, 256, None)])
def test_trained_then_add_equals_the_one_shot_build(n, d, nlist, gpu, tmp_path):
    import rvc_amd

    x = synth.make_clustered_rows(n, d, 12, seed=n)
    built, obj = rvc_amd.IVFFlatHIP.train(x, nlist=nlist, niter=3, seed=5, device=gpu, return_objective=True)
    h, obj_t = rvc_amd.IVFFlatHIP.trained(x, nlist=nlist, niter=3, seed=5, device=gpu, return_objective=True)
    assert h.ntotal == 0 and h.nlist == built.nlist and h.nprobe == 1 and h.is_trained
    assert np.array_equal(h.centroids(), built.centroids()) and np.array_equal(obj_t, obj[:3])
    trained_bytes, trained_file = file_of(h, tmp_path, "trained.index")
    assert trained_file["ntotal"] == 0 and np.array_equal(trained_file["centroids"], built.centroids())
    h.add(x)
    built_bytes, built_file = file_of(built, tmp_path, "built.index")
    assert file_of(h, tmp_path, "added.index")[0] == built_bytes
    assert_layout(built_file, layout(x, built.centroids()))  # the refactored build itself, against the oracle
    # the same rows in the reference's batches (web.py:561-563)
    h2 = rvc_amd.IVFFlatHIP.trained(x, nlist=nlist, niter=3, seed=5, device=gpu)
    for i in range(0, n, 512):
        h2.add(x[i:i + 512])
    assert file_of(h2, tmp_path, "added2.index")[0] == built_bytes


def test_skew_every_row_in_one_list_longer_than_lds(gpu, tmp_path):
    d = 4
    C = np.concatenate([np.zeros((1, d), np.float32), 1000 * np.eye(d, dtype=np.float32)])  # centroid 0 at the origin
    rng = np.random.default_rng(4)
    x0 = (0.01 * rng.standard_normal((40000, d))).astype(np.float32)  # all in list 0: a 320 KB segment of new ids
    x1 = (C[3] + 0.01 * rng.standard_normal((10, d))).astype(np.float32)
    h = empty(C, gpu)
    h.add(x0)
    _, got0 = file_of(h, tmp_path, "skew0.index")
    assert list(np.diff(got0["list_offsets"])) == [40000, 0, 0, 0, 0]
    assert_layout(got0, layout(x0, C))
    h.add(x1)
    _, got = file_of(h, tmp_path, "skew1.index")
    assert list(np.diff(got["list_offsets"])) == [40000, 0, 0, 10, 0]  # the empty lists stay empty
    assert_layout(got, layout(np.concatenate([x0, x1]), C))
    assert np.array_equal(h.reconstruct_n(39990, 20), np.concatenate([x0[-10:], x1]))


def test_ties_go_to_the_lower_list_and_duplicates_keep_id_order(gpu, tmp_path):
    rng = np.random.default_rng(6)
    d = 16
    C = (4 * rng.standard_normal((5, d))).astype(np.float32)
    C[3] = C[1]  # two identical centroids: an exact distance tie for every row
    x = (C[rng.integers(0, 5, size=200)] + 0.3 * rng.standard_normal((200, d))).astype(np.float32)
    x[50:60] = x[5]      # duplicates inside one add ...
    x[150:155] = x[5]    # ... and across adds
    x[199] = x[120]
    h = empty(C, gpu)
    h.add(x[:100])
    h.add(x[100:])
    _, got = file_of(h, tmp_path, "ties.index")
    exp = layout(x, C)
    assert_layout(got, exp)
    sizes = np.diff(got["list_offsets"])
    assert sizes[3] == 0 and sizes[1] > 0
    D, I = h.search(x[5:6].copy(), 8)
    assert list(I[0]) == [5] + list(range(50, 57)) and np.all(D[0] == 0)  # 16 copies of the row: the lowest ids, ascending


@pytest.mark.parametrize("nprobe", [1, 3])
def test_search_after_add_uses_no_stale_list_statistics(nprobe, gpu):
    """A search of 64 queries (the list-major kernels: row norms, largest norm, longest list) BEFORE the add, then rows 100 times
    larger into one list: a new largest norm and a new longest list.  The next search must equal the oracle on the new index."""
    rng = np.random.default_rng(9)
    d, nlist = 32, 6
    C = (3 * rng.standard_normal((nlist, d))).astype(np.float32)
    x0 = (C[rng.integers(0, nlist, size=240)] + rng.standard_normal((240, d))).astype(np.float32)
    q = (C[rng.integers(0, nlist, size=64)] + rng.standard_normal((64, d))).astype(np.float32)
    h = empty(C, gpu, nprobe=nprobe)
    h.add(x0)
    idx0 = dict(layout(x0, C), nprobe=nprobe)
    D, I = h.search(q, 8)
    Dr, Ir = ivf_oracle.search(idx0, q, 8)
    assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    x1 = (100 * (C[2] + rng.standard_normal((150, d)))).astype(np.float32)
    h.add(x1)
    idx1 = dict(layout(np.concatenate([x0, x1]), C), nprobe=nprobe)
    sizes = np.diff(idx1["list_offsets"])
    assert sizes.max() > np.diff(idx0["list_offsets"]).max() and np.abs(x1).max() > 10 * np.abs(x0).max()
    q2 = q.copy()
    q2[::4] = x1[:16] * np.float32(1.001)  # queries out among the large rows, the rest as before
    D, I = h.search(q2, 8)
    Dr, Ir = ivf_oracle.search(idx1, q2, 8)
    assert np.array_equal(I, Ir), "%d id mismatches" % int((I != Ir).sum())
    assert np.array_equal(D, Dr)
    Dt, It = h.search(torch.from_numpy(q2).to(gpu), 8)
    assert np.array_equal(It.cpu().numpy(), Ir)


def test_pos_last_reconstruct_and_blend_after_adds(gpu):
    rng = np.random.default_rng(12)
    d, nlist = 16, 20
    C = (2 * rng.standard_normal((nlist, d))).astype(np.float32)
    parts = [rng.standard_normal((m, d), dtype=np.float32) for m in (25, 1, 34)]  # ~3 rows per list: shorter than k = 8
    h = empty(C, gpu)
    for p in parts:
        h.add(p)
    x = np.concatenate(parts)
    assert np.array_equal(h.reconstruct_n(0, h.ntotal), x)
    assert np.array_equal(h.reconstruct_n(24, 3), x[24:27])
    idx = layout(x, C)
    q = rng.standard_normal((40, d), dtype=np.float32)
    D, I = h.search(q, 8)
    Dr, Ir = ivf_oracle.search(idx, q, 8)
    assert np.array_equal(I, Ir) and (I == -1).any() and np.array_equal(D, Dr)
    exp = ivf_oracle.blend(q, Dr, Ir, x, 0.75)  # ids of -1 select big_npy[-1] = the row added last
    got = h.search_blend(torch.from_numpy(q).to(gpu), 0.75).cpu().numpy()
    assert np.abs(got - exp).max() <= 1e-5


def test_add_to_indices_from_a_file_and_from_an_adopted_blob(gpu, tmp_path):
    import rvc_amd

    x, C = rows_and_centroids(400, 32, 9, seed=21)
    a, b = x[:250], x[250:]
    first = empty(C, gpu)
    first.add(a)
    path = str(tmp_path / "first.index")
    rvc_amd.write_index(first, path)
    exp = layout(x, C)
    # from a file
    r = rvc_amd.read_index(path, device=gpu)
    r.add(b)
    ref_bytes, got = file_of(r, tmp_path, "r.index")
    assert_layout(got, exp)
    # from an adopted blob: the adopted tensor is left as it was, the handle moves to a blob of its own
    t = first.blob()
    keep = t.clone()
    ad = rvc_amd.IVFFlatHIP.from_blob(t)
    ad.add(torch.from_numpy(b).to(gpu))  # a CUDA tensor, read in place
    assert torch.equal(t, keep)
    assert file_of(ad, tmp_path, "ad.index")[0] == ref_bytes  # ... and equals the numpy route, byte for byte
    assert file_of(rvc_amd.IVFFlatHIP.from_blob(t), tmp_path, "t.index")[0] == open(path, "rb").read()
    again = rvc_amd.IVFFlatHIP.from_blob(ad.blob())
    assert again.ntotal == 400 and file_of(again, tmp_path, "again.index")[0] == ref_bytes
    again.add(a[:3].astype(np.float64))  # any float dtype from the host
    assert again.ntotal == 403 and np.array_equal(again.reconstruct_n(400, 3), a[:3])


def test_empty_index_zero_rows_and_errors_leave_the_index_unchanged(gpu, tmp_path):
    import rvc_amd

    x, C = rows_and_centroids(120, 16, 5, seed=33)
    h = empty(C, gpu)
    q = x[:20].copy()
    D, I = h.search(q, 8)
    assert np.all(I == -1) and np.all(D == FLT_MAX)
    Dl, Il = h.search(np.concatenate([q, q, q, q]), 8)
    assert np.all(Il == -1) and np.all(Dl == FLT_MAX)
    h.add(x)
    before = file_of(h, tmp_path, "before.index")[0]
    h.add(x[:0])
    h.add(torch.empty(0, 16, device=gpu))
    assert h.ntotal == 120 and file_of(h, tmp_path, "zero.index")[0] == before
    xt = torch.from_numpy(x).to(gpu)
    for bad in (np.zeros((3, 17), np.float32), np.zeros(16, np.float32), xt[:, :8], xt.t()[:16, :16], xt.half(), torch.from_numpy(x),
                torch.zeros(3, 20, device=gpu)):
        with pytest.raises(ValueError):
            h.add(bad)
    assert h.ntotal == 120 and file_of(h, tmp_path, "after.index")[0] == before
    # the factory object
    for desc in ("IVF16,PQ128x4fs,RFlat", "IVF,Flat", "Flat", "IVF0,Flat", "IVF16,Flat "):
        with pytest.raises(ValueError, match="IVF<nlist>,Flat"):
            rvc_amd.index_factory(16, desc, device=gpu)
    f = rvc_amd.index_factory(16, "IVF5,Flat", device=gpu)
    assert isinstance(f, rvc_amd.IVFFlatHIP) and rvc_amd.extract_index_ivf(f) is f
    assert (f.is_trained, f.ntotal, f.d, f.nlist, f.nprobe) == (False, 0, 16, 5, 1)
    f.nprobe = 2
    assert f.nprobe == 2
    for call in (lambda: f.add(x), lambda: f.search(q, 8), lambda: rvc_amd.write_index(f, str(tmp_path / "no.index")),
                 lambda: f.reconstruct_n(0, 0), lambda: f.blob()):
        with pytest.raises(rvc_amd.RvcmiError, match="not trained"):
            call()
    with pytest.raises(rvc_amd.RvcmiError, match="at least nlist"):
        f.train(x[:4])
    with pytest.raises(ValueError):
        f.train(np.zeros((50, 12), np.float32))
    assert not f.is_trained and f.ntotal == 0
    f.train(x)
    assert f.is_trained and f.ntotal == 0 and f.nprobe == 2 and f.nlist == 5
    cent = f.centroids()
    f.train(x[:60])  # a second train is a no-op
    assert np.array_equal(f.centroids(), cent)
    f.add(x)
    assert f.ntotal == 120
    f.nprobe = 1
    _, got = file_of(f, tmp_path, "f.index")
    assert_layout(got, layout(x, cent))
    Df, If = f.search(q, 8)
    Dr, Ir = ivf_oracle.search(layout(x, cent), q, 8)
    assert np.array_equal(If, Ir) and np.array_equal(Df, Dr)


def test_the_reference_index_recipe_runs_behind_the_shim(gpu, tmp_path):
    """web.py:547-571 in this test's own words, through the module-level ``faiss`` of the unmodified pipeline module, faiss absent."""
    import rvc_amd

    def purge():
        for m in [m for m in sys.modules if m.split(".")[0] in ("rvc", "infer", "faiss")]:
            del sys.modules[m]

    purge()
    sys.path.insert(0, SKEL)
    try:
        rvc_amd.install(index_build=True, device=gpu)
        import infer.modules.vc.pipeline as pl

        faiss = pl.faiss
        big_npy = synth.make_clustered_rows(1200, 768, 30, seed=3)
        n_ivf = min(int(16 * np.sqrt(big_npy.shape[0])), big_npy.shape[0] // 39)
        assert n_ivf == 30
        index = faiss.index_factory(768, "IVF%s,Flat" % n_ivf)
        index_ivf = faiss.extract_index_ivf(index)
        index_ivf.nprobe = 1
        index.train(big_npy)
        trained_path = str(tmp_path / ("trained_IVF%s_Flat_nprobe_%s.index" % (n_ivf, index_ivf.nprobe)))
        faiss.write_index(index, trained_path)
        for i in range(0, big_npy.shape[0], 500):
            index.add(big_npy[i:i + 500])
        added_path = str(tmp_path / ("added_IVF%s_Flat_nprobe_%s.index" % (n_ivf, index_ivf.nprobe)))
        faiss.write_index(index, added_path)
        trained, added = ivf_oracle.read_index(trained_path), ivf_oracle.read_index(added_path)
        assert trained["ntotal"] == 0 and trained["nlist"] == 30 and trained["nprobe"] == 1
        assert np.array_equal(trained["centroids"], index.centroids()) and np.isfinite(trained["centroids"]).all()
        assert_layout(added, layout(big_npy, trained["centroids"]))
        with pytest.raises(ValueError, match="IVF<nlist>,Flat"):
            faiss.index_factory(768, "IVF%s,PQ128x4fs,RFlat" % n_ivf)
        # the file serves the inference side as any other
        again = faiss.read_index(added_path)
        assert again.ntotal == 1200 and np.array_equal(again.reconstruct_n(0, again.ntotal), big_npy)
        rvc_amd.uninstall()
        assert "faiss" not in sys.modules
        purge()
        rvc_amd.install(device=gpu)  # the default stays as it was
        import infer.modules.vc.pipeline as pl2

        with pytest.raises(AttributeError, match="faiss is not installed"):
            pl2.faiss.index_factory(768, "IVF16,Flat")
        with pytest.raises(AttributeError, match="faiss is not installed"):
            pl2.faiss.extract_index_ivf(index)
    finally:
        rvc_amd.uninstall()
        sys.path.remove(SKEL)
        purge()
    assert "faiss" not in sys.modules
