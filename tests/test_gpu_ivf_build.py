"""The index build on the device (rvcmi_ivf_build / rvcmi_ivf_train / rvcmi_kmeans behind IVFFlatHIP.train, .trained and kmeans) against
oracle/ivf_build_oracle.py, the build restated step by step in numpy fp64, on the table of tests/ivf_build_cases.py.

Centroids, list offsets, ids and vectors are compared bit for bit: a mean has no liberty (fp64, ascending ids, one division, one rounding), a
split centre is an fp32 product and a relocated centre is a copy of a row, and tests/test_cpu_ivf_build.py asserts for every case that no
decision of the run hangs on less than 1e-9 relative, which the device's summation order cannot cross.  The objective is a sum the device
orders differently: it is held to the bound of that, (n + d) * 2^-52 relative (at most n + d additions of non-negative fp64 terms at 2^-53
each, doubled for the rounding of the squares)."""
import re

import numpy as np
import pytest
import torch

import ivf_build_cases as bc
from oracle import ivf_oracle

pytestmark = pytest.mark.gpu

DEGENERATE = ["zero_rows", "dup_nlist40", "dup_nlist14"]  # duplicate centroids and empty lists: where searching the built index matters


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bar(name):
    n, d = bc.rows(name).shape
    return (n + d) * 2.0 ** -52


def close(got, want, name):
    return bool(np.all(np.abs(got - want) <= bar(name) * want))


_built = {}


def built(name, gpu, tmp_path_factory):
    """train() of a case, once: (index, objective, the written file read back by the python reader)"""
    if name not in _built:
        import rvc_amd

        index, obj = rvc_amd.IVFFlatHIP.train(bc.rows(name), device=gpu, return_objective=True, **bc.params(name))
        path = str(tmp_path_factory.mktemp("ivf_build") / (name + ".index"))
        rvc_amd.write_index(index, path)
        _built[name] = (index, obj, ivf_oracle.read_index(path))
    return _built[name]


@pytest.mark.parametrize("name", list(bc.CASES))
def test_built_index_equals_the_oracle(name, gpu, tmp_path_factory):
    x, o = bc.rows(name), bc.oracle(name)
    index, obj, f = built(name, gpu, tmp_path_factory)
    print("%s: objective device %s oracle %s, relative difference %s, bar %.3g"
          % (name, obj.tolist(), o["objective"].tolist(), (np.abs(obj - o["objective"]) / np.maximum(o["objective"], 1e-300)).tolist(), bar(name)))
    wrong = np.flatnonzero((bits(index.centroids()) != bits(o["centroids"])).any(axis=1))
    assert wrong.size == 0, "centroids %s differ from the oracle's" % wrong[:10].tolist()
    assert np.array_equal(bits(f["centroids"]), bits(o["centroids"]))
    assert f["ntotal"] == x.shape[0] and f["nlist"] == bc.params(name)["nlist"] and f["nprobe"] == 1
    assert np.array_equal(f["list_offsets"], o["list_offsets"])
    assert np.array_equal(f["ids"], o["ids"])
    assert np.array_equal(bits(f["vecs"]), bits(x[o["ids"]]))
    assert obj.shape == o["objective"].shape and close(obj, o["objective"], name)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_kmeans_and_trained_are_the_same_trajectory_without_the_last_assignment(name, gpu, tmp_path_factory):
    """rvcmi_kmeans and rvcmi_ivf_train: niter updates, no final assignment (the oracle's ``centres_only``, which is its full build less
    the last objective entry: tests/test_cpu_ivf_build.py); ``trained(x)`` + ``add(x)`` is ``train(x)`` byte for byte."""
    import rvc_amd

    x, o, p = bc.rows(name), bc.oracle(name), bc.params(name)
    got = rvc_amd.kmeans(x, p["nlist"], niter=p["niter"], seed=p["seed"], device=gpu)
    assert np.array_equal(bits(got), bits(o["centroids"]))
    t, obj = rvc_amd.IVFFlatHIP.trained(x, device=gpu, return_objective=True, **p)
    assert t.ntotal == 0 and np.array_equal(bits(t.centroids()), bits(o["centroids"]))
    assert obj.shape == (p["niter"],) and close(obj, o["objective"][:-1], name)
    t.add(x)
    assert torch.equal(t.blob(), built(name, gpu, tmp_path_factory)[0].blob())


@pytest.mark.parametrize("nprobe", [1, 3])
@pytest.mark.parametrize("name", DEGENERATE)
def test_search_on_the_degenerate_indices_equals_the_search_oracle(name, nprobe, gpu, tmp_path_factory):
    x = bc.rows(name)
    index, _, f = built(name, gpu, tmp_path_factory)
    cent, sizes = f["centroids"], np.diff(f["list_offsets"])
    assert int((sizes == 0).sum()) > 0, "no empty list"
    if name == "zero_rows":
        assert len(np.unique(cent, axis=0)) < len(cent), "no duplicate centroids"
    rng = np.random.default_rng(5)
    q = np.concatenate([x[::7], x[::11] + 0.01 * rng.standard_normal(x[::11].shape).astype(np.float32), cent,
                        rng.standard_normal((16, x.shape[1])).astype(np.float32)]).astype(np.float32)
    index.nprobe = nprobe
    try:
        D, I = index.search(q, 8)
    finally:
        index.nprobe = 1
    Dw, Iw = ivf_oracle.search(f, q, 8, nprobe=nprobe)
    assert np.array_equal(I, Iw)
    assert np.array_equal(D, Dw)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_objective_rises_only_where_the_oracle_splits_an_empty_list(name, gpu, tmp_path_factory):
    o, f = bc.oracle(name), bc.facts(name)
    _, obj, _ = built(name, gpu, tmp_path_factory)
    rise = np.diff(obj) > bar(name) * obj[:-1]
    if sum(f["splits"]) == 0:
        assert not rise.any(), "the objective rose without a split: %s" % obj.tolist()
    want = np.diff(o["objective"]) > bar(name) * o["objective"][:-1]
    assert not want[np.array(f["splits"], bool) == 0].any(), "the oracle's own objective rose in an iteration that split nothing"
    if name == "dup_nlist40":
        assert want[0] and obj[0] == 0.0 and obj[1] > 0.0
    assert np.array_equal(rise, want), "device %s oracle %s" % (obj.tolist(), o["objective"].tolist())


def _kernels(fn, gpu):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize(gpu)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(gpu)
    return sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})


@pytest.mark.parametrize("name,big", [("grid_n4096", True), ("grid_n4095", True), ("grid_n4032", False)])
def test_the_large_grid_assignment_kernel_runs_from_512_tiles_on(name, big, gpu):
    """coarse_assign_exact: k_coarse_gemm<2, 4> from 512 tiles of 128 lists x 64 rows on, k_coarse_gemm<1, 1> below.  4096 and 4095 rows are
    64 row tiles each (the last one of n = 4095 is a row short), 4032 rows are 63."""
    import rvc_amd

    names = _kernels(lambda: rvc_amd.IVFFlatHIP.train(bc.rows(name), device=gpu, **bc.params(name)), gpu)
    gemm = {m.group(1).replace(" ", "") for n in names for m in [re.search(r"k_coarse_gemm<([^>]*)>", n)] if m}
    print(name, sorted(gemm), [n for n in names if "k_coarse" in n])
    assert gemm == ({"2,4"} if big else {"1,1"}), names
