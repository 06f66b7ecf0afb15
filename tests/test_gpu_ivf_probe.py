"""nprobe > 1 on the scan kernels real indices use, and the row-group edges of their pipelined row loop (tests/ivf_probe_cases.py).

With ``min(nprobe, nlist) > 1`` a search is k_coarse_dist + k_coarse_select and then the query-major scan with its probe loop:
k_scan_v<4,16,2> at d = 256 (the legacy indices, which are the ones that carry nprobe = 9), k_scan_v<6,32,2> at d = 768, the generic
k_scan elsewhere (d = 64 here).  The list-major kernels refuse such a call.  Every comparison with the oracle asks for its bits, ids and
fp32 distances alike: tests/test_cpu_ivf_probe.py shows on the oracle alone that no summation order can change either on these cases.
Every input is a valid search."""
import numpy as np
import pytest
import torch

import ivf_probe_cases as cases
from oracle import glue_oracle, ivf_oracle, synth

pytestmark = pytest.mark.gpu

NPROBE_IDS = ["np1", "np2", "np9", "np_nlist", "np_nlist+3"]
LM_NAMES = {"ivf_plan", "ivf_select"}


def make(idx, gpu, nprobe=1):
    import rvc_amd

    h = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], nprobe=nprobe, device=gpu)
    assert h.nprobe == nprobe
    if nprobe == 1:
        h.set_option("IVF_LM", 0)  # 48 queries would go to the list-major kernels: the query-major scan is the one under test
    return h


def _path_names(h, fn):
    """fn() with the handle's profiler on -> (result, set of launch names)."""
    h.profile(True)
    r = fn()
    names = {st["name"] for st in h.profile_read()}
    h.profile(False)
    return r, names


def _same(got, exp, what):
    (D, I), (Dr, Ir) = got, exp
    bad = I != Ir
    assert not bad.any(), "%s: %d of %d ids differ from the oracle, first at query %d: got %s, expected %s" % (
        what, int(bad.sum()), I.size, int(np.argwhere(bad)[0][0]), I[np.argwhere(bad)[0][0]], Ir[np.argwhere(bad)[0][0]])
    badd = D != Dr
    assert not badd.any(), "%s: %d of %d distances differ from the oracle, first at query %d" % (what, int(badd.sum()), D.size, int(np.argwhere(badd)[0][0]))


def _search_all_k(h, q, gpu, what):
    """Every k, numpy and device-tensor queries -> {k: (D, I)}; the two entries must agree and no list-major kernel may have run."""
    out = {}
    qt = torch.from_numpy(np.array(q)).to(gpu)
    for k in cases.KS:
        (D, I), names = _path_names(h, lambda: h.search(np.array(q), k))
        assert {"ivf_coarse", "ivf_scan"} <= names and not (LM_NAMES & names), "%s k %d: launches %s" % (what, k, sorted(names))
        assert D.dtype == np.float32 and I.dtype == np.int64 and D.shape == I.shape == (q.shape[0], k)
        Dt, It = h.search(qt, k)
        assert Dt.is_cuda and It.is_cuda and It.dtype == torch.int64
        assert np.array_equal(It.cpu().numpy(), I) and np.array_equal(Dt.cpu().numpy(), D), "%s k %d: tensor and numpy queries disagree" % (what, k)
        out[k] = (D, I)
    print("%s: launches %s" % (what, sorted(names)))
    return out


# ---- 1. every kernel x nprobe x k against the oracle ------------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(5), ids=NPROBE_IDS)
@pytest.mark.parametrize("d", cases.DIMS)
def test_every_kernel_every_nprobe_equals_the_oracle(d, which, gpu):
    idx, q, planted = cases.probe_case(d)
    nprobe = cases.nprobes(idx["nlist"])[which]
    h = make(idx, gpu, nprobe)
    Dr, Ir = cases.expected(d, nprobe)
    got = _search_all_k(h, q, gpu, "d %d nprobe %d" % (d, nprobe))
    for k in cases.KS:
        _same(got[k], (Dr[:, :k], Ir[:, :k]), "d %d nprobe %d k %d" % (d, nprobe, k))
    # the planted row: distance 0 on every copy a probed list holds, the lowest id first
    D, I = got[8]
    copies = 2 if nprobe == 1 else 3
    assert np.all(D[0, :copies] == 0) and D[0, copies] > 0
    assert list(I[0, :copies]) == list(planted["ids"][3 - copies:])
    assert bool((I < 0).any()) == (nprobe <= 2)


# ---- 2. the specialised scans against the generic one -----------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(5), ids=NPROBE_IDS)
@pytest.mark.parametrize("d", [256, 768])
def test_specialised_scan_equals_the_generic_scan(d, which, gpu):
    idx, q, _ = cases.probe_case(d)
    nprobe = cases.nprobes(idx["nlist"])[which]
    h = make(idx, gpu, nprobe)
    spec = _search_all_k(h, q, gpu, "d %d nprobe %d specialised" % (d, nprobe))
    h.set_option("IVF_GENERIC", 1)
    gen = _search_all_k(h, q, gpu, "d %d nprobe %d generic" % (d, nprobe))
    h.set_option("IVF_GENERIC", None)
    for k in cases.KS:
        _same(spec[k], gen[k], "d %d nprobe %d k %d, specialised against generic" % (d, nprobe, k))


# ---- 3. the blend over results merged from several lists --------------------------------------------------------------------------

def _equal_bits(a, b):
    """Equal values everywhere, NaN rows (an exact hit: weight inf / inf) in the same places."""
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("nprobe", [2, 9])
@pytest.mark.parametrize("d", cases.DIMS)
def test_blend_with_several_probed_lists(d, nprobe, gpu):
    """``search_blend`` without the guard is the fused ``bfeats`` branch of k_scan_v at d = 256 / 768 (in place: the queries are the
    buffer it writes) and k_blend at d = 64; with the guard it is k_blend everywhere."""
    idx, q, _ = cases.probe_case(d)
    h = make(idx, gpu, nprobe)
    for k in (8, 5):  # pairwise / sequential weight sum
        exp = ivf_oracle.search_blend(cases.with_nprobe(idx, nprobe), q, 0.75, k)
        feats = torch.from_numpy(np.array(q)).to(gpu)
        ret, names = _path_names(h, lambda: h.search_blend(feats, 0.75, k))
        assert ret.data_ptr() == feats.data_ptr() and not (LM_NAMES & names)
        assert ("ivf_blend" in names) == (d == 64), "d %d: launches %s" % (d, sorted(names))
        got = feats.cpu().numpy()
        nan = np.isnan(exp).any(axis=1)
        assert nan[0] and np.isnan(exp[0]).all()  # query 0 is the planted row: distance 0
        assert np.array_equal(np.isnan(got).any(axis=1), nan) and np.array_equal(np.isnan(got).all(axis=1), nan)
        err = float(np.abs(got[~nan] - exp[~nan]).max())
        print("d %d nprobe %d k %d: blend max abs error %.3g, launches %s" % (d, nprobe, k, err, sorted(names)))
        assert err <= 1e-5
        # the realtime guard: a padded result anywhere among the k (nprobe 2 at k = 8; at k = 5 as the oracle says) skips the whole
        # call; none (nprobe 9) = the unguarded call's bits
        padded = bool((cases.expected(d, nprobe)[1][:, :k] < 0).any())
        assert padded == (nprobe == 2) or k != 8
        guarded = torch.from_numpy(np.array(q)).to(gpu)
        _, names = _path_names(h, lambda: h.search_blend(guarded, 0.75, k, skip_if_short=True))
        assert "ivf_blend" in names and not (LM_NAMES & names)
        if padded:
            assert np.array_equal(guarded.cpu().numpy(), q), "a result was padded: the guarded call must leave the features alone"
        else:
            assert _equal_bits(guarded.cpu().numpy(), got), "guarded (k_blend) and unguarded call differ with no result padded"


def test_glue_blend_expand_at_nprobe_9(gpu):
    """The realtime glue on a legacy index: 12 rows through ``retrieve_blend_expand(realtime_guard=True)``, and a bank of three such
    blocks whose sessions equal their solo calls.  The expansion copies rows and the protect mix is a convex combination of the
    blended and the original row, so the blend's 1e-5 bar carries over unchanged."""
    import rvc_amd

    d, nq, p_len, protect = 256, 12, 23, 0.33
    idx, q, _ = cases.probe_case(d)
    h = make(idx, gpu, 9)
    f = torch.from_numpy(np.array(q[1:1 + 3 * nq])).reshape(3, nq, d)  # (query 0 is the exact hit: a NaN row)
    pitchf = torch.stack([synth.make_f0(1, 80)[0][30 + s: 30 + s + 2 * nq] for s in range(3)]).contiguous()  # unvoiced, then voiced frames
    kw = dict(protect=protect, p_len=p_len, realtime_guard=True)
    solo = []
    for s in range(3):
        got = rvc_amd.glue.retrieve_blend_expand(f[s:s + 1].to(gpu), h, 0.75, pitchf[s:s + 1].to(gpu), **kw).cpu()
        blended = torch.from_numpy(ivf_oracle.search_blend(cases.with_nprobe(idx, 9), f[s].numpy(), 0.75)).unsqueeze(0)
        ref = glue_oracle.expand_protect(blended, f[s:s + 1], pitchf[s:s + 1], protect, p_len)
        plain = glue_oracle.expand_protect(f[s:s + 1], f[s:s + 1], pitchf[s:s + 1], protect, p_len)
        assert got.shape == ref.shape == (1, p_len, d)
        err = float((got - ref).abs().max())
        print("session %d: max abs error %.3g" % (s, err))
        assert err <= 1e-5
        assert float((got - plain).abs().max()) > 1e-2, "nothing was blended: no result is padded at nprobe 9"
        solo.append(got[0])
    bank = rvc_amd.glue.retrieve_blend_expand_batch(f.to(gpu), h, 0.75, pitchf.to(gpu), **kw).cpu()
    assert bank.shape == (3, p_len, d)
    for s in range(3):
        assert torch.equal(bank[s], solo[s]), "session %d of the bank differs from its solo call" % s


# ---- 4. ties between centroids at the nprobe cut ---------------------------------------------------------------------------------

@pytest.mark.parametrize("nprobe", [cases.CUT_STRADDLE, cases.CUT_INSIDE], ids=["straddle", "inside"])
@pytest.mark.parametrize("d", cases.DIMS)
def test_coarse_cut_between_identical_centroids(d, nprobe, gpu):
    """Two bit-identical centroids at ranks 3 and 4 of query 0.  nprobe 3 probes the lower list id only -- the other list holds the
    nearest row of the index, which must NOT come back; nprobe 4 probes both and it comes back first."""
    idx, q, info = cases.cut_case(d)
    h = make(idx, gpu, nprobe)
    exp = ivf_oracle.search(idx, q, 8, nprobe=nprobe)
    got = _search_all_k(h, q, gpu, "cut case d %d nprobe %d" % (d, nprobe))
    for k in cases.KS:
        _same(got[k], (exp[0][:, :k], exp[1][:, :k]), "cut case d %d nprobe %d k %d" % (d, nprobe, k))
    I = got[8][1]
    assert (info["near_id"] in I[0]) == (nprobe == cases.CUT_INSIDE) and (I[0, 0] == info["near_id"]) == (nprobe == cases.CUT_INSIDE)


# ---- 5. nprobe changing on a handle that has searched ----------------------------------------------------------------------------

def test_nprobe_transitions_on_one_handle(gpu):
    """``reserve()`` keeps the query capacity, the probe capacity, both coarse scratches and the list-major capacities behind one early
    return.  Up and down in nprobe and in query count on one handle, one explicit reserve in between: every step equals the oracle,
    and the (1, >= 16 queries) steps are back on the list-major kernels."""
    idx, _, _ = cases.probe_case(256)
    q = cases.transition_queries()
    import rvc_amd

    h = rvc_amd.IVFFlatHIP.from_arrays(idx["centroids"], idx["list_offsets"], idx["ids"], idx["vecs"], nprobe=1, device=gpu)
    for i, step in enumerate(cases.TRANSITIONS):
        if step == "reserve":
            h.nprobe = cases.TRANSITIONS[i + 1][0]
            h.reserve(cases.RESERVE_NQ)
            continue
        nprobe, nq = step
        h.nprobe = nprobe
        assert h.nprobe == nprobe
        (D, I), names = _path_names(h, lambda: h.search(np.array(q[:nq]), 8))
        what = "step %d (nprobe %d, %d queries)" % (i, nprobe, nq)
        print("%s: launches %s" % (what, sorted(names)))
        Dr, Ir = cases.transition_expected(nprobe)
        _same((D, I), (Dr[:nq], Ir[:nq]), what)
        lm = nprobe == 1 and nq >= 16
        assert ("ivf_plan" in names) == lm and ("ivf_select" in names) == lm, "%s: launches %s" % (what, sorted(names))


# ---- 6. nprobe survives storage --------------------------------------------------------------------------------------------------

def test_nprobe_survives_file_and_blob(tmp_path, gpu):
    """A legacy file's nprobe = 9 is what ``read_index`` hands to the scan: written and read back, and through a blob."""
    import rvc_amd

    idx, q, _ = cases.probe_case(256)
    Dr, Ir = cases.expected(256, 9)
    h = make(idx, gpu, 9)
    _same(h.search(np.array(q), 8), (Dr, Ir), "the handle itself")
    p = str(tmp_path / "legacy_nprobe_9.index")
    rvc_amd.write_index(h, p)
    assert ivf_oracle.read_index(p)["nprobe"] == 9  # (the independent python reader)
    h2 = rvc_amd.read_index(p, gpu)
    assert h2.nprobe == 9
    _same(h2.search(np.array(q), 8), (Dr, Ir), "write_index -> read_index")
    p2 = str(tmp_path / "legacy_py.index")
    ivf_oracle.write_index(cases.with_nprobe(idx, 9), p2)  # the python writer's file, as an old training script left it
    h3 = rvc_amd.read_index(p2, gpu)
    assert h3.nprobe == 9
    _same(h3.search(np.array(q), 8), (Dr, Ir), "python writer -> read_index")
    h4 = rvc_amd.IVFFlatHIP.from_blob(h.blob().clone())
    assert h4.nprobe == 9
    _same(h4.search(np.array(q), 8), (Dr, Ir), "blob -> from_blob")
