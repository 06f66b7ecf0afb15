"""The index build's oracle (oracle/ivf_build_oracle.py) and its table of cases (tests/ivf_build_cases.py) on the CPU:

* every case is admissible (each decision that hangs on a distance is an exact tie of equal terms or at least 1e-9 clear, so the device's
  summation order cannot change it) and shows the facts it is in the table for;
* every named wrong variant of the oracle changes the final centroids of at least one case: the table is not blind to that kind of bug;
* the host steps of csrc/ivf_kmeans.hpp, run by tests/host/ivf_format_main.cpp (``steps``, ``seeds``) as a child process, equal the oracle's
  step functions bit for bit on hand-made updates at nlist 40 and 19 that reach the `used` / `moved[nn]` skips, a local cursor ahead of the
  global one, both breaks and the cap on the moves.

The program is built as in tests/test_cpu_ivf_format.py: g++, ``RVCMI_HOST_TEST_CXXFLAGS`` adds flags (e.g. ``-O1 -g -fsanitize=address,undefined
-fno-sanitize-recover=all``), nothing is loaded into Python."""
import os
import shlex
import struct
import subprocess

import numpy as np
import pytest

import ivf_build_cases as bc
from oracle import ivf_build_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "retrieval-based-voice-conversion-webui_amd", "csrc")
SMALL = [n for n in bc.CASES if not n.startswith(("grid_", "two_chunks"))]  # (the variants are run on these: the large ones take seconds each)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_the_table_and_the_statements_cover_each_other():
    assert set(bc.MUST) == set(bc.CASES)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_case_is_admissible_and_shows_what_it_is_there_for(name):
    o, f = bc.oracle(name), bc.facts(name)
    rep = o["report"]
    assert all(r.get("ties_unequal", 0) == 0 and r.get("nn_ties_unequal", 0) == 0 for r in rep), "an exact tie of sums with unequal terms"
    small = {k: v for r in rep for k, v in bo.margins(r).items() if v < bo.MARGIN}
    assert not small and bo.admissible(rep), "margins below %g: %s" % (bo.MARGIN, small)
    for text, holds in bc.MUST[name]:
        assert holds(f, o), "%s no longer shows: %s (%s)" % (name, text, f)
    n, nlist, niter = bc.rows(name).shape[0], bc.params(name)["nlist"], bc.params(name)["niter"]
    assert o["objective"].shape == (niter + 1,) and o["centroids"].shape == (nlist, bc.rows(name).shape[1])
    assert o["list_offsets"][-1] == n and sorted(o["ids"].tolist()) == list(range(n))


def test_niter_3_and_4_differ_and_centres_only_is_the_same_trajectory():
    a, b = bc.oracle("moves_niter3"), bc.oracle("moves_niter4")
    assert not np.array_equal(bits(a["centroids"]), bits(b["centroids"]))
    assert a["objective"][0] == b["objective"][0] and a["objective"][1] != b["objective"][1]  # (niter 4 relocates in its first update)
    for name in ("moves_niter4", "dup_nlist14"):
        full, c = bc.oracle(name), bc.oracle(name, centres_only=True)
        assert np.array_equal(bits(full["centroids"]), bits(c["centroids"])) and c["list_offsets"] is None
        assert np.array_equal(full["objective"][:-1], c["objective"])


@pytest.mark.parametrize("variant", bo.VARIANTS)
def test_each_wrong_variant_changes_the_centroids_of_some_case(variant):
    changed = [n for n in SMALL if not np.array_equal(bits(bc.oracle(n)["centroids"]), bits(bc.oracle(n, variant=variant)["centroids"]))]
    assert changed, "no case of the table would notice a build with %s" % variant


# ---- the host steps themselves ----
@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ivf_build") / "ivf_format_main")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + shlex.split(os.environ.get("RVCMI_HOST_TEST_CXXFLAGS", ""))
    cmd += [os.path.join(ROOT, "tests", "host", "ivf_format_main.cpp"), os.path.join(CSRC, "error.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(prog, *args):
    return subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.mark.parametrize("n,nlist,seed", [(64, 4, 1234), (600, 15, 1), (2400, 60, 5), (20000, 8192, 5), (48, 48, 5), (7, 1, 2 ** 64 - 1)])
def test_seed_rows_equal_the_header(prog, n, nlist, seed):
    r = run(prog, "seeds", n, nlist, seed)
    assert r.returncode == 0, r.stdout
    assert [int(v) for v in r.stdout.split()] == bo.seed_rows(n, nlist, seed)


@pytest.mark.parametrize("name", list(bc.CRAFTED))
def test_host_update_equals_the_oracle_on_crafted_relocations(prog, tmp_path, name):
    x, assign, prev, nlist, must = bc.crafted(name)
    want, rep = bo.update(x, prev, assign, relocating=True)
    # the input reaches what it was made for, with margins the host's own summation order cannot cross
    got_facts = dict(splits=rep["splits"], moves=[j for j, _ in rep["moves"]], skip_used=rep["skip_used"], skip_moved=rep["skip_moved"],
                     cursor_diff=rep["cursor_diff"], brk=rep["brk"])
    assert {k: got_facts[k] for k in must} == must
    assert rep["nn_ties_unequal"] == 0 and min(bo.margins(rep).values()) >= bo.MARGIN, bo.margins(rep)
    assert rep["maxmoves"] == max(1, nlist // 20) and (rep["brk"] != "cap" or len(rep["moves"]) == rep["maxmoves"])
    src, out = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(struct.pack("<qqq", x.shape[0], x.shape[1], nlist) + x.tobytes() + assign.tobytes() + prev.tobytes())
    r = run(prog, "steps", src, out)
    assert r.returncode == 0 and "steps ok" in r.stdout, r.stdout
    buf = out.read_bytes()
    cent = np.frombuffer(buf, np.float32, nlist * 4).reshape(nlist, 4)
    (nm,) = struct.unpack_from("<q", buf, nlist * 16)
    moves = np.frombuffer(buf, np.int64, 2 * nm, nlist * 16 + 8).reshape(-1, 2)
    assert len(buf) == nlist * 16 + 8 + 16 * nm
    assert [tuple(m) for m in moves.tolist()] == rep["moves"]
    assert np.array_equal(bits(cent), bits(want))
    for j, row in rep["moves"]:
        assert np.array_equal(bits(cent[j]), bits(x[row]))
