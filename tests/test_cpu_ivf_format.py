"""The two formats of the IVF index (csrc/ivf_format.hpp: faiss' IwFl file, the device blob) and the host steps of k-means
(csrc/ivf_kmeans.hpp) on the CPU: tests/host/ivf_format_main.cpp is built with g++ and run as a child process.  Nothing is loaded
into Python.  ``RVCMI_HOST_TEST_CXXFLAGS`` adds compiler flags (default none) -- e.g. ``-O0 -g -fsanitize=address,undefined
-fno-sanitize-recover=all`` makes the same program a sanitizer run of the reader over every case here."""
import os
import shlex
import subprocess

import numpy as np
import pytest

import ivf_cases
from oracle import ivf_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "retrieval-based-voice-conversion-webui_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ivf_format") / "ivf_format_main")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + shlex.split(os.environ.get("RVCMI_HOST_TEST_CXXFLAGS", ""))
    cmd += [os.path.join(ROOT, "tests", "host", "ivf_format_main.cpp"), os.path.join(CSRC, "error.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def run(prog, *args):
    return subprocess.run([prog] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


@pytest.mark.parametrize("sparse", [False, True], ids=["full", "sprs"])
@pytest.mark.parametrize("n,d,nlist,empty", [(40, 8, 5, (2,)), (0, 8, 5, ()), (3000, 64, 37, ())], ids=["n40", "n0", "n3000"])
def test_file_to_blob_to_file_keeps_every_array(prog, tmp_path, n, d, nlist, empty, sparse):
    idx = ivf_cases.make_index(n, d, nlist, empty=empty, seed=n + 1)
    if empty:
        assert all(idx["list_offsets"][l + 1] == idx["list_offsets"][l] for l in empty)
    src, out = tmp_path / "in.index", tmp_path / "out.index"
    ivf_oracle.write_index(idx, str(src), sparse=sparse)
    r = run(prog, "roundtrip", src, out)  # parse, build_blob, write, parse again: the program compares its two parses
    assert r.returncode == 0 and "roundtrip ok" in r.stdout, r.stdout
    got = ivf_oracle.read_index(str(out))
    for k in ("d", "ntotal", "nlist", "nprobe"):
        assert got[k] == idx[k], k
    for k in ("centroids", "list_offsets", "ids", "vecs"):
        assert np.array_equal(got[k], idx[k]), k


def test_every_proper_prefix_is_refused_as_truncated(prog, tmp_path):
    idx = ivf_cases.make_index(40, 8, 5, empty=(2,), seed=41)
    src = tmp_path / "in.index"
    ivf_oracle.write_index(idx, str(src))
    r = run(prog, "prefixes", src, tmp_path / "prefix.index")
    assert r.returncode == 0 and "prefixes ok: %d refused" % os.path.getsize(src) in r.stdout, r.stdout


@pytest.mark.parametrize("name", sorted(ivf_cases.CRAFTED))
def test_a_file_whose_counts_lie_is_refused_with_err_io(prog, tmp_path, name):
    p = tmp_path / (name + ".index")
    p.write_bytes(ivf_cases.crafted(**ivf_cases.CRAFTED[name]))
    r = run(prog, "reject", p)
    assert r.returncode == 0 and r.stdout.startswith("rc=-3 "), (r.returncode, r.stdout)  # a normal exit, RVCMI_ERR_IO


def test_crafted_builder_writes_a_file_the_reader_takes_when_the_counts_are_true(prog, tmp_path):
    """The crafted files differ from this one only in the field under test: they are not refused for some other reason."""
    p = tmp_path / "true.index"
    p.write_bytes(ivf_cases.crafted(words=(3, 0), payload=3 * (4 * 4 + 8)))
    r = run(prog, "reject", p)
    assert r.returncode == 1 and r.stdout.startswith("rc=0 "), (r.returncode, r.stdout)


def test_kmeans_host_steps(prog):
    r = run(prog, "kmeans")
    assert r.returncode == 0 and "kmeans ok" in r.stdout, r.stdout
