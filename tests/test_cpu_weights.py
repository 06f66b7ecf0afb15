"""csrc/weights.hpp -- the named-weight table every create call reads and the 256-byte offset planner of the workspaces -- driven by a
stand-alone C++ program (tests/host/weights_main.cpp, built here with -fsanitize=address,undefined together with csrc/error.cpp; nothing of
it is loaded into Python)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "retrieval-based-voice-conversion-webui_amd", "csrc")


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("weights") / "weights_main")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "weights_main.cpp"), os.path.join(CSRC, "error.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("weights ok"), r.stdout
    return r.stdout


@pytest.mark.parametrize("case, code, text", [
    ("missing", -5, "missing weight tensor 'c.weight'"),
    ("wrong rank", -1, "a.weight"),
    ("rank 5 asked for", -1, "a.weight"),
    ("rank 5 supplied", -1, "r5"),
    ("wrong extent", -1, "dim 1 is 3, expected 4"),
    ("null data", -1, "no data"),
    ("null name", -1, "tensor 1 has no name"),
    ("one left over", -1, "3 tensors were supplied, the recognised thing has 1"),
])
def test_refusals_carry_the_code_and_name_the_tensor(out, case, code, text):
    line = [l for l in out.splitlines() if l.startswith("ok %s: " % case)]
    assert len(line) == 1 and line[0].startswith("ok %s: %d " % (case, code)) and text in line[0], out


@pytest.mark.parametrize("case", ["found", "duplicate: the last wins", "a refused tensor does not count as used", "asking twice counts once", "carve"])
def test_lookups_and_offsets(out, case):
    assert "ok %s\n" % case in out, out


def test_the_header_is_host_only():
    """No HIP include: weights.hpp, like ivf_format.hpp, builds with a plain C++ compiler (the fixture above is the proof; this names why)."""
    src = open(os.path.join(CSRC, "weights.hpp")).read()
    assert "hip/" not in src and '#include "common.hpp"' not in src
