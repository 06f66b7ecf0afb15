"""Every header of csrc/ includes what it uses: each one is given to hipcc on its own (gfx950, -fsyntax-only) and must compile.
Nothing in the compiler's output is inspected; the test is skipped where there is no hipcc."""
import glob
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "retrieval-based-voice-conversion-webui_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HIPCC = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp")))


@pytest.mark.skipif(HIPCC is None, reason="no hipcc")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_on_its_own(header):
    cmd = [HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-x", "hip", os.path.join(CSRC, header)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
