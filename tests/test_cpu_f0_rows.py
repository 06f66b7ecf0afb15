"""The descriptor validation of ``rvcmi_glue_rmvpe_f0_ragged`` (csrc/f0_rows.hpp, host only) driven by a stand-alone C++ program
(tests/host/f0_rows_main.cpp, built here with -fsanitize=address,undefined; nothing of it is loaded into Python), and the layout of the
ctypes mirror of ``rvcmi_f0_row``.  No GPU."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_descriptor_validation_stand_alone(tmp_path):
    exe = str(tmp_path / "f0_rows_main")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "f0_rows_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("f0 rows ok"), r.stdout
    assert "FAILED" not in r.stdout and r.stdout.count(" ok") >= 21


def test_ctypes_descriptor_layout():
    from rvc_amd import _lib

    assert C.sizeof(_lib.F0Row) == 32 and C.alignment(_lib.F0Row) == 8
    assert [(n, getattr(_lib.F0Row, n).offset) for n, _ in _lib.F0Row._fields_] == [("out_off", 0), ("key_mul", 8), ("first_row", 16), ("n", 20),
                                                                                    ("p_len", 24), ("reserved_", 28)]
