"""The per-session sliders of the realtime bank, host side: the setters' validation (``SessionSliders``), the active-session
plans of the three ``glue.*_sessions`` wrappers as pure functions, the gate cutoffs per session, the C declarations, and the host-only
validation of the new entry points (csrc/session_rows.hpp) driven by a stand-alone C++ program built here with
-fsanitize=address,undefined (tests/host/session_rows_main.cpp; nothing of it is loaded into Python).  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import input_gate_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rvcmi_ivf_search_blend_expand_sessions", "rvcmi_glue_envelope_mix_sessions", "rvcmi_glue_input_gate_sessions")


def test_host_validation_stand_alone(tmp_path):
    exe = str(tmp_path / "session_rows_main")
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "host", "session_rows_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("session rows ok"), r.stdout
    assert "FAILED" not in r.stdout and r.stdout.count(" ok") >= 39


def test_setters_validate_and_sessions_follow_the_bank_until_set():
    from rvc_amd import SessionSliders

    sl = SessionSliders(3)
    assert set(sl.own) == {"index_rate", "protect", "rms_mix_rate", "threhold"}
    for name, bank in (("index_rate", 0.75), ("protect", 1.0), ("rms_mix_rate", 0.0), ("threhold", -60)):
        assert sl.values(name, bank) == [bank] * 3 and not sl.differs(name, bank)
        for bad_i in (-1, 3, 17):
            with pytest.raises(IndexError):
                sl.set(name, bad_i, 0.5)
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError):
                sl.set(name, 1, bad)
        assert sl.values(name, bank) == [bank] * 3          # a refused call changes nothing
        sl.set(name, 1, bank)                               # explicitly the bank-wide value: still the bank-wide path
        assert sl.values(name, bank) == [bank] * 3 and not sl.differs(name, bank)
        sl.set(name, 2, 0.25)
        assert sl.values(name, bank) == [bank, bank, 0.25] and sl.differs(name, bank)
        assert sl.values(name, 0.25) == [0.25, bank, 0.25] and sl.differs(name, 0.25)   # session 0 follows a bank-wide value that moves; 1 keeps its own
        sl.set(name, 2, None)
        sl.set(name, 1, None)
        assert sl.own[name] == [None] * 3 and not sl.differs(name, bank)
    assert isinstance(SessionSliders(2, ("protect",)).values("protect", 0.33)[0], float)


def test_bank_classes_carry_the_setters():
    """The setters exist on the classes and go through ``SessionSliders`` (constructing a bank needs a GPU: tests/test_gpu_rt_bank_sliders.py)."""
    import inspect

    import rvc_amd

    for name in ("set_index_rate", "set_protect", "set_rms_mix_rate", "set_threhold"):
        assert list(inspect.signature(getattr(rvc_amd.RealtimeBank, name)).parameters)[:2] == ["self", "i"]
    for name in ("set_session_index_rate", "set_session_protect"):
        assert callable(getattr(rvc_amd.RealtimeVCBatch, name))
    for fn in (rvc_amd.RealtimeVCBatch.infer, rvc_amd.realtime.rvc_infer_batch_hip):
        p = inspect.signature(fn).parameters
        assert p["index_rates"].default is None and p["protects"].default is None


def test_active_session_plans():
    from rvc_amd import glue

    # retrieval: who blends, the packed slot of each, whose protect mix applies
    plan = glue.session_blend_plan([0.75, 0.0, 0.3], [0.33, 1.0, 0.49], True, True)
    assert plan == [(0.75, 0.33, 0, 1), (0.0, 1.0, -1, 0), (0.3, 0.49, 1, 1)]
    assert glue.session_blend_plan([0.75, 0.0, 0.3], [0.33, 1.0, 0.49], False, True) == [(0.0, 0.33, -1, 1), (0.0, 1.0, -1, 0), (0.0, 0.49, -1, 1)]
    assert glue.session_blend_plan([0.75, 0.0, 0.3], [0.33, 1.0, 0.49], True, False) == [(0.75, 1.0, 0, 0), (0.0, 1.0, -1, 0), (0.3, 1.0, 1, 0)]
    assert [r[2] for r in glue.session_blend_plan([0, 0, 0.5, 0, 0.5, 0.5], [1.0] * 6, True, True)] == [-1, -1, 0, -1, 1, 2]
    assert [r[2] for r in glue.session_blend_plan([0, 0, 0], [0.2] * 3, True, True)] == [-1, -1, -1]
    assert glue.session_blend_plan([0.5], [0.5], True, True) == [(0.5, 1.0, 0, 0)]   # protect mixes below 0.5 only (pipeline.py:153)
    for bad in (([float("nan")], [1.0]), ([0.5], [float("inf")]), ([0.5, 0.5], [1.0]), ([], [])):
        with pytest.raises(ValueError):
            glue.session_blend_plan(bad[0], bad[1], True, True)
    # envelope mix: the exponent is float32(1 - rate) rounded once from the double difference; on iff rate < 1
    plan = glue.session_mix_plan([0.0, 0.5, 1.0, 0.3, 1.5])
    assert [r[1] for r in plan] == [1, 1, 0, 1, 0]
    assert [np.float32(r[0]) for r in plan] == [np.float32(1.0 - r) for r in (0.0, 0.5, 1.0, 0.3, 1.5)]
    assert plan[3][0] == float(np.float32(1.0 - 0.3)) != 1.0 - 0.3
    with pytest.raises(ValueError):
        glue.session_mix_plan([0.5, float("nan")])
    # gate: on iff threhold > -60
    plan = glue.session_gate_plan([-40.5, -20, -60, -55, -60.01])
    assert [r[2] for r in plan] == [1, 1, 0, 1, 0] and plan[2][:2] == (0.0, 0.0)
    with pytest.raises(ValueError):
        glue.session_gate_plan([-40, float("nan")])


def test_gate_cutoffs_per_session():
    """Each session's cutoffs are those of ``input_gate_cutoffs`` at ITS threshold, and they decide as the host gate does at that threshold."""
    from rvc_amd import glue
    from rvc_amd.realtime import amplitude_to_db, input_gate_cutoffs

    plan = glue.session_gate_plan(gc.CUTOFF_THRESHOLDS)
    assert len({p[:2] for p in plan}) == len(gc.CUTOFF_THRESHOLDS)          # distinct thresholds, distinct cutoffs
    for t, (cut_a, cut_b, on) in zip(gc.CUTOFF_THRESHOLDS, plan):
        assert on == 1 and (cut_a, cut_b) == input_gate_cutoffs(t)
        assert np.float32(cut_a) == cut_a and np.float32(cut_b) == cut_b     # exact float32 values
        a = np.float32(cut_a)
        below = np.nextafter(a, np.float32(0))
        assert not bool((amplitude_to_db(np.array([a], np.float32)) < t)[0]) and bool((amplitude_to_db(np.array([below], np.float32)) < t)[0])
    a = [p[0] for p in plan]
    assert a == sorted(a)   # a higher threshold gates more


def test_new_entry_points_are_declared_bound_and_exported():
    from rvc_amd import _lib

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rvcmi.h")).read(), flags=re.S)
    bound = {s[0]: s for s in _lib.SYMBOLS}
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, "%s is not declared in include/rvcmi.h" % name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == len(m.group(1).split(","))
        assert hasattr(lib, name), "librvcmi.so does not export %s" % name
        assert "sess_host" in m.group(1) and "sess_dev" in m.group(1)       # the values are given twice
    # the ctypes mirrors of the three descriptors
    for struct, cname, size in ((_lib.SessionBlend, "rvcmi_session_blend", 16), (_lib.SessionMix, "rvcmi_session_mix", 8),
                                (_lib.SessionGate, "rvcmi_session_gate", 16)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % cname, hdr).group(1)
        names = [n.strip() for d in body.split(";") if d.strip() for n in d.strip().split(" ", 1)[1].split(",")]
        assert names == [n for n, _ in struct._fields_] and C.sizeof(struct) == size and C.alignment(struct) == 4
