"""The bank's formant shift per session, the parts that need no GPU: the block geometry of a shift against the
reference's expressions, the two new C entry points in the header / library / binding, and the host part of the ragged resampler."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import rt_formant_cases as fc
from conftest import ROOT


def test_formant_geometry_is_the_reference_expression_over_the_whole_slider():
    """(factor, return_length2, upp_res) for every slider value, model rate and block length the GUI can produce; the three expressions of
    infer/lib/rtrvc.py:190-191, 248 written out here."""
    import rvc_amd

    assert len(fc.SLIDER) == 81 and fc.SLIDER[0] == -2.0 and fc.SLIDER[-1] == 2.0 and 0.0 in fc.SLIDER
    distinct = {}
    for sr in fc.RATES:
        for rl in fc.RETURN_LENGTHS:
            for shift in fc.SLIDER:
                factor = pow(2, shift / 12)
                return_length2 = int(np.ceil(rl * factor))
                upp_res = int(np.floor(factor * sr // 100))
                got = rvc_amd.formant_geometry(shift, rl, sr)
                assert got == (factor, return_length2, upp_res), (sr, rl, shift, got)
                assert all(type(v) is t for v, t in zip(got, (float, int, int)))
                assert rl * upp_res <= return_length2 * (sr // 100)   # the resampler's input lies inside the decoded block
                distinct.setdefault(sr, set()).add(upp_res)
    assert rvc_amd.formant_geometry(0.0, 20, 48000) == (1.0, 20, 480)
    assert all(len(v) <= 81 for v in distinct.values())
    assert fc.geometry(fc.FORMANTS[0]) == (23, 538) and fc.geometry(fc.FORMANTS[1]) == (20, 480) and fc.geometry(fc.FORMANTS[2]) == (19, 443)


def test_the_unresampled_edge_at_32k():
    """+0.05 at 32 kHz: a longer decode that the reference does not resample; nowhere else on the slider grid, at no rate."""
    import rvc_amd

    for rl in fc.RETURN_LENGTHS:
        _, rl2, upp_res = rvc_amd.formant_geometry(0.05, rl, 32000)
        assert upp_res == 320 and rl2 == rl + 1
    edges = {(sr, shift) for sr in fc.RATES for rl in fc.RETURN_LENGTHS for shift in fc.SLIDER
             if shift != 0 and rvc_amd.formant_geometry(shift, rl, sr)[2] == sr // 100}
    assert edges == {(32000, 0.05)}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rvcmi.h")).read(), flags=re.S)


def test_the_new_entry_points_are_declared_exported_and_bound():
    from rvc_amd import _lib

    src = _header()
    lib = C.CDLL(_lib.LIB_PATH)
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for name, nargs in (("rvcmi_nsf_forward_nres", 11), ("rvcmi_glue_resample_poly_ragged", 11)):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m, "%s is not declared in include/rvcmi.h" % name
        assert len(m.group(1).split(",")) == nargs
        assert hasattr(lib, name), "librvcmi.so does not export %s" % name
        assert name in bound and bound[name][1] is C.c_int and len(bound[name][2]) == nargs
    assert _lib.lib().rvcmi_version() == _lib.RVCMI_VERSION == 2
    # the descriptor struct, field for field
    body = re.search(r"typedef struct \{([^}]*)\} rvcmi_resample_row;", src).group(1)
    fields = [n.strip() for d in body.split(";") if d.strip() for n in d.strip().split(None, 1)[1].split(",")]
    assert fields == [n for n, _ in _lib.ResampleRow._fields_]
    assert C.sizeof(_lib.ResampleRow) == 8 + 8 + 4 * 4
    assert _lib.ERR_INVALID == -1 and _lib.ERR_NOMEM == -4


def test_ragged_resampler_plan_on_the_host():
    """Equal rates share one table, an un-resampled row has none, the tables tile the concatenated buffer in order, a changed tuple
    rebuilds and an unchanged one does not; every descriptor holds what ``SincResample`` would pass for that row."""
    import rvc_amd

    rs = rvc_amd.SincResampleRagged(480)
    assert rs.plan((538, 480, 444, 538), 20) is True and rs.rebuilds == 1
    assert rs.plan([538, 480, 444, 538], 20) is False and rs.rebuilds == 1
    tabs = {o: rvc_amd.sinc_resample_kernel(o, 480) for o in (538, 444)}
    assert sorted(rs.offsets) == [444, 538]
    assert rs.offsets[538] == 0 and rs.offsets[444] == tabs[538][0].numel()
    assert rs.table_floats == sum(t[0].numel() for t in tabs.values())
    assert rs.rows[0] == rs.rows[3]                                   # equal shifts: one table, the same descriptor
    for r, o in zip(rs.rows, (538, 480, 444, 538)):
        assert r["n"] == 20 * o
        if o == 480:
            assert r["orig"] == r["new"]                              # copied, not resampled
            continue
        k, width, of, nf = tabs[o]
        assert (r["w_off"], r["orig"], r["new"], r["K"], r["width"]) == (rs.offsets[o], of, nf, k.shape[1], width)
        assert r["K"] == 2 * width + of and r["w_off"] + nf * r["K"] <= rs.table_floats
    # offsets tile the buffer: sorted by offset, each table ends where the next one starts
    order = sorted(rs.offsets, key=rs.offsets.get)
    ends = [rs.offsets[o] + tabs[o][0].numel() for o in order]
    assert [rs.offsets[o] for o in order[1:]] + [rs.table_floats] == ends
    assert rs.plan((538, 480, 466, 538), 20) is True and rs.rebuilds == 2 and sorted(rs.offsets) == [466, 538]
    assert rs.plan((538, 480, 466, 538), 60) is True and rs.rebuilds == 3 and rs.rows[0]["n"] == 60 * 538
    assert rs.plan((480, 480), 20) is True and rs.table_floats == 0 and not rs.offsets
    with pytest.raises(ValueError):
        rs.plan((), 20)
    with pytest.raises(ValueError):
        rs.plan((0, 480), 20)


def test_table_sizes_over_the_slider():
    """What a bank may have to keep: K <= 543 taps; the largest table per rate."""
    import rvc_amd

    want = {48000: 260640, 40000: 184400, 32000: 119360}
    for sr in fc.RATES:
        new = sr // 100
        sizes, Ks = [], []
        for shift in fc.SLIDER:
            upp_res = rvc_amd.formant_geometry(shift, 20, sr)[2]
            if upp_res != new:
                k = rvc_amd.sinc_resample_kernel(upp_res, new)[0]
                sizes.append(int(k.numel()))
                Ks.append(int(k.shape[1]))
        assert max(Ks) <= 543 and max(sizes) == want[sr], (sr, max(Ks), max(sizes))


def test_per_session_formant_state_needs_no_device():
    """The host state of the two objects: lists of S values, bounds-checked setters, the bank-wide forms still refused."""
    import rvc_amd

    net = type("N", (), {})()
    vc = rvc_amd.RealtimeVCBatch(net, 3, device="cpu")
    assert vc.formants == [0.0, 0.0, 0.0]
    vc.set_session_formant(1, -1.35)
    assert vc.formants == [0.0, -1.35, 0.0]
    for bad in (3, -1):
        with pytest.raises(IndexError):
            vc.set_session_formant(bad, 1.0)
    with pytest.raises(ValueError):
        vc.set_session_formant(0, float("nan"))
    with pytest.raises(ValueError, match="formant"):
        vc.set_formant(1.0)
    vc.set_formant(0)
    with pytest.raises(ValueError, match="set_session_formant"):
        rvc_amd.RealtimeVCBatch(net, 3, device="cpu", formant_shift=0.5)
