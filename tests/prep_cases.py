"""The cases of tests/golden/prep_filtfilt.npz (tools/make_golden_prep.py) for the CPU and the GPU tests of the device input
preparation: seeded inputs regenerated from their recipes, and the exact (long-double) filter result at the fixture's positions."""
import os
import sys
import types

import numpy as np

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_prep import CASES, CUT_GEOMETRY, make_input, positions, sha  # noqa: E402,F401

_D = None


def golden():
    global _D
    if _D is None:
        _D = load_golden("prep_filtfilt")
    return _D


def names():
    return [str(n) for n in golden()["names"]]


def long_names():
    return [n for n in names() if CASES[n][1] > CUT_GEOMETRY[3]]


def load(name):
    """-> x (the case's dtype), idx (compared positions), exact (float64 at idx), b, a, cuts (long cases: the host loop's cuts on the
    scipy-filtered signal when the fixture was made, else None)."""
    d = golden()
    x = make_input(name)
    # a recipe that no longer regenerates the fixture's input is a failure of the test, not a reason to skip it
    assert sha(x) == str(d[name + "_input_sha256"]), "%s: the input does not have the sha256 the fixture was made with" % name
    idx = positions(x.shape[0])
    exact = d[name + "_exact"]
    assert exact.dtype == np.float64 and exact.shape == idx.shape
    cuts = [int(t) for t in d[name + "_cuts"]] if name + "_cuts" in d else None
    return types.SimpleNamespace(name=name, x=x, idx=idx, exact=exact, b=d["b"], a=d["a"], cuts=cuts)
