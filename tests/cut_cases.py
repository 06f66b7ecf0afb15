"""The cases of tests/golden/cut_points.npz (tools/make_golden_cuts.py) for the CPU and the GPU tests of the quiet-point search."""
import os
import sys
import types

import numpy as np

from conftest import ROOT, load_golden

sys.path.insert(0, os.path.join(ROOT, "tools"))
from make_golden_cuts import long_input, periodic_input, sha  # noqa: E402

_D = None


def golden():
    global _D
    if _D is None:
        _D = load_golden("cut_points")
    return _D


def names():
    return [str(n) for n in golden()["names"]]


class Case(types.SimpleNamespace):
    """window, t_center, t_query, t_max, n, audio (float64), opt_ts (list of int), sums (flat float64 or None), sums_sha256."""

    def state(self):
        """What ``_cut_points`` reads of a ``Pipeline``."""
        return types.SimpleNamespace(window=self.window, t_center=self.t_center, t_query=self.t_query, t_max=self.t_max)

    def searched(self):
        """pipeline.py:224: the search runs at all."""
        return self.n + 2 * (self.window // 2) > self.t_max

    def lengths(self):
        """Samples of every cut's search window that lie inside the signal."""
        return [min(t + self.t_query, self.n) - (t - self.t_query) for t in range(self.t_center, self.n, self.t_center)]


def load(name):
    d = golden()
    p = name + "_"
    window, t_center, t_query, t_max, n = (int(v) for v in d[p + "geom"])
    kind, seed = str(d[p + "kind"]), int(d[p + "seed"])
    audio = d[p + "audio"] if kind == "stored" else (long_input if kind == "long" else periodic_input)(seed, n)
    # a recipe that no longer regenerates the fixture's input is a failure of the test, not a reason to skip it
    assert audio.dtype == np.float64 and audio.shape == (n,) and sha(audio) == str(d[p + "input_sha256"]), \
        "%s: the input does not have the sha256 the fixture was made with" % name
    return Case(name=name, window=window, t_center=t_center, t_query=t_query, t_max=t_max, n=n, audio=audio,
                opt_ts=[int(t) for t in d[p + "opt_ts"]], sums=d.get(p + "sums"), sums_sha256=str(d[p + "sums_sha256"]))
