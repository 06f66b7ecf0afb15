"""The checker of csrc/gru.hip checked (no GPU): oracle/gru_oracle.py is torch's ``nn.GRU``, and the bars tests/gru_cases.py derives from it
are sharp enough to tell the kernel's documented design from the recurrences that look like it.

  * With the operand rounding off, the fp64 oracle is ``torch.nn.GRU`` in fp32 on the CPU to 1e-5 max-abs (measured 2e-7 .. 2.2e-6, the worst at
    gain 2.5, T = 301): the five cases tests/test_gpu_gru.py has always run plus input sizes 16, 48 and 400.
  * The bars separate: for every gain-1 case with T >= 7 the named wrong recurrences of the oracle differ from it by at least 2x the RMS bar
    (the state through its fp16 copy, GX as fp16, h truncated: measured >= 2.6x) or 10x (b_hn outside r * (...), b_hh missing from r and z, the
    last step on the previous step's GX: measured >= 400x).  Whoever widens the factors of ``gru_cases.bars`` fails here.
  * The saturated case (x * 40: pre-activations past fp32 exp's overflow at 88.7) is finite in both arithmetics.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import gru_cases as gc  # noqa: E402
from oracle import gru_oracle  # noqa: E402


@pytest.mark.parametrize("c", gc.EXISTING + gc.INPUT_SIZES, ids=gc.case_id)
def test_the_oracle_is_torchs_gru(c):
    ref = gc.module(c)
    x = gc.inputs(c)
    with torch.no_grad():
        y_ref, hn_ref = ref(x)
    y, hn = gru_oracle.bigru(*gc.weights(ref), x.numpy(), round_operands=False)
    assert y.shape == tuple(y_ref.shape) and hn.shape == tuple(hn_ref.shape)
    ey, eh = gc.err(y, y_ref.numpy())[1], gc.err(hn, hn_ref.numpy())[1]
    print("%s: oracle (exact operands) vs nn.GRU fp32: y %.2e h_n %.2e max-abs" % (gc.case_id(c), ey, eh))
    assert ey <= 1e-5 and eh <= 1e-5


SEPARATION = tuple(c for c in dict.fromkeys(gc.EXISTING + gc.TABLE) if c.gain == 1.0 and c.T >= 7)


@pytest.mark.parametrize("c", SEPARATION, ids=gc.case_id)
def test_the_bars_separate_the_design_from_its_lookalikes(c):
    b = gc.bars(c)
    assert b["bar_rms"] == 3 * b["floor_rms"] + 1e-6 and b["bar_max"] == 4 * b["floor_max"] + 4e-6
    w, x = gc.weights(gc.module(c)), gc.inputs(c).numpy()
    for variant, factor in (("state_fp16", 2), ("gx_fp16", 2), ("h_trunc", 2), ("bhn_outside", 10), ("no_bhh_rz", 10), ("tail_gx", 10)):
        y, _ = gru_oracle.bigru(*w, x, variant=variant)
        rms = gc.err(y, b["y"])[0]
        print("%s %s: %.2e RMS = %.1f x bar_rms (floor %.2e)" % (gc.case_id(c), variant, rms, rms / b["bar_rms"], b["floor_rms"]))
        assert rms >= factor * b["bar_rms"], "%s is only %.2f x the RMS bar of %s" % (variant, rms / b["bar_rms"], gc.case_id(c))


def test_the_saturated_case_overflows_exp_and_stays_finite():
    c = gc.SATURATED
    w_ih, w_hh, b_ih, b_hh = gc.weights(gc.module(c))
    x = gc.inputs(c).numpy().astype(np.float64)
    assert np.abs(x @ w_ih[0].T).max() > 100.0  # (fp32 exp overflows past 88.7; the n gate's exp(-2v) past 44.4)
    for arith in ("f64", "f32"):
        y, hn = gru_oracle.bigru(w_ih, w_hh, b_ih, b_hh, x, arith=arith)
        assert np.isfinite(y).all() and np.isfinite(hn).all() and np.abs(y).max() <= 1.0, arith
    b = gc.bars(c)
    assert np.isfinite([b["floor_rms"], b["floor_max"]]).all()
