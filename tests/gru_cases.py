"""Shared pieces of the GRU tests (tests/test_cpu_gru.py, tests/test_gpu_gru.py) and of tools/gru_parity.py: the seeded cases, their fp64
oracle (oracle/gru_oracle.py with the kernel's fp16 operand rounding) and the bars csrc/gru.hip is held to against it.

The bars are derived, not measured on the kernel.  ``floor`` = the oracle's own recurrence evaluated in float32 against its float64 evaluation:
fp32 rounding that now and then flips the fp16 rounding of h.  The kernel differs from that fp32 evaluation in summation order and in its gate
approximations (v_rcp_f32, 1 ulp; the fast exp); perturbing exp by +-2 ulp and rcp by +-1 ulp at random moved the floor by at most 1.5x, and the
factors are twice that: ``bar_rms = 3 * floor_rms + 1e-6``, ``bar_max = 4 * floor_max + 4e-6``.  The additive terms allow for the 1-ulp rcp and
the fast exp on gate values in (-1, 1), about 32 fp32 ulps of 1; they decide T <= 3, where no flip has happened yet.
tests/test_cpu_gru.py asserts that the named wrong recurrences of the oracle stand clear of these bars, so widening them fails there.
"""
import collections
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import gru_oracle  # noqa: E402

Case = collections.namedtuple("Case", "B T I seed gain xscale", defaults=(384, 0, 1.0, 1.0))

# what test_gru_hip_matches_torch_fp32 has always run (same seeds, same weights and inputs)
EXISTING = tuple(Case(B, T, 384, seed, gain) for B, T, seed, gain in ((1, 1, 0, 1.0), (2, 7, 1, 1.0), (1, 1216, 2, 1.0), (3, 301, 3, 2.5), (64, 40, 4, 1.0)))
# input sizes whose K loop (16 per trip, unrolled by 8) makes 1, 3 and 25 trips
INPUT_SIZES = (Case(2, 33, 16, 11), Case(4, 100, 48, 12), Case(1, 50, 400, 13))
# |pre-activation| well past 88.7, where fp32 exp overflows: the gates must land on their limits
SATURATED = Case(2, 64, 384, 19, 1.0, 40.0)
# the table of the GPU test: T = 1, 2, 3 (the request two steps ahead, its clamp to T - 1, the odd tail), M = 32 and 33 rows (the
# projection's 32-row tile: clamped loads and the early return), the K-loop trip counts, long sequences, saturation
TABLE = (Case(1, 1, 384, 5), Case(1, 2, 384, 6), Case(1, 3, 384, 7), Case(2, 7, 384, 8), Case(32, 1, 384, 9), Case(11, 3, 384, 10)) + INPUT_SIZES + (
    Case(3, 301, 384, 14), Case(1, 1216, 384, 15), SATURATED)
RAGGED_ROWS = (1, 2, 33, 7, 64, 3)  # lengths that are no multiple of 32 (the f0 batch only ever sends multiples)


def case_id(c):
    return "B%d-T%d-I%d-seed%d%s%s" % (c.B, c.T, c.I, c.seed, "" if c.gain == 1.0 else "-gain%g" % c.gain, "" if c.xscale == 1.0 else "-x%g" % c.xscale)


def module(c):
    """torch's own layer with its default initialisation, seeded (times ``gain``)."""
    torch.manual_seed(c.seed)
    ref = torch.nn.GRU(c.I, 256, num_layers=1, batch_first=True, bidirectional=True).eval()
    if c.gain != 1.0:
        with torch.no_grad():
            for p in ref.parameters():
                p.mul_(c.gain)
    return ref


def weights(gru):
    """-> (w_ih, w_hh, b_ih, b_hh) stacked [2, ...] forward / reverse as ``GRUHIP.__init__`` stacks them, float64"""
    def both(name):
        return torch.stack([getattr(gru, name + "_l0").detach(), getattr(gru, name + "_l0_reverse").detach()]).double().numpy()

    return both("weight_ih"), both("weight_hh"), both("bias_ih"), both("bias_hh")


def inputs(c):
    """-> x [B, T, I] float32"""
    return c.xscale * torch.randn(c.B, c.T, c.I, generator=torch.Generator().manual_seed(100 + c.seed))


def err(got, want):
    """-> (RMS, max-abs) of got - want, in float64"""
    e = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    return float(np.sqrt(np.mean(e * e))), float(np.abs(e).max())


def bars_of(y32, y64):
    floor_rms, floor_max = err(y32, y64)
    return {"floor_rms": floor_rms, "floor_max": floor_max, "bar_rms": 3 * floor_rms + 1e-6, "bar_max": 4 * floor_max + 4e-6}


@functools.lru_cache(maxsize=None)
def bars(c):
    """The oracle of a case (``y``, ``hn``: float64, fp16 operands; computed once, never changed) and the bars against it."""
    w, x = weights(module(c)), inputs(c).numpy()
    y64, hn64 = gru_oracle.bigru(*w, x)
    y32, _ = gru_oracle.bigru(*w, x, arith="f32")
    out = {"y": y64, "hn": hn64, **bars_of(y32, y64)}
    y64.setflags(write=False)
    hn64.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ragged_case(seed=16):
    """-> (module, x_rows [M, 384] float32, offsets): RAGGED_ROWS packed"""
    c = Case(1, sum(RAGGED_ROWS), 384, seed)
    off = [0]
    for r in RAGGED_ROWS:
        off.append(off[-1] + r)
    return module(c), inputs(c)[0], off


@functools.lru_cache(maxsize=None)
def ragged_bars(seed=16):
    """Per sequence of ``ragged_case``: the oracle of that sequence alone and its bars."""
    gru, x, off = ragged_case(seed)
    w = weights(gru)
    y64, hn64 = gru_oracle.ragged(*w, x.numpy(), off)
    y32, _ = gru_oracle.ragged(*w, x.numpy(), off, arith="f32")
    return [{"y": y64[a:b], "hn": hn64[:, i], **bars_of(y32[a:b], y64[a:b])} for i, (a, b) in enumerate(zip(off[:-1], off[1:]))]
