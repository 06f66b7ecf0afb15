"""Inputs and the numpy statement of the device rule for the input gate tests (tests/test_cpu_input_gate.py, tests/test_gpu_input_gate.py).
Seeded, no GPU.  The oracle is ``rvc_amd.realtime.input_gate`` itself, per session."""
import numpy as np

GEOMETRIES = ((160, 1280), (441, 2205), (480, 1440))     # (zc, blk): the CPU comparison
CUTOFF_THRESHOLDS = (-59.95, -55, -40.5, -20, -0.05, 0)


def device_rule(block, rms_buffer, zc, cut_a, cut_b):
    """What rvcmi_glue_input_gate_batch computes for one session, in numpy: -> (out [blk + 2 zc], new rms_buffer [4 zc]).  No logarithm: the
    two float32 cutoffs decide."""
    from rvc_amd.realtime import frame_rms_np

    x = np.append(np.asarray(rms_buffer, np.float32), np.asarray(block, np.float32))
    blk = len(block)
    rms = frame_rms_np(x, 4 * zc, zc)[2:]
    assert len(rms) == blk // zc + 3
    has_nan = bool(np.isnan(rms).any())
    mx = np.float32(0) if has_nan else rms.max()
    quiet = np.zeros(len(rms), bool) if has_nan or not (mx < np.float32(cut_b)) else rms < np.float32(cut_a)
    j = np.arange(blk + 2 * zc)
    out = x[2 * zc + j].copy()
    out[quiet[(j + zc // 2) // zc]] = 0
    return out, x[-4 * zc:].copy()


def level(db):
    """The amplitude of white noise whose RMS sits at ``db`` dB."""
    return np.float32(10.0 ** (db / 20.0))


def stretches(rng, n, zc, threhold, spread=2.0, loud=None, nan_at=None):
    """``n`` samples of noise whose level changes every 3 hops between ``threhold - spread`` and ``threhold + spread`` dB (so frames fall on
    both sides of the gate, some within a fraction of a dB); ``loud``: (index, value) of one sample that engages the 80 dB clip;
    ``nan_at``: index of one NaN."""
    x = rng.standard_normal(n).astype(np.float32)
    for lo in range(0, n, 3 * zc):
        x[lo: lo + 3 * zc] *= level(threhold + rng.uniform(-spread, spread))
    if loud is not None:
        x[loud[0]] = np.float32(loud[1])
    if nan_at is not None:
        x[nan_at] = np.float32("nan")
    return x


def loud_value(threhold):
    """One sample of this height lifts a frame's RMS far enough that ``max - 80 dB`` lies above the threshold: every frame of the call is
    kept.  (RMS of the frame = value / sqrt(4 zc); 30 dB of room covers zc up to 480.)"""
    return float(10.0 ** ((threhold + 80.0 + 40.0) / 20.0))
