"""The spectral gate on the device, stage by stage, on every tile edge (tests/gate_cases.py): rvcmi_glue_spectral_gate called through the
C ABI with a caller-owned scratch, and X * mask, XN, xmax, thresh, the raw mask and the windowed frames read back at the offsets of the
documented layout (csrc/glue.hip), each compared with oracle/gate_oracle.py at the bar the oracle derives from the case's own data.  X
before masking is overwritten in place, so it is checked through a prop_decrease = 0, no-filter call of the same case, where Y == X.
Stationary masks must be bit-equal (tests/test_cpu_gate_oracle.py shows every decision is 16x its bound clear of its threshold).  Then
TorchGateHIP against the raw call, bit-equality where the arithmetic leaves no room, and batch / dtype invariance."""
import ctypes as C

import numpy as np
import pytest
import torch

import gate_cases as gc

pytestmark = pytest.mark.gpu


def _dev(a, dev, dtype=None):
    return None if a is None else torch.tensor(np.asarray(a), device=dev, dtype=dtype)


def device_run(name, dev, prop=None, no_filter=False):
    """One call of the C entry point on the case; -> (out [B, Lout] fp32, the scratch's stages as numpy arrays)."""
    from rvc_amd import _lib

    c = gc.CASES[name]
    x, xn = gc.inputs(name)
    B, F, K = c.B, c.F, c.K
    Fn = 1 + c.Ln // c.hop if c.Ln else 0
    assert not (c.nonstat and c.Ln)  # (the layout's XN part exists only for a stationary call with a noise signal)
    L = _lib.lib()
    lay = gc.layout(B, c.L, c.Ln, c.n_fft, c.hop)
    nbytes = int(L.rvcmi_glue_spectral_gate_scratch_bytes(B, c.L, c.Ln, c.n_fft, c.hop))
    assert nbytes == lay["total"], "the restated layout disagrees with the library: %d vs %d bytes" % (lay["total"], nbytes)
    xd, xnd, w = _dev(x, dev), _dev(xn, dev), _dev(gc.window(c), dev, torch.float64)
    f = None if no_filter else _dev(gc.filt(name), dev)
    nf, nt = (0, 0) if f is None else f.shape
    scratch = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    out = torch.full((B, max(c.Lout, 1)), float("nan"), device=dev, dtype=torch.float32)  # (never null, also when nothing is written)
    with torch.cuda.device(dev):
        _lib.check(L.rvcmi_glue_spectral_gate(_lib.ptr(xd), B, c.L, _lib.ptr(xnd), c.Ln, c.n_fft, c.hop, _lib.ptr(w), _lib.ptr(f), int(nf), int(nt),
                                              1 if c.nonstat else 0, 1.5, 1.3, float(c.temp), int(c.nmm), float(c.prop if prop is None else prop),
                                              _lib.ptr(out), _lib.ptr(scratch), C.c_size_t(nbytes), _lib.stream_ptr(dev)))
    torch.cuda.synchronize(dev)

    def part(key, count, dtype, shape):
        size = torch.empty(0, dtype=dtype).element_size()
        return scratch[lay[key]: lay[key] + count * size].view(dtype).view(shape).cpu().numpy()

    Y = part("X", B * F * K * 2, torch.float64, (B, F, K, 2))
    s = dict(Y=Y[..., 0] + 1j * Y[..., 1], xmax=part("xmax", B * K, torch.float64, (B, K)), thresh=part("thresh", B * K, torch.float64, (B, K)),
             mraw=part("mask", B * F * K, torch.float32, (B, F, K)), z=part("frames", B * F * c.n_fft, torch.float64, (B, F, c.n_fft)))
    if Fn:
        XN = part("XN", B * Fn * K * 2, torch.float64, (B, Fn, K, 2))
        s["XN"] = XN[..., 0] + 1j * XN[..., 1]
    return out[:, :c.Lout].contiguous(), s


def stage_ratios(name, dev):
    """error / bar of every stage of a case (the worst entry); a stationary mask counts its differing entries instead."""
    c, o = gc.CASES[name], gc.oracle(name)
    out, s = device_run(name, dev)
    _, s0 = device_run(name, dev, prop=0.0, no_filter=True)
    keep = [b for b in range(c.B) if b not in gc.zero_rows(name) or c.nonstat]
    q = {"X": gc.ratio(s0["Y"], gc.oracle_x(name)["X"], o["bar_X"]), "xmax": gc.ratio(s["xmax"], o["xmax"], o["bar_xmax"])}
    assert np.array_equal(gc.oracle_x(name)["X"], o["X"])
    if "XN" in s:
        q["XN"] = gc.ratio(s["XN"], o["XN"], o["bar_XN"])
    if c.nonstat:
        q["mraw"] = gc.ratio(s["mraw"], o["mraw"], o["bar_mraw"])
    else:
        q["thresh"] = gc.ratio(s["thresh"], o["thresh"], o["bar_thresh"])
        q["mraw_differing"] = int((s["mraw"][keep] != o["mraw"][keep]).sum())
    q["Y"] = gc.ratio(s["Y"], o["Y"], o["bar_Y"])
    q["z"] = gc.ratio(s["z"], o["z"], o["bar_z"])
    q["y"] = gc.ratio(out.cpu().numpy().astype(np.float64), o["y"], o["bar_y"])
    return q


@pytest.mark.parametrize("name", gc.NAMES)
def test_every_stage_is_within_its_derived_bar(name, gpu):
    q = stage_ratios(name, gpu)
    print("%-20s " % name + "  ".join("%s %.3g" % kv for kv in q.items()))
    differing = q.pop("mraw_differing", 0)
    assert differing == 0, "%d stationary mask values differ from the oracle's" % differing
    assert all(v <= 1.0 for v in q.values()), q


@pytest.mark.parametrize("name", gc.GROUPS["prop"][:3])
def test_prop_decrease_zero_returns_x_bit_for_bit(name, gpu):
    """The fp64 round trip is far inside half an fp32 ulp (derived in tests/test_cpu_gate_oracle.py): also at n_fft = 4096 and 2."""
    c = gc.CASES[name]
    out, s = device_run(name, gpu)
    assert (s["mraw"] == 1).all()
    assert torch.equal(out.cpu(), torch.tensor(gc.inputs(name)[0][:, :c.Lout]))


def _class_call(name, dev, rows=None, dtype=torch.float32, expand=False):
    import rvc_amd

    c = gc.CASES[name]
    x, xn = gc.inputs(name)
    if rows is not None:
        x, xn = x[rows], (xn[rows] if xn is not None else None)
    if expand:
        xn = xn[:1]
    tg = rvc_amd.TorchGateHIP(**gc.class_kwargs(c)).to(dev)
    return tg(_dev(x, dev, dtype), _dev(xn, dev, dtype))


@pytest.mark.parametrize("name", [n for n in gc.CLASS_CASES if n in gc.GROUPS["hopwin"] + gc.GROUPS["nonstat"] + gc.GROUPS["smoothing"]
                                  + gc.GROUPS["prop"] + gc.GROUPS["batch"] + ["nfft2_f9", "nfft4096_f9", "Fn1", "xn_none"]])
def test_the_class_is_the_raw_call(name, gpu):
    """TorchGateHIP builds the window (win_length < n_fft centred) and the filter on the host and allocates its own scratch: the same
    bits as the C call on the table's window and filter."""
    got = _class_call(name, gpu)
    out, _ = device_run(name, gpu)
    assert got.dtype == torch.float32 and torch.equal(got, out)


def test_a_single_noise_frame_masks_everything(gpu):
    """Fn = 1: torch's unbiased std of one frame is NaN, every decision is false, the mask is 1 - prop everywhere and the output finite."""
    c = gc.CASES["Fn1"]
    out, s = device_run("Fn1", gpu)
    assert np.isnan(s["thresh"]).all() and (s["mraw"] == np.float32(c.prop) * np.float32(-1) + np.float32(1)).all()
    assert torch.isfinite(out).all()


def test_one_frame_of_x_writes_its_stages_and_no_output(gpu):
    c = gc.CASES["F1"]
    out, s = device_run("F1", gpu)
    assert c.F == 1 and out.shape == (1, 0) and np.isfinite(s["z"]).all() and np.abs(s["Y"]).max() > 0


@pytest.mark.parametrize("name", gc.GROUPS["batch"])
def test_each_row_is_bit_equal_to_its_lone_call(name, gpu):
    both = _class_call(name, gpu)
    assert not torch.equal(both[0], both[2])
    for r in range(gc.CASES[name].B):
        assert torch.equal(both[r: r + 1], _class_call(name, gpu, rows=slice(r, r + 1))), r
    if name == "b3_zero_row":
        assert not both[1].any()


def test_xn_of_one_row_is_expanded(gpu):
    """gate.py: xn [1, Ln] against x [B, L] equals the explicit copy."""
    import rvc_amd

    c = gc.CASES["b3_gains"]
    x, xn = gc.inputs("b3_gains")
    tg = rvc_amd.TorchGateHIP(**gc.class_kwargs(c)).to(gpu)
    xd, xn0 = _dev(x, gpu), _dev(xn[:1], gpu)
    assert torch.equal(tg(xd, xn0), tg(xd, xn0.repeat(c.B, 1)))
    assert torch.equal(tg(xd, xn0[0]), tg(xd, xn0))  # a 1-D xn too


@pytest.mark.parametrize("name", ["b3_gains", "b3_nonstat"])
def test_fp64_input_returns_fp64_equal_to_the_fp32_call(name, gpu):
    y32, y64 = _class_call(name, gpu), _class_call(name, gpu, dtype=torch.float64)
    assert y64.dtype == torch.float64 and y32.dtype == torch.float32 and torch.equal(y64.float(), y32) and torch.equal(y64, y32.double())


def test_the_class_refuses_an_uncovered_overlap_add(gpu):
    """hann with hop = n_fft: the raw call divides 0 by 0 where no frame covers a sample; the class raises on the host, as torch.istft."""
    import rvc_amd

    x = torch.ones(1, 1000, device=gpu)
    tg = rvc_amd.TorchGateHIP(sr=gc.SR, n_fft=128, hop_length=128, freq_mask_smooth_hz=None, time_mask_smooth_ms=None).to(gpu)
    with pytest.raises(ValueError, match="window overlap add min"):
        tg(x)
    w = torch.hann_window(128, dtype=torch.float64, device=gpu)
    assert not torch.isfinite(rvc_amd.glue.spectral_gate(x, None, 128, 128, w)).all()   # the raw call leaves it to the caller
