"""oracle/gate_oracle.py pinned before anything is asked of the device (tests/gate_cases.py is the table):

(a) against torch on the CPU in fp64 -- torch.stft(pad_mode="constant", center=True), torch.std_mean, conv1d / conv2d(padding="same"),
    torch.istft -- on every case: which side an even kernel pads, that smoothing is a correlation, the win_length < n_fft centring,
    the output's length and trim;
(b) against the reference's own TorchGate run in fp64 (tests/golden/gui_torchgate_edges.npz, tools/make_golden_gate.py);
(c) against tests/golden/gui_torchgate.npz, the 13 cases at the GUI's sizes;
(d) every named wrong variant stands clear of the bar of the stage it corrupts, so the bars are tight enough to catch it;
(e) every stationary decision is at least 16x its own propagated bound from its threshold, none left out;
and TorchGateHIP's host-side overlap-add guard."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gate_cases as gc
from conftest import load_golden
from oracle import gate_oracle


def _torch_stages(name):
    """TorchGate.forward restated on torch's own fp64 ops, (bin, frame) layout turned to the oracle's (frame, bin)."""
    c = gc.CASES[name]
    x, xn = gc.inputs(name)
    if c.window == "hann":  # as the class calls it: the short window, centred by torch
        wl = c.n_fft if c.win_length is None else c.win_length
        kw = dict(n_fft=c.n_fft, hop_length=c.hop, win_length=wl, window=torch.hann_window(wl, dtype=torch.float64))
    else:
        kw = dict(n_fft=c.n_fft, hop_length=c.hop, win_length=c.n_fft, window=torch.from_numpy(gc.window(c)))

    def stft(v):
        return torch.stft(torch.tensor(v, dtype=torch.float64), return_complex=True, pad_mode="constant", center=True, **kw)

    def amp_to_db(X):
        db = 20 * torch.log10(X.abs() + torch.finfo(torch.float64).eps)
        return torch.max(db, (db.max(-1).values - 40).unsqueeze(-1))

    X = stft(x)
    r = {"X": X}
    if c.nonstat:
        a = X.abs()
        s = F.conv1d(a.reshape(-1, 1, a.shape[-1]), torch.ones(1, 1, c.nmm, dtype=torch.float64), padding="same").view(a.shape) / c.nmm
        m = torch.sigmoid(((a - s) / (s + 1e-6) - 1.3) / c.temp)
    else:
        X_db = amp_to_db(X)
        XN_db = amp_to_db(stft(xn)) if xn is not None else X_db
        std, mean = torch.std_mean(XN_db, dim=-1)
        r["thresh"] = mean + std * 1.5
        m = X_db > r["thresh"].unsqueeze(2)
    m = c.prop * (m.float() - 1.0) + 1.0
    r["mraw"] = m
    f = gc.filt(name)
    msk = m.double()
    if f is not None:
        msk = F.conv2d(msk.unsqueeze(1), torch.from_numpy(f).double()[None, None], padding="same").squeeze(1)
    r["msk"] = msk
    r["Y"] = X * msk
    if c.Lout:
        r["y"] = torch.istft(r["Y"], center=True, **kw)
    return {k: (v.transpose(1, 2) if v.dim() == 3 else v).numpy() for k, v in r.items()}


@pytest.mark.parametrize("name", gc.NAMES)
def test_oracle_equals_torch_fp64_stage_by_stage(name):
    """(a).  torch's FFT is well inside the direct sum's bound, so the bars of the device are the bars here; the stationary mask is
    compared for equality (part (e) makes that well defined) and the non-stationary one at its own bar."""
    c, o = gc.CASES[name], gc.oracle(name)
    with torch.no_grad():
        t = _torch_stages(name)
    keep = [b for b in range(c.B) if b not in gc.zero_rows(name) or c.nonstat]
    assert gc.ratio(t["X"], o["X"], o["bar_X"]) <= 1.0
    if not c.nonstat:
        assert gc.ratio(t["thresh"], o["thresh"], o["bar_thresh"]) <= 1.0
        assert np.array_equal(t["mraw"][keep], o["mraw"][keep])
    else:
        assert gc.ratio(t["mraw"], o["mraw"], o["bar_mraw"]) <= 1.0
    assert t["mraw"].dtype == np.float32 and o["mraw"].dtype == np.float32
    assert gc.ratio(t["msk"][keep], o["msk"][keep], o["bar_msk"][keep]) <= 1.0
    assert gc.ratio(t["Y"][keep], o["Y"][keep], o["bar_Y"][keep]) <= 1.0
    assert o["y"].shape == (c.B, c.Lout)
    if c.Lout:
        assert gc.ratio(t["y"], o["y"], o["bar_y"]) <= 1.0
    for k, v in o.items():
        if k.startswith("bar_") and k != "bar_thresh":
            assert np.isfinite(v).all() and (np.asarray(v) >= 0).all(), k


def test_fn1_threshold_is_nan_and_the_output_finite():
    o = gc.oracle("Fn1")
    c = gc.CASES["Fn1"]
    x, _ = gc.inputs("Fn1")
    assert np.isnan(o["thresh"]).all() and (o["mraw"] == np.float32(0.9) * np.float32(-1) + np.float32(1)).all()
    assert np.isfinite(o["y"]).all()
    # mask all zero -> (1 - prop) x up to the smoothing's edge loss; without a filter it is (1 - prop) x to rounding
    plain = gc.run("Fn1", filt=None)
    want = float(o["mraw"][0, 0, 0]) * x[:, :c.Lout].astype(np.float64)
    assert gc.ratio(plain["y"], want, plain["bar_y"]) <= 1.0


def test_a_small_temperature_saturates_the_sigmoid_to_exactly_zero():
    """temp_coeff = 0.01: where the slowness ratio is well under its threshold the fp64 sigmoid is below the smallest fp32 number, so
    m is exactly 0 and the mask exactly 1 - prop; at temp_coeff = 0.1 the same input leaves every m positive."""
    c, o = gc.CASES["temp0.01"], gc.oracle("temp0.01")
    assert 0 < (o["m"] == 0).mean() < 1
    assert (o["mraw"][o["m"] == 0] == np.float32(c.prop) * np.float32(-1) + np.float32(1)).all()
    assert (gc.run("temp0.01", temp_coeff=0.1)["m"] > 0).all()


def _fixture_inputs_ok(d, name):
    x, xn = gc.inputs(name)
    h = hashlib.sha256(x.tobytes() + (xn.tobytes() if xn is not None else b"")).hexdigest()
    assert h == str(d[name + "_sha256"]), "regenerated inputs differ from the fixture's"


@pytest.mark.parametrize("name", gc.FIXTURE_CASES)
def test_oracle_reproduces_the_reference_class(name):
    """(b).  ref64 is the reference's TorchGate built and run under an fp64 default dtype: its mask is fp32 and so is its smoothing,
    so the oracle sums the smoothing in fp32 here and must land within the output's bar (which holds the fp32 chain's bound)."""
    d = load_golden("gui_torchgate_edges")
    _fixture_inputs_ok(d, name)
    o = gc.run(name, smooth_fp32=True)
    ref = d[name + "_ref64"]
    assert ref.dtype == np.float64 and ref.shape == o["y"].shape
    assert gc.ratio(ref, o["y"], gc.oracle(name)["bar_y"]) <= 1.0


def test_the_fixture_holds_every_case_the_class_can_express():
    d = load_golden("gui_torchgate_edges")
    assert sorted(k[:-len("_ref64")] for k in d if k.endswith("_ref64")) == sorted(gc.FIXTURE_CASES)
    dropped = set(gc.CLASS_CASES) - set(gc.FIXTURE_CASES)
    assert all(n.replace("_f17", "_f9") in gc.FIXTURE_CASES for n in dropped) and len(dropped) == 5


def test_oracle_reproduces_the_gui_fixture():
    """(c).  The 13 cases of tests/golden/gui_torchgate.npz at the GUI's sizes, the same check."""
    import rvc_amd
    from test_gpu_torchgate import GATE_CASES, _gate_inputs

    d = load_golden("gui_torchgate")
    assert len(GATE_CASES) == 13
    for case in GATE_CASES:
        x, xn, kind, sr = _gate_inputs(d, case)
        n_fft = 4 * (sr // 100)
        f = rvc_amd.TorchGateHIP(sr=sr, n_fft=n_fft, prop_decrease=0.9).smoothing_filter[0, 0].numpy()
        o = gate_oracle.gate(x, None if kind == "none" else xn, n_fft, n_fft // 4, gate_oracle.hann_window(n_fft), f,
                             nonstationary=kind == "nonstat", prop_decrease=0.9, smooth_fp32=True)
        q = gc.ratio(d[case + "_ref64"], o["y"], o["bar_y"])
        assert q <= 1.0, (case, q)


# (d): variant -> (the stage it corrupts, a table case on which it must show)
WRONG = {
    "biased_std": ("thresh", "Fn2"),
    "clamp_from_x": ("thresh", "quiet_xn"),
    "no_clamp": ("thresh", "deep_lead"),
    "reflect_pad": ("X", "F9"),
    "symmetric_hann": ("X", "F9"),
    "window_not_centred": ("X", "win64"),
    "movemean_other_side": ("mraw", "nmm20"),
    "smooth_flipped": ("Y", "filt_2x3"),
    "smooth_other_side": ("Y", "filt_4x1"),
    "ola_no_division": ("y", "F9"),
    "keep_last_partial_hop": ("y", "F9"),
}


def test_every_variant_is_named():
    assert sorted(WRONG) == sorted(gate_oracle.VARIANTS + gate_oracle.WINDOW_VARIANTS)


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_wrong_variant_stands_clear_of_its_bar(variant):
    stage, name = WRONG[variant]
    o, w = gc.oracle(name), gc.run(name, variant=variant)
    got, want, bar = w[stage], o[stage], np.broadcast_to(o["bar_" + stage], o[stage].shape)
    if got.shape != want.shape:  # a longer output: the samples it should not have, against the widest bar of those it should
        n = want.shape[-1]
        assert got.shape[-1] > n and gc.ratio(got[..., :n], want, bar) <= 1.0
        clear = np.abs(got[..., n:]).max() / bar.max()
    else:
        clear = gc.ratio(got, want, bar)
    assert clear >= 1.25, "%s on %s: only %.3g x the bar of %s" % (variant, name, clear, stage)


def test_other_padding_side_only_shows_on_even_kernels():
    """The two conventions agree for odd sizes; the table's even ones (n_movemean = 2, 20; 4 x 1, 2 x 3) are what tells them apart."""
    for name, variant, stage in (("nmm19", "movemean_other_side", "mraw"), ("nmm21", "movemean_other_side", "mraw"),
                                 ("filt_1x5", "smooth_other_side", "Y")):
        assert np.array_equal(gc.run(name, variant=variant)[stage], gc.oracle(name)[stage]), name
    assert not np.array_equal(gc.run("nmm2", variant="movemean_other_side")["mraw"], gc.oracle("nmm2")["mraw"])
    for name in ("filt_2x3", "filt_3x4"):  # an even side over bins, and one over frames
        assert gc.ratio(gc.run(name, variant="smooth_other_side")["Y"], gc.oracle(name)["Y"], gc.oracle(name)["bar_Y"]) >= 1.25


@pytest.mark.parametrize("name", gc.STATIONARY)
def test_every_stationary_decision_is_16x_its_bound_from_the_threshold(name):
    """(e).  No decision is excluded: only a row whose x is all zero (its output is zero whatever the mask) and a single noise frame
    (NaN threshold: every decision is false) have nothing to check."""
    c, o = gc.CASES[name], gc.oracle(name)
    if name == "Fn1":
        assert np.isnan(o["thresh"]).all() and (o["mraw"] == np.float32(1) - np.float32(c.prop)).all()
        return
    keep = [b for b in range(c.B) if b not in gc.zero_rows(name)]
    margin, bound = o["margin"][keep], o["margin_bound"][keep]
    assert margin.shape == (len(keep), c.F, c.K) and np.isfinite(margin).all() and np.isfinite(bound).all()
    assert (margin >= 16.0 * bound).all(), "smallest margin / bound %.3g" % float((margin / bound).min())
    if c.prop > 0:
        assert 0 < (o["mraw"][keep] == 1).sum() < o["mraw"][keep].size or name == "quiet_xn"   # both outcomes occur


@pytest.mark.parametrize("name", gc.GROUPS["prop"][:3])
def test_prop_decrease_zero_returns_x_bit_for_bit(name):
    """prop_decrease = 0 and no filter: the mask is exactly 1 (0 * (m - 1) + 1 in fp32), Y = X, and the true output is x itself, an
    fp32 number.  The device's fp64 result is within bar_y64 of it, and rounds back to x when that is under a quarter of an fp32 ulp at
    the sample (a quarter: below a power of two the neighbour is half as far).  The worst-case bar is absolute, so it proves this for
    all but the samples closest to zero; it does at the signal's RMS, and the oracle's own fp64 round trip rounds to x on EVERY sample,
    which is what the device test demands."""
    c, o = gc.CASES[name], gc.oracle(name)
    x, _ = gc.inputs(name)
    x = x[:, :c.Lout]
    assert c.prop == 0.0 and c.filt is None and (o["mraw"] == 1).all() and np.array_equal(o["Y"], o["X"])
    assert np.array_equal(o["y"].astype(np.float32), x)
    quarter_ulp = 0.25 * np.spacing(np.abs(x)).astype(np.float64)
    rms = np.float32(np.sqrt(np.mean(x.astype(np.float64) ** 2)))
    assert o["bar_y64"].max() < 0.25 * float(np.spacing(rms))
    proven = float((o["bar_y64"] < quarter_ulp).mean())
    print("%s: bit-equality proven by the worst-case bound on %.1f %% of the samples" % (name, 100 * proven))
    assert proven > 0.9


def test_scratch_layout_restated():
    """Each part 256-byte aligned, in the documented order; the total is checked against the library on the device."""
    lay = gc.layout(3, 300, 500, 128, 32)
    F, Fn, K = 10, 16, 65
    assert [lay[k] for k in ("X", "XN", "xmax", "thresh", "mask", "frames")] == sorted(lay[k] for k in ("X", "XN", "xmax", "thresh", "mask", "frames"))
    assert lay["XN"] == gc._a256(3 * F * K * 16) and lay["xmax"] - lay["XN"] == gc._a256(3 * Fn * K * 16)
    assert lay["total"] - lay["frames"] == gc._a256(3 * F * 128 * 8) and all(v % 256 == 0 for v in lay.values())
    assert gc.layout(1, 300, 0, 128, 32)["xmax"] == gc.layout(1, 300, 0, 128, 32)["XN"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# TorchGateHIP's overlap-add guard (host side)
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(n_fft=128, hop_length=128), dict(n_fft=128, win_length=64, hop_length=96),
                                dict(n_fft=128, win_length=32, hop_length=33)], ids=["hann_hop_n_fft", "hop_gt_win", "hop_win_plus_1"])
def test_gate_refuses_what_istft_refuses(kw):
    import rvc_amd

    tg = rvc_amd.TorchGateHIP(sr=gc.SR, freq_mask_smooth_hz=None, time_mask_smooth_ms=None, **kw)
    wl = kw.get("win_length", kw["n_fft"])
    L = 1000
    Y = torch.stft(torch.randn(1, L, dtype=torch.float64), n_fft=kw["n_fft"], hop_length=kw["hop_length"], win_length=wl,
                   window=torch.hann_window(wl, dtype=torch.float64), return_complex=True, pad_mode="constant", center=True)
    with pytest.raises(RuntimeError, match="window overlap add min|hop_length <= win_length"):
        torch.istft(Y, n_fft=kw["n_fft"], hop_length=kw["hop_length"], win_length=wl, window=torch.hann_window(wl, dtype=torch.float64))
    with pytest.raises(ValueError, match="window overlap add min"):
        tg._check_overlap_add(L)


@pytest.mark.parametrize("name", [n for n in gc.CLASS_CASES if gc.CASES[n].n_fft <= 128] + ["nfft4096_f9"])
def test_gate_accepts_what_istft_accepts(name):
    """Every table case the class can express passes the guard, and its envelope over the kept range is what the guard summed."""
    import rvc_amd

    c = gc.CASES[name]
    tg = rvc_amd.TorchGateHIP(**gc.class_kwargs(c))
    tg._check_overlap_add(c.L)
    if c.Lout:
        assert gate_oracle.ola_envelope(gc.window(c), c.n_fft, c.hop, c.L).min() >= 1e-11
    assert np.array_equal(tg._window(torch.device("cpu")).numpy(), gc.window(c))


def test_guard_follows_the_number_of_frames():
    """hann(64) centred in 128 with hop 48: two frames leave nothing uncovered inside the kept range, a third does not change that; with
    hop 96 the gap between frames 0 and 1 is inside it as soon as there are two.  The guard sums the call's own frames, as istft does."""
    import rvc_amd

    ok = rvc_amd.TorchGateHIP(sr=gc.SR, n_fft=128, win_length=64, hop_length=48, freq_mask_smooth_hz=None, time_mask_smooth_ms=None)
    for L in (10, 48, 100, 5000):
        ok._check_overlap_add(L)
    bad = rvc_amd.TorchGateHIP(sr=gc.SR, n_fft=128, win_length=64, hop_length=96, freq_mask_smooth_hz=None, time_mask_smooth_ms=None)
    bad._check_overlap_add(95)  # one frame: nothing is kept
    for L in (96, 200, 5000):
        with pytest.raises(ValueError, match="window overlap add min"):
            bad._check_overlap_add(L)
