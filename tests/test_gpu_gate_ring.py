"""The bank's noise reduction on the device: rvcmi_glue_spectral_gate_ring_batch (the spectral gate over a rolling cache of noise spectra)
against rvcmi_glue_spectral_gate on contiguous copies of the same rows -- the two run the same instructions per frame, so every comparison is
``torch.equal``: the output, the threshold / maximum statistics, and the cached noise spectra themselves.  Five consecutive steps per case
(the ring wraps), S = 3 with the modes rotating through off / cold / warm, rows that are slices of longer buffers with canaries around them.
Then TorchGateBank's state machine, rvcmi_glue_nr_stitch_batch and rvcmi_glue_masked_write_batch against torch, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import gate_cases as gc

S, PAD, STEPS = 3, 5, 5
CANARY = -77.25
GEOMS = [(8, 2), (64, 16), (100, 25)]
FNS = [7, 8, 9, 17, 40]    # GATE_FT - 1, GATE_FT and GATE_FT + 1 noise frames, two tiles and a frame, five tiles


def _a256(v):
    return (v + 255) // 256 * 256


def ring_layout(S_, n, n_fft, hop):
    """csrc/gate_ring.hpp's scratch restated: X | xmax | thresh | mask | frames, each part 256-byte aligned."""
    F, K = 1 + n // hop, n_fft // 2 + 1
    o, off = {}, 0
    for key, size in (("X", S_ * F * K * 16), ("xmax", S_ * K * 8), ("thresh", S_ * K * 8), ("mask", S_ * F * K * 4), ("frames", S_ * F * n_fft * 8)):
        o[key] = off
        off += _a256(size)
    o["total"] = off
    return o


def hann(n_fft, dev):
    return torch.hann_window(n_fft, dtype=torch.float64).to(dev)


def reference(x, xn, n_fft, hop, w, f, dev):
    """rvcmi_glue_spectral_gate on contiguous copies -> (out [S, Lout], xmax [S, K], thresh [S, K], XN [S, Fn, K, 2])."""
    from rvc_amd import _lib

    L = _lib.lib()
    x, xn = x.contiguous(), xn.contiguous()
    B, n, nn = x.shape[0], x.shape[1], xn.shape[1]
    F, Fn, K = 1 + n // hop, 1 + nn // hop, n_fft // 2 + 1
    lay = gc.layout(B, n, nn, n_fft, hop)
    nbytes = int(L.rvcmi_glue_spectral_gate_scratch_bytes(B, n, nn, n_fft, hop))
    assert nbytes == lay["total"]
    scratch = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
    out = torch.empty(B, hop * (n // hop), device=dev, dtype=torch.float32)
    nf, nt = (0, 0) if f is None else f.shape
    with torch.cuda.device(dev):
        _lib.check(L.rvcmi_glue_spectral_gate(_lib.ptr(x), B, n, _lib.ptr(xn), nn, n_fft, hop, _lib.ptr(w), _lib.ptr(f), int(nf), int(nt), 0, 1.5, 1.3, 0.1,
                                              20, 0.9, _lib.ptr(out), _lib.ptr(scratch), C.c_size_t(nbytes), _lib.stream_ptr(dev)))

    def part(key, shape):
        count = int(np.prod(shape))
        return scratch[lay[key]: lay[key] + 8 * count].view(torch.float64).view(shape).clone()

    return out, part("xmax", (B, K)), part("thresh", (B, K)), part("XN", (B, Fn, K, 2))


def signal(rng, rows, n, dev):
    """Tones plus noise at very different levels per row, so that the mask is neither all ones nor all zeros."""
    t = np.arange(n)
    x = np.stack([(0.5 / (r + 1)) * np.sin(0.37 * (r + 1) * t + r) + 0.05 * rng.standard_normal(n) for r in range(rows)])
    return torch.from_numpy(x.astype(np.float32)).to(dev)


def run_steps(n_fft, hop, Fn, shift, extra, f, dev, rng):
    """Five steps of the ring call on slices of canaried buffers against the reference; -> the number of active (session, step) pairs."""
    from rvc_amd import glue, _lib

    nn, n = (Fn - 1) * hop + (hop // 2), 9 * hop + 1
    tail = shift + extra
    Lout, K = hop * (n // hop), n_fft // 2 + 1
    w = hann(n_fft, dev)
    x_buf = torch.full((S, n + 2 * PAD), CANARY, device=dev)
    xn_buf = torch.full((S, nn + 2 * PAD), CANARY, device=dev)
    out_buf = torch.full((S, Lout + 2 * PAD), CANARY, device=dev)
    x, xn, out = x_buf[:, PAD: PAD + n], xn_buf[:, PAD: PAD + nn], out_buf[:, PAD: PAD + Lout]
    xn.copy_(signal(rng, S, nn, dev))
    rbytes = int(_lib.lib().rvcmi_glue_spectral_gate_ring_bytes(S, nn, n_fft, hop))
    assert rbytes == S * Fn * K * 16
    ring = torch.full((rbytes + 256,), 0xAB, device=dev, dtype=torch.uint8)   # 256 canary bytes behind the cache
    lay = ring_layout(S, n, n_fft, hop)
    assert lay["total"] == int(_lib.lib().rvcmi_glue_spectral_gate_ring_scratch_bytes(S, n, n_fft, hop))
    plan = glue.gate_ring_plan(nn, n_fft, hop, shift, tail)
    valid, base, active_pairs = [False] * S, 0, 0
    for step in range(STEPS):
        if step:   # the roll the caller vouches for: left by `shift`, the last `tail` samples new
            if 0 < shift < nn:
                xn[:, : nn - shift] = xn[:, shift:].clone()
            t = min(max(tail, shift), nn)
            if t:
                xn[:, nn - t:] = signal(rng, S, t, dev) * (1.0 + 0.3 * step)
        x.copy_(signal(rng, S, n, dev))
        phase = [(step + s) % 3 for s in range(S)]                     # 0 off, 1 cold, 2 warm (cold when there is nothing to be warm about)
        mode = [0 if p == 0 else (1 if (p == 2 and valid[s]) else 2) for s, p in enumerate(phase)]
        base += plan["advance"]
        out.fill_(123.5)
        scratch = torch.full((lay["total"],), 0xCD, device=dev, dtype=torch.uint8)
        ring_before = ring.clone()
        glue.spectral_gate_ring(x, xn, shift, tail, ring, base, torch.tensor(mode, dtype=torch.uint8, device=dev), 2 in mode, n_fft, hop, w, f,
                                n_std_thresh=1.5, prop_decrease=0.9, out=out, scratch=scratch)
        ref_out, ref_xmax, ref_thresh, ref_xn = reference(x, xn, n_fft, hop, w, f, dev)
        cache = ring[:rbytes].view(torch.float64).view(S, Fn, K, 2)
        cache_before = ring_before[:rbytes].view(torch.float64).view(S, Fn, K, 2)
        got = {k: scratch[lay[k]: lay[k] + S * K * 8].view(torch.float64).view(S, K) for k in ("xmax", "thresh")}
        slots = [(base + fr) % Fn for fr in range(Fn)]
        for s in range(S):
            what = "n_fft %d hop %d Fn %d shift %d tail %d step %d session %d mode %d" % (n_fft, hop, Fn, shift, tail, step, s, mode[s])
            if mode[s] == 0:
                assert bool((out[s] == 123.5).all()), "an off session's out row was written: " + what
                assert torch.equal(cache[s].view(torch.int64), cache_before[s].view(torch.int64)), "an off session's ring rows were written: " + what
                xs = scratch[lay["X"]:].view(-1)[s * (1 + n // hop) * K * 16: (s + 1) * (1 + n // hop) * K * 16]
                assert bool((xs == 0xCD).all()) and bool((got["thresh"][s].view(torch.uint8) == 0xCD).all()), "an off session's scratch was written: " + what
                continue
            active_pairs += 1
            assert torch.equal(cache[s][slots].view(torch.int64), ref_xn[s].view(torch.int64)), "cached noise spectra: " + what
            assert torch.equal(got["xmax"][s].view(torch.int64), ref_xmax[s].view(torch.int64)), "xmax: " + what
            assert torch.equal(got["thresh"][s].view(torch.int64), ref_thresh[s].view(torch.int64)), "thresh: " + what
            assert torch.equal(out[s], ref_out[s]), "out: " + what
            if mode[s] == 1 and plan["n_dirty"] < Fn:   # a warm session's clean slots were not rewritten (they are equal because they were kept)
                clean = [(base + fr) % Fn for fr in range(plan["head"], plan["back"])]
                assert torch.equal(cache[s][clean].view(torch.int64), cache_before[s][clean].view(torch.int64)), "clean slots: " + what
        valid = [m != 0 for m in mode]
        for buf, k in ((x_buf, n), (xn_buf, nn), (out_buf, Lout)):
            assert bool((buf[:, :PAD] == CANARY).all()) and bool((buf[:, PAD + k:] == CANARY).all()), "canary: step %d" % step
        assert bool((ring[rbytes:] == 0xAB).all())
        mask_vals = ref_out[[s for s in range(S) if mode[s]]]
        assert torch.isfinite(mask_vals).all()
    return active_pairs


@pytest.mark.gpu
@pytest.mark.parametrize("Fn", FNS)
@pytest.mark.parametrize("n_fft, hop", GEOMS)
def test_ring_equals_the_uncached_gate(n_fft, hop, Fn, gpu):
    from rvc_amd import TorchGateHIP

    rng = np.random.default_rng(1000 * n_fft + Fn)
    tg = TorchGateHIP(sr=gc.SR, n_fft=n_fft, prop_decrease=0.9, freq_mask_smooth_hz=2.5 * gc.SR / (n_fft / 2), time_mask_smooth_ms=1.5 * hop / gc.SR * 1000)
    filt = tg.smoothing_filter.reshape(tg.smoothing_filter.shape[-2], tg.smoothing_filter.shape[-1]).to(gpu, torch.float32).contiguous()
    assert tuple(filt.shape) == (5, 3)
    pairs = 0
    for shift in (0, hop, 3 * hop, Fn * hop, hop + 1):
        for extra in (0, 2 * hop):
            for f in (filt, None):
                pairs += run_steps(n_fft, hop, Fn, shift, extra, f, gpu, rng)
    assert pairs == 5 * 2 * 2 * 10   # 10 active (session, step) pairs per run


@pytest.mark.gpu
def test_ring_at_a_gui_frame_size(gpu):
    """n_fft = 1764, hop = 441 (the GUI's 44.1 kHz gate): four LDS chunks per frame, 14 bin groups."""
    rng = np.random.default_rng(1764)
    assert run_steps(1764, 441, 17, 441, 0, None, gpu, rng) == 10


@pytest.mark.gpu
def test_bank_object_goes_cold_after_a_pause_and_uploads_modes_only_on_change(gpu):
    """TorchGateBank over six blocks of a rolling buffer: session 1 is off for two steps and on again (stale -> cold), session 2 is
    invalidated once; every active row equals TorchGateHIP on that row alone."""
    from rvc_amd import TorchGateBank, TorchGateHIP

    n_fft, hop, blk = 64, 16, 48
    nn, n = 40 * hop, blk + 2 * hop
    tg = TorchGateHIP(sr=gc.SR, n_fft=n_fft, prop_decrease=0.9, freq_mask_smooth_hz=2.5 * gc.SR / (n_fft / 2), time_mask_smooth_ms=1.5 * hop / gc.SR * 1000).to(gpu)
    bank = TorchGateBank(tg, S, nn)
    assert bank.ring is None and bank.ring_bytes == S * 41 * 33 * 16
    rng = np.random.default_rng(9)
    buf = signal(rng, S, nn, gpu)
    actives = [[True, True, True], [True, True, True], [True, False, True], [True, False, True], [True, True, True], [True, True, True], [True, True, True]]
    want = [[2, 2, 2], [1, 1, 1], [1, 0, 2], [1, 0, 1], [1, 2, 1], [1, 1, 1], [1, 1, 1]]
    uploads, seen = 0, None
    for j, act in enumerate(actives):
        buf[:, :-blk] = buf[:, blk:].clone()
        buf[:, -blk:] = signal(rng, S, blk, gpu) * (1 + j)
        if j == 2:
            bank.invalidate(2)
        y = bank.forward(buf[:, -n:], buf, blk, blk, act)
        assert bank.last_modes == want[j], (j, bank.last_modes)
        if bank.mode is not seen:
            uploads, seen = uploads + 1, bank.mode
        for s in range(S):
            if act[s]:
                assert torch.equal(y[s], tg(buf[s, -n:][None], buf[s][None])[0]), (j, s)
    assert uploads == 6   # every block but the last, which repeats its predecessor's modes


@pytest.mark.gpu
def test_bank_object_without_the_cache_gives_the_same_rows(gpu, monkeypatch):
    """RVCMI_GATE_RING=0 (development): every active session cold in every call."""
    from rvc_amd import TorchGateBank, TorchGateHIP

    monkeypatch.setenv("RVCMI_GATE_RING", "0")
    tg = TorchGateHIP(sr=gc.SR, n_fft=64, prop_decrease=0.9, freq_mask_smooth_hz=None, time_mask_smooth_ms=None).to(gpu)
    bank = TorchGateBank(tg, 2, 640)
    rng = np.random.default_rng(3)
    buf = signal(rng, 2, 640, gpu)
    for j in range(3):
        buf[:, :-48] = buf[:, 48:].clone()
        buf[:, -48:] = signal(rng, 2, 48, gpu)
        y = bank.forward(buf[:, -80:], buf, 48, 48, [True, j != 1])
        assert bank.last_modes == [2, 2 if j != 1 else 0]
        assert torch.equal(y[0], tg(buf[0, -80:][None], buf[0][None])[0])


@pytest.mark.gpu
@pytest.mark.parametrize("Lb, blk, nd", [(4, 7, 30), (8, 8, 8), (300, 700, 2100)])
def test_nr_stitch_equals_the_three_torch_statements(Lb, blk, nd, gpu):
    from rvc_amd import glue

    rng = np.random.default_rng(Lb)
    mk = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(gpu)
    g_buf, nr_buf, den_buf = mk(S, blk + Lb + 2 * PAD), mk(S, Lb + 2 * PAD), mk(S, nd + 2 * PAD)
    g, nr, den = g_buf[:, PAD: PAD + blk + Lb], nr_buf[:, PAD: PAD + Lb], den_buf[:, PAD: PAD + nd]
    fade_in = torch.sin(0.5 * np.pi * torch.linspace(0.0, 1.0, steps=Lb, dtype=torch.float32)) ** 2
    fi, fo = fade_in.to(gpu), (1 - fade_in).to(gpu)
    mode = torch.tensor([1, 0, 2], dtype=torch.uint8, device=gpu)
    g0, nr0, den0 = g_buf.clone(), nr_buf.clone(), den_buf.clone()
    want_nr, want_den = nr.clone(), den.clone()
    for s in (0, 2):   # RealtimeStream.process, gui.py:986-990
        d, b, w = den[s].clone(), nr[s].clone(), g[s].clone()
        d[:-blk] = d[blk:].clone()
        w[:Lb] *= fi
        w[:Lb] += b * fo
        d[-blk:] = w[:blk]
        b[:] = w[blk:]
        want_nr[s], want_den[s] = b, d
    glue.nr_stitch_batch(g, nr, den, fi, fo, blk, mode, den_prev=den[:, blk:].clone() if nd > blk else None)
    assert torch.equal(nr, want_nr) and torch.equal(den, want_den)
    assert torch.equal(g_buf, g0)
    for buf, ref, k in ((nr_buf, nr0, Lb), (den_buf, den0, nd)):
        assert torch.equal(buf[:, :PAD], ref[:, :PAD]) and torch.equal(buf[:, PAD + k:], ref[:, PAD + k:])
    assert torch.equal(nr_buf[1], nr0[1]) and torch.equal(den_buf[1], den0[1])


@pytest.mark.gpu
def test_masked_write_picks_the_range_per_session(gpu):
    from rvc_amd import glue

    rng = np.random.default_rng(11)
    mk = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(gpu)
    dst_buf, a, b = mk(S, 600 + 2 * PAD), mk(S, 257), mk(S, 300)
    dst = dst_buf[:, PAD: PAD + 600]
    mode = torch.tensor([0, 2, 1], dtype=torch.uint8, device=gpu)
    want = dst_buf.clone()
    want[0, PAD + 300: PAD + 600] = b[0]
    want[1, PAD + 343: PAD + 600], want[2, PAD + 343: PAD + 600] = a[1], a[2]
    glue.masked_write_batch(dst, mode, a, 343, b, 300)
    assert torch.equal(dst_buf, want)
    glue.masked_write_batch(dst, mode, b[:, :5], 0)
    want[1, PAD: PAD + 5], want[2, PAD: PAD + 5] = b[1, :5], b[2, :5]
    assert torch.equal(dst_buf, want)
    L = __import__("rvc_amd")._lib
    p, st = L.ptr, L.stream_ptr(gpu)
    assert L.lib().rvcmi_glue_masked_write_batch(S, p(dst), 610, 600, p(a), 257, 344, 257, None, 0, 0, 0, p(mode), st) == L.ERR_INVALID
    assert L.lib().rvcmi_glue_masked_write_batch(0, p(dst), 610, 600, p(a), 257, 0, 257, None, 0, 0, 0, p(mode), st) == L.ERR_INVALID
    assert L.lib().rvcmi_glue_masked_write_batch(S, p(dst), 599, 600, p(a), 257, 0, 257, None, 0, 0, 0, p(mode), st) == L.ERR_INVALID


@pytest.mark.gpu
def test_rejections_return_invalid_and_launch_nothing(gpu):
    from rvc_amd import _lib

    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr(gpu)
    n_fft, hop, n, nn = 64, 16, 80, 640
    x, xn = torch.zeros(S, n, device=gpu), torch.zeros(S, nn, device=gpu)
    out = torch.full((S, 80), 5.0, device=gpu)
    w = hann(n_fft, gpu)
    mode = torch.full((S,), 2, dtype=torch.uint8, device=gpu)
    rb, sb = int(L.rvcmi_glue_spectral_gate_ring_bytes(S, nn, n_fft, hop)), int(L.rvcmi_glue_spectral_gate_ring_scratch_bytes(S, n, n_fft, hop))
    ring, scratch = torch.zeros(rb, dtype=torch.uint8, device=gpu), torch.zeros(sb, dtype=torch.uint8, device=gpu)

    def call(S_=S, xs=n, ns=nn, os_=80, n_fft_=n_fft, nonstat=0, rb_=rb, sb_=sb, win=None):
        return L.rvcmi_glue_spectral_gate_ring_batch(S_, p(x), xs, n, p(xn), ns, nn, p(out), os_, 16, 16, p(ring), C.c_size_t(rb_), 0, p(mode), 1, n_fft_, hop,
                                                     p(w if win is None else win), None, 0, 0, nonstat, 1.5, 0.9, p(scratch), C.c_size_t(sb_), st)

    assert call() == 0
    torch.cuda.synchronize(gpu)
    out.fill_(5.0)
    big = torch.zeros(4098, dtype=torch.float64, device=gpu)
    for kw in (dict(S_=0), dict(S_=65536), dict(xs=n - 1), dict(ns=nn - 1), dict(os_=79), dict(n_fft_=63), dict(n_fft_=4098, win=big), dict(nonstat=1),
               dict(rb_=rb - 1), dict(sb_=sb - 1)):
        assert call(**kw) == _lib.ERR_INVALID, kw
        assert b"spectral_gate_ring" in L.rvcmi_last_error()
    fi = torch.zeros(8, device=gpu)
    g, nr, den = torch.zeros(S, 24, device=gpu), torch.zeros(S, 8, device=gpu), torch.zeros(S, 64, device=gpu)
    stitch = lambda S_=S, gs=24, Lb=8, blk=16, nrs=8, ds=64, nd=64: L.rvcmi_glue_nr_stitch_batch(S_, p(g), gs, Lb, blk, p(fi), p(fi), p(nr), nrs, p(den), ds, nd, None, 0,
                                                                                              p(mode), st)
    assert stitch() == 0
    for kw in (dict(S_=0), dict(gs=23), dict(nrs=7), dict(ds=63), dict(Lb=17, gs=40, nrs=17), dict(nd=15, ds=15), dict(Lb=0)):
        assert stitch(**kw) == _lib.ERR_INVALID, kw
    torch.cuda.synchronize(gpu)
    assert bool((out == 5.0).all())
