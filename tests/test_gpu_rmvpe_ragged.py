"""Ragged batched RMVPE f0 (``RMVPEHIP.salience_batch`` / ``f0_batch``, ``rvcmi_unet_forward_ragged``, ``rvcmi_gru_forward_ragged``): waveforms
of different lengths packed along the frame axis, every sequence computed as its own call computes it.

The shapes are the smallest at which a boundary can go wrong: 5120 / 513 / 5037 samples are 33 / 4 / 32 frames, padded to 64 / 32 / 32 rows
(one sequence is a single row at the deepest U-Net level, two neighbours share every boundary, the layers that split their K loop run);
48077 + 5120 are 320 + 64 rows and reach the tiles that do not split.

  * each sequence's salience against the torch fp32 chain ON THAT SEQUENCE ALONE, at the bar of ``test_salience_against_the_torch_fp32_network``
    (max and RMS error no larger than the torch ``.half()`` chain's on that sequence);
  * no read across a boundary: a sequence's result is bit-equal when its neighbours change (same launch shapes, so any difference is a leak);
  * the degenerate forms are the dense path bit for bit, and the dense path gives the bits it gave before any ragged call;
  * the GRU entry alone (bit-equal to the dense entry per sequence; the bar of tests/test_gpu_gru.py against ``nn.GRU``) and the U-Net entry
    alone (the bar of tests/test_gpu_unet.py against the fp32 evaluation of each sequence alone);
  * ``f0_batch`` = the decode of its own salience; the refusals; the routing in ``convert_files``.
"""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import rmvpe_cases as rc  # noqa: E402
import unet_cases as uc  # noqa: E402
from test_gpu_dropin import rvc_tree  # noqa: E402,F401  (skeleton checkout)

pytestmark = pytest.mark.gpu
SMALL, LARGE = (5120, 513, 5037), (48077, 5120)


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _standin(half):
    return rc.RmvpeStandIn(torch.device("cuda:0"), half)


@functools.lru_cache(maxsize=None)
def _hip():
    import rvc_amd

    hip = rvc_amd.RMVPEHIP.from_reference(_standin(True))
    assert hip is not None and hip.is_half
    return hip


def _wav(n, seed=0, gain=1.0):
    return gain * (rc.signal("voiced", n, seed) + 0.3 * rc.signal("noise", n, seed + 1))


def _batch(lengths, seed=0, gain=1.0):
    return [_wav(n, seed + 10 * i, gain).to("cuda:0") for i, n in enumerate(lengths)]


@functools.lru_cache(maxsize=None)
def _references(lengths):
    """Per sequence (torch fp32 chain, torch .half() chain) on that sequence ALONE -- computed once, never changed."""
    r32, r16 = _standin(False), _standin(True)
    out = []
    with torch.no_grad():
        for w in _batch(lengths):
            ref = r32._mel2hidden(r32.mel_extractor(w[None], center=True))[0].float()
            half = r16._mel2hidden(r16.mel_extractor(w[None], center=True))[0].float()
            out.append((ref, half))
    return out


@pytest.fixture(scope="module", autouse=True)
def dense_before(gpu):
    """The dense [3, n] salience, computed before this module makes its first ragged call."""
    x = torch.stack(_batch((5037, 5037, 5037)))
    return x, _hip().salience(x).clone()


def _stream(gpu):
    return C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _offsets(rows, gpu):
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    return off, (C.c_int * len(off))(*off), torch.tensor(off, dtype=torch.int32, device=gpu)


# ---------------------------------------------------------------- 1. equals the separate call

@pytest.mark.parametrize("lengths", (SMALL, LARGE))
def test_every_sequence_meets_the_bar_of_its_own_call(lengths, gpu):
    got = _hip().salience_batch(_batch(lengths))
    assert len(got) == len(lengths)
    for i, (n, (ref, half)) in enumerate(zip(lengths, _references(lengths))):
        T = n // rc.HOP + 1
        g = got[i]
        assert g.shape == (T, 360) and g.dtype == torch.float32 and bool(torch.isfinite(g).all())
        e_hip, e_half = float((g - ref).abs().max()), float((half - ref).abs().max())
        r_hip, r_half = float((g - ref).pow(2).mean().sqrt()), float((half - ref).pow(2).mean().sqrt())
        print("ragged salience %s[%d] n=%d: HIP max %.3g rms %.3g | torch .half() max %.3g rms %.3g" % (lengths, i, n, e_hip, r_hip, e_half, r_half))
        assert float(ref.max()) - float(ref.min()) > 0.05, "the seeded network's salience is flat: the comparison would see nothing"
        assert e_half > 0 and e_hip <= e_half and r_hip <= r_half, (lengths, i, e_hip, e_half, r_hip, r_half)


# ---------------------------------------------------------------- 2. no leak across boundaries

@pytest.mark.parametrize("pos", (0, 1, 2))
def test_a_sequence_does_not_depend_on_its_neighbours(pos, gpu):
    hip = _hip()
    a = _batch(SMALL)
    b = _batch(SMALL, seed=100, gain=10.0)          # other content, 10x the amplitude, the same lengths
    b[pos] = a[pos]
    sa, sb = hip.salience_batch(a), hip.salience_batch(b)
    assert torch.equal(sa[pos], sb[pos]), "sequence %d changed with its neighbours: max |d| %.3g" % (pos, float((sa[pos] - sb[pos]).abs().max()))
    assert all(not torch.equal(sa[j], sb[j]) for j in range(3) if j != pos), "the neighbours did not change: the test would see nothing"


# ---------------------------------------------------------------- 3. the degenerate forms are the dense path

def test_one_sequence_and_equal_lengths_are_the_dense_path_bit_for_bit(dense_before, gpu):
    hip = _hip()
    for n in (513, 5120, 48077):
        w = _wav(n).to(gpu)
        assert torch.equal(hip.salience_batch([w])[0], hip.salience(w)), n
    x, before = dense_before
    got = hip.salience_batch(list(x))
    assert len(got) == 3 and all(torch.equal(got[i], before[i]) for i in range(3))
    assert torch.equal(hip.salience(x), before), "the dense path changed after ragged calls"


# ---------------------------------------------------------------- 4. the GRU piece alone

def test_ragged_gru_is_the_dense_gru_per_sequence(gpu):
    import rvc_amd
    from rvc_amd import _lib

    L = _lib.lib()
    torch.manual_seed(3)
    ref = torch.nn.GRU(384, 256, num_layers=1, batch_first=True, bidirectional=True).eval()
    m = rvc_amd.GRUHIP(ref, device=gpu)
    rows = (32, 96, 32)
    off, off_h, off_d = _offsets(rows, gpu)
    x = torch.randn(off[-1], 384, generator=torch.Generator().manual_seed(4)).half()
    xd = x.to(gpu)
    y = torch.full((off[-1], 512), float("nan"), device=gpu)
    hn = torch.full((2, 3, 256), float("nan"), device=gpu)
    _lib.check(L.rvcmi_gru_forward_ragged(m._h, 3, off_h, _p(off_d), _p(xd), _p(y), _p(hn), _stream(gpu)))
    errs = []
    for i, T in enumerate(rows):
        xi = xd[off[i]: off[i + 1]].contiguous()
        yi, hi = torch.empty(T, 512, device=gpu), torch.empty(2, 1, 256, device=gpu)
        _lib.check(L.rvcmi_gru_forward(m._h, 1, T, _p(xi), _p(yi), _p(hi), _stream(gpu)))
        assert torch.equal(y[off[i]: off[i + 1]], yi) and torch.equal(hn[:, i], hi[:, 0]), "sequence %d differs from its dense call" % i
        with torch.no_grad():
            y_ref, hn_ref = ref(x[off[i]: off[i + 1]].float()[None])
        errs.append((y[off[i]: off[i + 1]].cpu() - y_ref[0]).flatten())
        assert float((hn[:, i].cpu() - hn_ref[:, 0]).abs().max()) <= 1e-2
    e = torch.cat(errs)
    rms, mx = float(e.pow(2).mean().sqrt()), float(e.abs().max())
    print("ragged GRU vs nn.GRU fp32: RMS %.3e max %.3e" % (rms, mx))
    assert bool(torch.isfinite(y).all()) and rms <= 2e-3 and mx <= 1e-2


# ---------------------------------------------------------------- 5. the U-Net piece alone

def _unet_ragged(hip, mel_rows, rows, gpu):
    """mel_rows [R, 128] on the GPU -> [R, 384]"""
    from rvc_amd import _lib

    L = _lib.lib()
    off, off_h, off_d = _offsets(rows, gpu)
    nbytes = int(L.rvcmi_unet_workspace_bytes_ragged(hip._h, len(rows), off_h))
    assert nbytes > 0
    ws = torch.empty(nbytes, device=gpu, dtype=torch.uint8)
    out = torch.full((off[-1], 3, 128), float("nan"), device=gpu)
    _lib.check(L.rvcmi_unet_forward_ragged(hip._h, len(rows), off_h, _p(off_d), _p(mel_rows), _p(out), _p(ws), _stream(gpu)))
    return out.flatten(1), off


def test_ragged_unet_is_the_dense_unet_per_sequence(gpu):
    import rvc_amd

    sd = uc.seeded_weights(uc.golden_keys(), 17)
    hip = rvc_amd.UNetHIP.from_state_dict(sd, gpu)
    rows = (64, 32, 32)
    mels = [uc.seeded_mel(1, T, 200 + i) for i, T in enumerate(rows)]
    for i, T in enumerate((33, 4, 32)):  # zero pad frames behind the real ones, as the estimator's input has them
        mels[i][:, :, T:] = 0
    packed = torch.cat([m[0].T for m in mels]).contiguous().to(gpu)
    got, off = _unet_ragged(hip, packed, rows, gpu)
    assert bool(torch.isfinite(got).all())
    sd16 = uc.to(sd, gpu, torch.float16)
    for i, m in enumerate(mels):
        with torch.no_grad():
            ref = uc.forward(sd, m)[0]
            half = uc.forward(sd16, m.to(gpu).half())[0].float().cpu()
            dense = hip(m.to(gpu).transpose(-1, -2).unsqueeze(1)).transpose(1, 2).flatten(-2)[0]
        g = got[off[i]: off[i + 1]]
        e = g.cpu().double() - ref.double()
        h = half.double() - ref.double()
        r, mx, hr, hm = float(e.pow(2).mean().sqrt()), float(e.abs().max()), float(h.pow(2).mean().sqrt()), float(h.abs().max())
        de = dense.cpu().double() - ref.double()
        dd = (g - dense).cpu().double()
        d_r, d_mx, dd_r, dd_mx = float(de.pow(2).mean().sqrt()), float(de.abs().max()), float(dd.pow(2).mean().sqrt()), float(dd.abs().max())
        print("ragged unet seq %d (%d rows): rms %.4e max %.4e | torch .half() rms %.4e max %.4e | dense call vs fp32 rms %.4e max %.4e | "
              "ragged vs dense rms %.4e max %.4e" % (i, rows[i], r, mx, hr, hm, d_r, d_mx, dd_r, dd_mx))
        assert hr > 0 and r <= 2 * hr and mx <= 2 * hm, (i, r, mx, hr, hm)
    # Against the dense forward of each sequence ALONE, bit for bit wherever the two make the same sums.  A layer splits its K loop when its
    # launch has fewer than 128 blocks, and the split is chosen from the launch size; partial sums in another order flip fp16 roundings, which
    # the 56 residual units carry on like any other rounding, so at (64, 32, 32) rows the two are two evaluations of equal standing (the
    # figures above) and no bound below the sum of their errors follows from the formats.  Where the sums are the same, equality is exact:
    #   * the launch sizes of a dense call: one sequence = B 1; three equal lengths = B 3, each a single row at the deepest level;
    #   * unequal lengths with no split in either call: from 8192 rows on, the smallest launches (the 512-channel layers on rows / 32 x 4
    #     pixels: 64-pixel x 64-channel blocks) have 128 blocks.  8224 + 8192 rows put the boundary on an odd row of the deepest level.
    for rows_eq in ((64,), (32, 32, 32)):
        m = uc.seeded_mel(len(rows_eq), rows_eq[0], 400 + len(rows_eq))
        with torch.no_grad():
            dense = hip(m.to(gpu).transpose(-1, -2).unsqueeze(1)).transpose(1, 2).flatten(-2)
        got_eq, _ = _unet_ragged(hip, m.transpose(1, 2).reshape(-1, 128).contiguous().to(gpu), rows_eq, gpu)
        assert torch.equal(got_eq, dense.reshape(-1, 384)), "rows %s: not the dense path's bits" % (rows_eq,)
    rows_big = (8224, 8192)
    big = [uc.seeded_mel(1, T, 500 + j).to(gpu) for j, T in enumerate(rows_big)]
    got_big, off_big = _unet_ragged(hip, torch.cat([m[0].T for m in big]).contiguous(), rows_big, gpu)
    for j, m in enumerate(big):
        with torch.no_grad():
            dense = hip(m.transpose(-1, -2).unsqueeze(1)).transpose(1, 2).flatten(-2)[0]
        g = got_big[off_big[j]: off_big[j + 1]]
        assert torch.equal(g, dense), "sequence %d of %s differs from its dense call in %d values, max %.3g" % (
            j, rows_big, int((g != dense).sum()), float((g - dense).abs().max()))
    del big, got_big
    # the leak test at this level: other neighbours (pad rows included), the same bits
    for pos in range(3):
        other = [10 * uc.seeded_mel(1, T, 300 + j) for j, T in enumerate(rows)]
        other[pos] = mels[pos]
        got2, _ = _unet_ragged(hip, torch.cat([m[0].T for m in other]).contiguous().to(gpu), rows, gpu)
        assert torch.equal(got2[off[pos]: off[pos + 1]], got[off[pos]: off[pos + 1]]), "sequence %d reads a neighbour's rows" % pos


# ---------------------------------------------------------------- 6. f0_batch

def test_f0_batch_is_the_decode_of_its_own_salience(gpu):
    import rvc_amd

    hip = _hip()
    wavs = _batch(LARGE + (513,))
    sal = hip.salience_batch(wavs)
    p_lens = [300, 32, 4]
    for key in (0, 1.5):
        got = hip.f0_batch(wavs, p_lens, key)
        assert len(got) == 3
        for (pitch, pitchf), s, p in zip(got, sal, p_lens):
            want = rvc_amd.glue.rmvpe_f0(s, p, key, 0.03)
            assert pitch.shape == (1, p) and pitch.dtype == torch.int64 and pitchf.shape == (1, p) and pitchf.dtype == torch.float32
            assert torch.equal(pitch, want[0]) and torch.equal(pitchf, want[1])
    assert float(got[0][1].max()) > 0, "nothing voiced: the decode comparison would see nothing"


# ---------------------------------------------------------------- 7. refusals, identity

def test_refusals_and_run_to_run_identity(gpu):
    import rvc_amd
    from rvc_amd import _lib

    hip = _hip()
    wavs = _batch(SMALL)
    first = hip.salience_batch(wavs)
    for bad in ([], [wavs[0], wavs[1].cpu()], [wavs[0], wavs[1][:400]], wavs[0], [wavs[0], wavs[1][None]]):
        with pytest.raises(rvc_amd.RvcmiError):
            hip.salience_batch(bad)
        with pytest.raises(rvc_amd.RvcmiError):
            hip.f0_batch(bad, [4] * (len(bad) if isinstance(bad, list) else 1))
    with pytest.raises(rvc_amd.RvcmiError):
        hip.f0_batch(wavs, [32, 4])  # one p_len per waveform
    torch.empty(1 << 22, device=gpu).normal_()
    again = hip.salience_batch(wavs)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # the C level: nothing launched, the output untouched
    L = _lib.lib()
    mel = torch.zeros(128, 128, device=gpu)
    ws = torch.empty(int(hip.unet.workspace_bytes(1, 128)), device=gpu, dtype=torch.uint8)
    for rows, nseq in (((48, 48), 2), ((64, -32), 2), ((64, 0, 32), 3), ((32,), 0)):
        off, off_h, off_d = _offsets(rows, gpu)
        out = torch.full((128, 3, 128), float("nan"), device=gpu)
        assert L.rvcmi_unet_workspace_bytes_ragged(hip.unet._h, nseq, off_h) == 0
        code = L.rvcmi_unet_forward_ragged(hip.unet._h, nseq, off_h, _p(off_d), _p(mel), _p(out), _p(ws), _stream(gpu))
        torch.cuda.synchronize()
        assert code == _lib.ERR_INVALID and bool(torch.isnan(out).all()), rows
    off_h = (C.c_int * 3)(32, 64, 96)   # does not start at 0
    assert L.rvcmi_unet_workspace_bytes_ragged(hip.unet._h, 2, off_h) == 0
    x16 = torch.zeros(128, 384, device=gpu, dtype=torch.float16)
    for rows, nseq in (((64, -32), 2), ((64, 0), 2), ((32,), 0)):
        off, off_h, off_d = _offsets(rows, gpu)
        y = torch.full((128, 512), float("nan"), device=gpu)
        code = L.rvcmi_gru_forward_ragged(hip.gru._h, nseq, off_h, _p(off_d), _p(x16), _p(y), None, _stream(gpu))
        torch.cuda.synchronize()
        assert code == _lib.ERR_INVALID and bool(torch.isnan(y).all()), rows


# ---------------------------------------------------------------- 8. pipeline routing

def test_convert_files_routes_a_group_through_one_f0_batch(rvc_tree, gpu, tmp_path, monkeypatch):  # noqa: F811
    """The skeleton pipeline with a counting wrapper around ``RMVPEHIP.f0`` / ``f0_batch``: a group of three different lengths is ONE
    ``f0_batch`` call and no ``f0`` call, every file's segment receives that call's entry for it; ``RVCMI_RMVPE_BATCH=0`` gives per-file calls
    (without the variable the module default ``rmvpe.RMVPE_BATCH`` decides); a group of one, files with an ``f0_file``, another method and the
    switch off never enter the batch, and with the switch off the outputs are those of the per-file ``Pipeline.pipeline`` bit for bit (in the
    setting of the convert_files test of test_gpu_dropin.py: its geometry, estimator and pinned kernel families)."""
    import rvc_amd.rmvpe as rm
    import rvc_amd
    import rvc_amd.pipeline as rp
    from oracle import synth
    from test_gpu_prep import _webui_pipe

    d, seed, pl, pipe, net_g, tail = _webui_pipe(gpu, tmp_path, x_center=2, x_max=3)
    for key, val in (("RB_STREAM", 0), ("NO_RB_SPLIT", 1)):
        net_g.dec.set_option(key, val)
    for key, val in (("FR_NJ", 1), ("FR_FFN_SPLIT", 1), ("FR_WN_SPLIT", 1)):
        net_g._rvcmi_front.set_option(key, val)
    monkeypatch.delenv("RVCMI_RMVPE_BATCH", raising=False)
    monkeypatch.delenv("RVCMI_DEVICE_PREP", raising=False)
    r = rc.RmvpeStandIn(gpu, True)

    def host_f0(x, p_len, f0_up_key, f0_method, filter_radius, inp_f0=None):
        host.append(f0_method if inp_f0 is None else "f0_file")
        return np.full(p_len, 100, dtype=np.int64), np.full(p_len, 220.0, dtype=np.float32)

    pipe.f0_gen = types.SimpleNamespace(rmvpe=r, is_half=True, device=gpu, calculate=host_f0)
    audios = [synth.make_audio16k(n, seed + 1 + i) for i, n in enumerate((30000, 20000, 47000))]
    assert all(a.shape[0] + pipe.window <= pipe.t_max for a in audios)  # one segment per file
    hub = synth.FakeHubert(768, seed)
    calls, batches, host, fed = [], [], [], []
    real_f0, real_batch, real_hub = rvc_amd.RMVPEHIP.f0, rvc_amd.RMVPEHIP.f0_batch, rp.hubert_device
    monkeypatch.setattr(rvc_amd.RMVPEHIP, "f0", lambda self, *a, **k: (calls.append(1), real_f0(self, *a, **k))[1])
    monkeypatch.setattr(rvc_amd.RMVPEHIP, "f0_batch", lambda self, *a, **k: (lambda res: (batches.append(res), res)[1])(real_batch(self, *a, **k)))
    monkeypatch.setattr(rp, "hubert_device", lambda self, model, a0, pt, pf, version: (fed.append((pt, pf)), real_hub(self, model, a0, pt, pf, version))[1])

    def convert(files, method="rmvpe", f0_files=None):
        del calls[:], batches[:], host[:], fed[:]
        torch.manual_seed(5)
        t = tail[:1] + (method,) + tail[2:]
        return pipe.convert_files(hub, net_g, int(d["sid"]), [a.copy() for a in files], [0, 0, 0], *t, f0_files=f0_files)

    monkeypatch.setenv("RVCMI_RMVPE_HIP", "1")
    monkeypatch.setenv("RVCMI_RMVPE_BATCH", "1")
    on = convert(audios)
    assert len(batches) == 1 and calls == [] and host == [] and len(fed) == 3 and len(batches[0]) == 3
    for (pt, pf), (pitch, pitchf) in zip(fed, batches[0]):
        assert torch.equal(pt, pitch) and torch.equal(pf, pitchf)
    assert len(on) == 3 and all(np.isfinite(o).all() for o in on)
    monkeypatch.setenv("RVCMI_RMVPE_BATCH", "0")
    per_file = convert(audios)
    assert batches == [] and calls == [1, 1, 1]
    assert all(o.shape == p.shape for o, p in zip(on, per_file))
    monkeypatch.delenv("RVCMI_RMVPE_BATCH")
    convert(audios)
    assert (len(batches) == 1 and calls == []) if rm.RMVPE_BATCH else (batches == [] and calls == [1, 1, 1])
    monkeypatch.setenv("RVCMI_RMVPE_BATCH", "1")
    convert(audios[:1])
    assert batches == [] and calls == [1]
    f0_path = tmp_path / "f0.csv"
    f0_path.write_text("0.0,220.0\n1.0,230.0\n")
    named = types.SimpleNamespace(name=str(f0_path))
    convert(audios, f0_files=[named, None, named])
    assert batches == [] and calls == [1] and host == ["f0_file", "f0_file"]
    convert(audios, method="pm")
    assert batches == [] and calls == [] and host == ["pm"] * 3
    monkeypatch.setenv("RVCMI_RMVPE_HIP", "0")
    off = convert(audios)
    assert batches == [] and calls == [] and r.hidden_calls == 3  # the object's own mel extractor and network, once per file
    assert all(o.shape == p.shape and np.isfinite(o).all() for o, p in zip(off, per_file))
    # Bit-equality with the switch off.  With it off convert_files runs the parent's statements only, so what this compares is the group
    # against the per-file Pipeline.pipeline, as test_gpu_dropin.py's convert_files test does -- and in that test's setting: its geometry, its
    # pinned kernel families and the skeleton's estimator, whose salience is a seeded function of the frame count alone.  The torch stand-in
    # above is a real half-precision network on torch's own convolutions; nothing in this suite pins those to the same bits from one run of
    # a shape to the next, so an equality on it would test torch, not the routing.
    d, seed, pl, pipe, net_g, tail = _webui_pipe(gpu, tmp_path)
    for key, val in (("RB_STREAM", 0), ("NO_RB_SPLIT", 1)):
        net_g.dec.set_option(key, val)
    for key, val in (("FR_NJ", 1), ("FR_FFN_SPLIT", 1), ("FR_WN_SPLIT", 1)):
        net_g._rvcmi_front.set_option(key, val)
    audios = [synth.make_audio16k(16000 * 2 + 77, seed + 1), synth.make_audio16k(16000, seed + 3), synth.make_audio16k(50000, seed + 4)]
    off = convert(audios)
    assert batches == [] and calls == [] and pipe.f0_gen.rmvpe.model.calls == 3
    torch.manual_seed(5)
    alone = [pipe.pipeline(hub, net_g, int(d["sid"]), a.copy(), [0, 0, 0], *tail) for a in audios]
    for i, (o, a) in enumerate(zip(off, alone)):
        assert o.shape == a.shape and np.array_equal(o, a), "file %d: with the switch off the group differs from the per-file pipeline" % i
