"""The ragged f0 decode (``rvcmi_glue_rmvpe_f0_ragged`` / ``glue.rmvpe_f0_ragged``): the decode chain of many sequences in two
launches, every item bit-equal to ``glue.rmvpe_f0`` on its rows alone.

1. every small voiced / unvoiced pattern and the decode's edge rows as the items of one call; 2. the two homes of the work arrays (LDS,
global) with canaries around every output slice; 3. what is refused, before anything is launched; 4. ``RMVPEHIP.f0_batch`` with a key per
waveform, and the one batched mel launch of equal-length sequences."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import glue_cases as gcs
import rmvpe_cases as rc

pytestmark = pytest.mark.gpu

CANARY_P, CANARY_F = -7, -7.5


def _pack(items, gpu, gap_every=3):
    """items: (salience [n, 360] numpy, p_len, key) -> (packed salience on the device with a gap row of 0.7s after every ``gap_every``-th item,
    rows for rmvpe_f0_ragged)."""
    parts, rows, r = [], [], 0
    for i, (sal, p, k) in enumerate(items):
        parts.append(np.asarray(sal, np.float32))
        rows.append((r, int(sal.shape[0]), int(p), k))
        r += int(sal.shape[0])
        if i % gap_every == gap_every - 1:
            parts.append(np.full((1, 360), 0.7, np.float32))
            r += 1
    return torch.from_numpy(np.concatenate(parts)).to(gpu), rows


def _solo(packed, row):
    import rvc_amd

    r, n, p, k = row
    return rvc_amd.glue.rmvpe_f0(packed[r: r + n].clone(), p, k)


EXTRA_KEYS = (0.25, 3, -12)   # for the additional items: a fractional key, and integral ones on either side of the cases' own


def _meets_oracle(got_p, got_f, want_p, want_f):
    """The bars of tests/test_gpu_glue_edges.py: pitch identical, pitchf 1e-6 relative with equal zero sets."""
    return (np.array_equal(got_p, want_p) and np.array_equal(got_f == 0, want_f == 0) and np.allclose(got_f, want_f, rtol=gcs.F0_RTOL, atol=0))


def test_every_small_pattern_as_items_of_one_call(gpu):
    """All 254 patterns of 1 .. 7 frames x their p_lens x keys 0 / -5.5 -- every case of ``rmvpe_pattern_cases`` with ITS OWN key -- as the
    items of ONE call; neighbours have different keys already (the key is the innermost loop of the cases).  Behind them come additional
    items, every seventh case again with another key (``EXTRA_KEYS``), and a gap row stands behind every third item.  Every item is
    bit-equal to the solo call on its rows alone AND meets the oracle: the precomputed ``rmvpe_pattern_oracle()`` for the cases, at the
    bars of tests/test_gpu_glue_edges.py; ``oracle_rmvpe_f0`` for the additional items, where the margins of glue_cases hold (as
    ``test_decode_edge_rows_as_items`` does; most do, which is asserted)."""
    import rvc_amd

    cases = gcs.rmvpe_pattern_cases()
    oracle = gcs.rmvpe_pattern_oracle()
    extra = [(n, m, p, EXTRA_KEYS[j % len(EXTRA_KEYS)]) for j, (n, m, p, _) in enumerate(cases[::7])]
    every = list(cases) + extra
    assert all(a[3] != b[3] for a, b in zip(cases[::2], cases[1::2]))    # neighbours: keys 0 and -5.5
    packed, rows = _pack([(gcs.pattern_salience(n, m), p, k) for n, m, p, k in every], gpu)
    assert [r[3] for r in rows[: len(cases)]] == [c[3] for c in cases]   # every case runs with the key it names
    got = rvc_amd.glue.rmvpe_f0_ragged(packed, rows)
    assert len(got) == len(every) and len(cases) > 3000 and len(extra) > 400
    base = got[0][0].untyped_storage().data_ptr()
    assert all(g[0].untyped_storage().data_ptr() == base for g in got)   # views of one packed tensor
    solo = [_solo(packed, row) for row in rows]                           # every item's solo call on its rows alone
    sizes = [row[2] for row in rows]
    eq_p = torch.cat([g[0][0] for g in got]) == torch.cat([s[0][0] for s in solo])
    gf, sf = torch.cat([g[1][0] for g in got]), torch.cat([s[1][0] for s in solo])
    eq_f = gf.view(torch.int32) == sf.view(torch.int32)                   # bit for bit
    bad = [i for i, (a, b) in enumerate(zip(torch.split(eq_p.cpu(), sizes), torch.split(eq_f.cpu(), sizes))) if not (bool(a.all()) and bool(b.all()))]
    assert not bad, "items that differ from their solo call: %s" % [(i, every[i], rows[i]) for i in bad[:5]]
    pitch_all = torch.split(torch.cat([g[0][0] for g in got]).cpu(), sizes)
    pitchf_all = torch.split(gf.cpu(), sizes)
    for i, (case, row) in enumerate(zip(cases, rows)):                    # every case against the precomputed oracle, unconditionally
        assert got[i][0].shape == (1, row[2]) and got[i][0].dtype == torch.int64 and got[i][1].dtype == torch.float32
        assert _meets_oracle(pitch_all[i].numpy(), pitchf_all[i].numpy(), *oracle[i]), (i, case)
    held = 0
    for i, (n, m, p, k) in enumerate(extra, start=len(cases)):            # every additional item against the oracle, margins guarded
        sal = gcs.pattern_salience(n, m)
        dec, mel, _, _ = gcs.chain_parts(sal, p, k)
        if gcs.mel_margin(mel[:p]) > gcs.MEL_MARGIN and gcs.hz_margin(dec) > gcs.HZ_MARGIN:
            wp, wpf = gcs.oracle_rmvpe_f0(sal, p, k)
            assert _meets_oracle(pitch_all[i].numpy(), pitchf_all[i].numpy(), np.asarray(wp)[:p], np.asarray(wpf)[:p]), (i, n, m, p, k)
            held += 1
    assert held > 0.9 * len(extra), (held, len(extra))


def test_decode_edge_rows_as_items(gpu):
    """The rows of ``decode_edge_salience`` (peaks at bins 0 / 3 / 356 / 359, ties inside and across lanes, all-equal and all-zero rows), each
    row an item of its own and the 13- and 11-frame blocks as two more, with keys of their own."""
    import rvc_amd

    sal = gcs.decode_edge_salience()
    items = [(sal[i: i + 1], 3, 0.5 * i - 2) for i in range(sal.shape[0])] + [(sal, 17, -5.5), (sal[:11], 11, 0)]
    packed, rows = _pack(items, gpu, gap_every=2)
    got = rvc_amd.glue.rmvpe_f0_ragged(packed, rows)
    for g, row, (s, p, k) in zip(got, rows, items):
        sp, spf = _solo(packed, row)
        assert torch.equal(g[0], sp) and torch.equal(g[1], spf), row
        wp, wpf = gcs.oracle_rmvpe_f0(np.asarray(s), p, k)
        dec, mel, _, _ = gcs.chain_parts(np.asarray(s), p, k)
        if gcs.mel_margin(mel[:p]) > gcs.MEL_MARGIN and gcs.hz_margin(dec) > gcs.HZ_MARGIN:
            assert np.array_equal(g[0][0].cpu().numpy(), np.asarray(wp)[:p]), row
            assert np.allclose(g[1][0].cpu().numpy(), np.asarray(wpf)[:p], rtol=gcs.F0_RTOL, atol=0), row


def _raw_call(gpu, packed, rows, out_len, gaps):
    """The C entry on canary-filled outputs: item i's output starts ``gaps[i]`` elements behind the previous item's end.  -> (code, pitch,
    pitchf, offsets)."""
    from rvc_amd import _lib

    L = _lib.lib()
    desc, off, offs = (_lib.F0Row * len(rows))(), 0, []
    for d, (r, n, p, k), g in zip(desc, rows, gaps):
        off += g
        d.out_off, d.key_mul, d.first_row, d.n, d.p_len = off, L.rvcmi_glue_f0_key_mul(float(k)), r, n, p
        offs.append(off)
        off += p
    desc_dev = torch.frombuffer(bytearray(bytes(desc)), dtype=torch.uint8).to(gpu)
    pitch = torch.full((out_len,), CANARY_P, device=gpu, dtype=torch.int64)
    pitchf = torch.full((out_len,), CANARY_F, device=gpu, dtype=torch.float32)
    scratch = torch.empty(packed.shape[0], device=gpu, dtype=torch.float64)
    with torch.cuda.device(gpu):
        code = L.rvcmi_glue_rmvpe_f0_ragged(_lib.ptr(packed), packed.shape[0], 360, len(rows), C.cast(desc, C.c_void_p), _lib.ptr(desc_dev), 0.03,
                                            _lib.ptr(scratch), _lib.ptr(pitch), _lib.ptr(pitchf), out_len, _lib.stream_ptr(gpu))
    torch.cuda.synchronize(gpu)
    return code, pitch, pitchf, offs


def _check_items_and_canaries(gpu, packed, rows, gaps, tail=5):
    out_len = sum(gaps) + sum(r[2] for r in rows) + tail
    code, pitch, pitchf, offs = _raw_call(gpu, packed, rows, out_len, gaps)
    assert code == 0
    written = torch.zeros(out_len, dtype=torch.bool, device=gpu)
    for row, o in zip(rows, offs):
        sp, spf = _solo(packed, row)
        assert torch.equal(pitch[o: o + row[2]], sp[0]) and torch.equal(pitchf[o: o + row[2]], spf[0]), row
        written[o: o + row[2]] = True
    assert int((~written).sum()) == sum(gaps) + tail
    assert bool((pitch[~written] == CANARY_P).all()) and bool((pitchf[~written] == CANARY_F).all())   # between the slices and behind the last


def test_work_arrays_in_lds(gpu):
    """Items of 5, 1 and 64 frames (dynamic LDS sized for the largest), p_len below, at and above n."""
    sal = gcs.threshold_salience()
    items = [(sal[100: 105], 9, 2), (sal[400: 401], 4, -5.5), (sal[1000: 1064], 33, 0)]
    packed, rows = _pack(items, gpu, gap_every=1)
    _check_items_and_canaries(gpu, packed, rows, gaps=[3, 0, 2])


@functools.lru_cache(maxsize=None)
def _threshold_packed():
    return torch.from_numpy(np.ascontiguousarray(gcs.threshold_salience()))


@pytest.mark.parametrize("which", [0, 1])
def test_work_arrays_at_the_lds_threshold(which, gpu):
    """The ``THRESHOLD_RMVPE`` pair of glue_cases (n + p_len = 20480: the last size in LDS; one more: global) together with a 3-frame item in
    one call: past 160 KiB EVERY item of the launch works in global memory (its scratch rows in place, its pitch slice as the r array), and
    each still equals its solo call."""
    n, p, k = gcs.THRESHOLD_RMVPE[which]
    big = _threshold_packed().to(gpu)
    small = torch.from_numpy(gcs.pattern_salience(3, 0b101)).to(gpu)
    packed = torch.cat((small, torch.full((2, 360), 0.7, device=gpu), big[:n]))
    rows = [(0, 3, 7, -5.5), (5, n, p, k)]
    _check_items_and_canaries(gpu, packed, rows, gaps=[1, 4])


def test_rejections_launch_nothing(gpu):
    from rvc_amd import _lib

    packed = torch.from_numpy(gcs.pattern_salience(7, 0b1011101)).to(gpu)
    good = [(0, 3, 5, 0), (3, 4, 6, 2)]
    assert _raw_call(gpu, packed, good, 16, [0, 0])[0] == 0
    bad = {
        "overlapping outputs": (good, 16, [0, -2]),
        "overlapping sources": ([(0, 4, 5, 0), (3, 4, 6, 2)], 16, [0, 0]),
        "a source past R": ([(0, 3, 5, 0), (3, 5, 6, 2)], 16, [0, 0]),
        "p_len = 0": ([(0, 3, 0, 0), (3, 4, 6, 2)], 16, [0, 0]),
        "n = 0": ([(0, 0, 5, 0), (3, 4, 6, 2)], 16, [0, 0]),
        "an output past the end": (good, 10, [0, 0]),
        "a key that is not finite": ([(0, 3, 5, float("inf")), (3, 4, 6, 2)], 16, [0, 0]),
        "a NaN key": ([(0, 3, 5, 0), (3, 4, 6, float("nan"))], 16, [0, 0]),
    }
    for what, (rows, out_len, gaps) in bad.items():
        code, pitch, pitchf, _ = _raw_call(gpu, packed, rows, out_len, gaps)
        assert code == _lib.ERR_INVALID, what
        assert bool((pitch == CANARY_P).all()) and bool((pitchf == CANARY_F).all()), what
    import rvc_amd

    with pytest.raises(_lib.RvcmiError) as e:
        rvc_amd.glue.rmvpe_f0_ragged(packed, [(0, 3, 5, float("-inf"))])
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.RvcmiError):
        rvc_amd.glue.rmvpe_f0_ragged(packed, [])


def test_descriptors_are_uploaded_once_per_tuple_of_rows(gpu):
    import rvc_amd

    packed = torch.from_numpy(gcs.pattern_salience(7, 0b1011101)).to(gpu)
    rows = [(0, 3, 5, 0.75), (3, 4, 6, 2)]
    first = rvc_amd.glue.rmvpe_f0_ragged(packed, rows)
    n = rvc_amd.glue.f0_rows_uploads
    again = rvc_amd.glue.rmvpe_f0_ragged(packed, list(rows))
    assert rvc_amd.glue.f0_rows_uploads == n
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(first, again))
    rvc_amd.glue.rmvpe_f0_ragged(packed, [(0, 3, 5, 0.75), (3, 4, 6, 2.5)])
    assert rvc_amd.glue.f0_rows_uploads == n + 1


def test_f0_gather_defers_the_per_sequence_calls_into_one_ragged_call(gpu):
    """Inside ``glue._f0_gather`` (private to the package: ``rvc_infer_batch_hip``) a ``glue.rmvpe_f0`` call on rows of the packed salience launches nothing and returns views that the end of
    the block fills with the bits of the call alone; a call on any other tensor runs at once; nothing stays open after an exception."""
    import rvc_amd

    glue = rvc_amd.glue
    sal = gcs.decode_edge_salience()
    packed = torch.from_numpy(np.concatenate((sal, np.full((1, 360), 0.7, np.float32), sal[:11]))).to(gpu)
    items = [(0, 13, 17, -5.5), (14, 11, 11, 0)]
    solo = [glue.rmvpe_f0(packed[r: r + n].clone(), p, k) for r, n, p, k in items]
    other = packed[:5].clone()
    _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)   # (the profiler's own start-up)
    got = []

    def block(count_inside):
        with glue._f0_gather(packed, 28) as g:
            ask = lambda: got.extend([glue.rmvpe_f0(packed[r: r + n], p, k) for r, n, p, k in items])  # noqa: E731
            inside = _launches(ask, gpu) if count_inside else ask()
            got.append(glue.rmvpe_f0(other, 5, 2))               # not rows of the packed salience: decoded at once
            assert len(g.rows) == 2
        return g, inside

    g, inside = block(True)
    assert inside == []                                           # the gathered calls launched nothing
    whole = _launches(lambda: block(False), gpu)
    assert sum("k_f0_post_ragged" in k for k in whole) == 1 and sum("k_rmvpe_decode" in k for k in whole) == 2
    assert sum("k_f0_post" in k and "ragged" not in k for k in whole) == 1    # (the one call that was not gathered)
    for (p, pf), (sp, spf) in zip(got[:2], solo):
        assert torch.equal(p, sp) and torch.equal(pf, spf)
    assert torch.equal(g.pitch, torch.cat([s[0][0] for s in solo])) and g.pitch.shape == (28,)
    wp, wpf = glue.rmvpe_f0(other, 5, 2)
    assert torch.equal(got[2][0], wp) and torch.equal(got[2][1], wpf)
    with pytest.raises(ValueError):
        with glue._f0_gather(packed, 10):
            glue.rmvpe_f0(packed[:13], 17, 0)                    # more frames than were announced
    assert glue._F0_GATHER.blocks == []
    again = glue.rmvpe_f0(packed[:13], 17, -5.5)                 # outside a block: the call alone, as ever
    assert torch.equal(again[0], solo[0][0]) and torch.equal(again[1], solo[0][1])


# ---- RMVPEHIP ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _hip():
    import rvc_amd

    hip = rvc_amd.RMVPEHIP.from_reference(rc.RmvpeStandIn(torch.device("cuda:0"), True))
    assert hip is not None
    return hip


def _wavs(lengths, gpu):
    return [(rc.signal("voiced", n, 10 * i) + 0.3 * rc.signal("noise", n, 10 * i + 1)).to(gpu) for i, n in enumerate(lengths)]


def test_f0_batch_with_a_key_per_waveform_equals_the_loop_it_replaces(gpu):
    import rvc_amd

    hip = _hip()
    wavs, p_lens, keys = _wavs((5120, 513, 5037), gpu), [33, 9, 40], [0, -5.5, 3]
    got = hip.f0_batch(wavs, p_lens, keys)
    sal, off, frames = hip._salience_ragged(hip._wavs(wavs))
    for g, o, t, p, k in zip(got, off, frames, p_lens, keys):
        wp, wpf = rvc_amd.glue.rmvpe_f0(sal[o: o + t], p, k)
        assert torch.equal(g[0], wp) and torch.equal(g[1], wpf)
    one = hip.f0_batch(wavs, p_lens, -5.5)
    assert torch.equal(one[1][0], got[1][0]) and torch.equal(one[1][1], got[1][1])
    with pytest.raises(rvc_amd._lib.RvcmiError):
        hip.f0_batch(wavs, p_lens, [0, 1])


def _launches(fn, gpu):
    """Kernels and device-to-device copies ``fn`` enqueues, by torch.profiler (as tests/test_gpu_rt_formant.py counts them)."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize(gpu)
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize(gpu)
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return sorted(n for n in names if "memset" not in n.lower() and not ("memcpy" in n.lower() and "dtod" not in n.lower()))


def test_equal_lengths_take_one_mel_launch_and_the_same_rows(gpu):
    """Three waveforms of one length: the packed salience equals what the per-sequence mel loop gives (the loop is kept for unequal lengths
    and is taken here by the members one at a time: a batch of one has nothing to stack), and ``salience_batch`` issues the same number of
    launches for 2 and 3 waveforms."""
    from rvc_amd import _lib
    from rvc_amd.rmvpe import N_MELS

    hip = _hip()
    wavs = _wavs((5037, 5037, 5037), gpu)
    xs = hip._wavs(wavs)
    sal, off, frames = hip._salience_ragged(xs)
    assert off == [0, 32, 64, 96] and frames == [32, 32, 32]
    # the per-sequence mel loop, restated: each sequence's mel into its own rows of the packed buffer
    mel_loop = torch.empty(96, N_MELS, device=gpu)
    mel_one = torch.empty(96, N_MELS, device=gpu)
    L, st = _lib.lib(), _lib.stream_ptr(gpu)
    with torch.cuda.device(gpu):
        for i, x in enumerate(xs):
            _lib.check(L.rvcmi_mel_forward(hip._h, 1, 5037, _lib.ptr(x), 1 if hip.is_half else 0, 32, C.c_void_p(mel_loop.data_ptr() + 4 * N_MELS * 32 * i), st))
        _lib.check(L.rvcmi_mel_forward(hip._h, 3, 5037, _lib.ptr(torch.cat(xs)), 1 if hip.is_half else 0, 32, _lib.ptr(mel_one), st))
    assert torch.equal(mel_one, mel_loop)
    # ... and through the whole network: a length that differs by one sample keeps the loop (same frame counts, same packed layout)
    mixed = hip._salience_ragged(hip._wavs([wavs[0], wavs[1], torch.cat((wavs[2], wavs[2][-1:]))]))[0]
    assert torch.equal(sal[:64], mixed[:64])
    _launches(lambda: torch.zeros(4, device=gpu).add_(1), gpu)   # (the profiler's own start-up)
    hip.salience_batch(wavs[:2])
    two = _launches(lambda: hip.salience_batch(wavs[:2]), gpu)
    three = _launches(lambda: hip.salience_batch(wavs), gpu)
    assert len(two) == len(three) > 10, (len(two), len(three))
    assert sum("k_rmvpe_logmel" in k for k in three) == 1
