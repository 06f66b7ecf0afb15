"""Host side of the realtime GUI block (rvc_amd.RealtimeStream): the block geometry of gui.py:783-855 and the input gate of
gui.py:950-963, both of which need no device."""
import numpy as np
import pytest

# (samplerate, block_time, crossfade_time, extra_time) -> zc, block_frame, block_frame_16k, crossfade_frame, sola_buffer_frame,
# sola_search_frame, extra_frame, skip_head, return_length, len(input_wav), len(input_wav_res)   (gui.py:783-840)
GEOMETRY = [
    (32000, 0.25, 0.05, 2.5, 320, 8000, 4000, 1600, 1280, 320, 80000, 250, 30, 89920, 44960),
    (32000, 0.25, 0.05, 0.5, 320, 8000, 4000, 1600, 1280, 320, 16000, 50, 30, 25920, 12960),
    (32000, 0.25, 0.03, 2.5, 320, 8000, 4000, 960, 960, 320, 80000, 250, 29, 89280, 44640),
    (32000, 0.25, 0.03, 0.5, 320, 8000, 4000, 960, 960, 320, 16000, 50, 29, 25280, 12640),
    (32000, 0.1, 0.05, 2.5, 320, 3200, 1600, 1600, 1280, 320, 80000, 250, 15, 85120, 42560),
    (32000, 0.1, 0.05, 0.5, 320, 3200, 1600, 1600, 1280, 320, 16000, 50, 15, 21120, 10560),
    (32000, 0.1, 0.03, 2.5, 320, 3200, 1600, 960, 960, 320, 80000, 250, 14, 84480, 42240),
    (32000, 0.1, 0.03, 0.5, 320, 3200, 1600, 960, 960, 320, 16000, 50, 14, 20480, 10240),
    (40000, 0.25, 0.05, 2.5, 400, 10000, 4000, 2000, 1600, 400, 100000, 250, 30, 112400, 44960),
    (40000, 0.25, 0.05, 0.5, 400, 10000, 4000, 2000, 1600, 400, 20000, 50, 30, 32400, 12960),
    (40000, 0.25, 0.03, 2.5, 400, 10000, 4000, 1200, 1200, 400, 100000, 250, 29, 111600, 44640),
    (40000, 0.25, 0.03, 0.5, 400, 10000, 4000, 1200, 1200, 400, 20000, 50, 29, 31600, 12640),
    (40000, 0.1, 0.05, 2.5, 400, 4000, 1600, 2000, 1600, 400, 100000, 250, 15, 106400, 42560),
    (40000, 0.1, 0.05, 0.5, 400, 4000, 1600, 2000, 1600, 400, 20000, 50, 15, 26400, 10560),
    (40000, 0.1, 0.03, 2.5, 400, 4000, 1600, 1200, 1200, 400, 100000, 250, 14, 105600, 42240),
    (40000, 0.1, 0.03, 0.5, 400, 4000, 1600, 1200, 1200, 400, 20000, 50, 14, 25600, 10240),
    (44100, 0.25, 0.05, 2.5, 441, 11025, 4000, 2205, 1764, 441, 110250, 250, 30, 123921, 44960),
    (44100, 0.25, 0.05, 0.5, 441, 11025, 4000, 2205, 1764, 441, 22050, 50, 30, 35721, 12960),
    (44100, 0.25, 0.03, 2.5, 441, 11025, 4000, 1323, 1323, 441, 110250, 250, 29, 123039, 44640),
    (44100, 0.25, 0.03, 0.5, 441, 11025, 4000, 1323, 1323, 441, 22050, 50, 29, 34839, 12640),
    (44100, 0.1, 0.05, 2.5, 441, 4410, 1600, 2205, 1764, 441, 110250, 250, 15, 117306, 42560),
    (44100, 0.1, 0.05, 0.5, 441, 4410, 1600, 2205, 1764, 441, 22050, 50, 15, 29106, 10560),
    (44100, 0.1, 0.03, 2.5, 441, 4410, 1600, 1323, 1323, 441, 110250, 250, 14, 116424, 42240),
    (44100, 0.1, 0.03, 0.5, 441, 4410, 1600, 1323, 1323, 441, 22050, 50, 14, 28224, 10240),
    (48000, 0.25, 0.05, 2.5, 480, 12000, 4000, 2400, 1920, 480, 120000, 250, 30, 134880, 44960),
    (48000, 0.25, 0.05, 0.5, 480, 12000, 4000, 2400, 1920, 480, 24000, 50, 30, 38880, 12960),
    (48000, 0.25, 0.03, 2.5, 480, 12000, 4000, 1440, 1440, 480, 120000, 250, 29, 133920, 44640),
    (48000, 0.25, 0.03, 0.5, 480, 12000, 4000, 1440, 1440, 480, 24000, 50, 29, 37920, 12640),
    (48000, 0.1, 0.05, 2.5, 480, 4800, 1600, 2400, 1920, 480, 120000, 250, 15, 127680, 42560),
    (48000, 0.1, 0.05, 0.5, 480, 4800, 1600, 2400, 1920, 480, 24000, 50, 15, 31680, 10560),
    (48000, 0.1, 0.03, 2.5, 480, 4800, 1600, 1440, 1440, 480, 120000, 250, 14, 126720, 42240),
    (48000, 0.1, 0.03, 0.5, 480, 4800, 1600, 1440, 1440, 480, 24000, 50, 14, 30720, 10240),
]
KEYS = ("zc", "block_frame", "block_frame_16k", "crossfade_frame", "sola_buffer_frame", "sola_search_frame", "extra_frame", "skip_head",
        "return_length", "input_wav_len", "input_wav_res_len")


@pytest.mark.parametrize("row", GEOMETRY, ids=lambda r: "%d-%s-%s-%s" % r[:4])
def test_stream_geometry_matches_the_gui(row):
    from rvc_amd.realtime import stream_geometry

    g = stream_geometry(row[0], block_time=row[1], crossfade_time=row[2], extra_time=row[3])
    assert tuple(g[k] for k in KEYS) == row[4:]


def test_stream_needs_a_gpu_device():
    import types

    import rvc_amd

    with pytest.raises(rvc_amd.RvcmiError):
        rvc_amd.RealtimeStream(types.SimpleNamespace(tgt_sr=40000, infer=None), device="cpu")


def _gui_gate(indata, rms_buffer, zc, threhold):
    """gui.py:950-963 with librosa.feature.rms (centred, zero padded) and amplitude_to_db(ref=1.0, amin=1e-5, top_db=80) spelled out."""
    indata = np.append(rms_buffer, indata)
    padded = np.pad(indata, (2 * zc, 2 * zc))
    nfr = 1 + indata.shape[0] // zc
    rms = np.array([np.sqrt(np.float32(np.sum(padded[i * zc: i * zc + 4 * zc].astype(np.float64) ** 2) / (4 * zc))) for i in range(nfr)],
                   dtype=np.float32)[2:]
    rms_buffer[:] = indata[-4 * zc:]
    indata = indata[2 * zc - zc // 2:]
    db = 10.0 * np.log10(np.maximum(np.float32(1e-10), rms.astype(np.float32) ** 2))
    db = np.maximum(db, db.max() - 80.0)
    for i in range(db.shape[0]):
        if db[i] < threhold:
            indata[i * zc: (i + 1) * zc] = 0
    return indata[zc // 2:]


@pytest.mark.parametrize("threhold", [-55, -40, -20])
def test_input_gate_matches_the_gui(threhold):
    from rvc_amd.realtime import input_gate

    zc, blk = 400, 4000
    rng = np.random.default_rng(7)
    ours, gui = np.zeros(4 * zc, np.float32), np.zeros(4 * zc, np.float32)
    gated_somewhere = False
    for j, (amp_loud, amp_quiet) in enumerate(((0.3, 3e-4), (30.0, 3e-4), (0.05, 0.01), (0.0, 0.0))):
        x = (amp_loud * rng.standard_normal(blk)).astype(np.float32)
        x[800:3200] *= amp_quiet / max(amp_loud, 1e-30)   # a quiet stretch: three frames lie wholly inside it
        got = input_gate(x, ours, zc, threhold)
        want = _gui_gate(x.copy(), gui, zc, threhold)
        assert got.shape == (blk + 2 * zc,)                 # the GUI writes block + 2 zc samples into input_wav
        assert np.array_equal(got, want), j
        assert np.array_equal(ours, gui)
        gated_somewhere |= bool((got[2 * zc:] == 0).any() and (x != 0).all())
    assert gated_somewhere


def test_input_gate_top_db_clip():
    """With a frame at +29.5 dB, the 80 dB clip lifts a -70 dB frame to -50.5 dB, above a -55 dB gate: it is kept."""
    from rvc_amd.realtime import amplitude_to_db, input_gate

    zc, blk = 400, 4000
    x = np.full(blk, 30.0, np.float32)
    x[1200:3200] = 3e-4
    got = input_gate(x, np.zeros(4 * zc, np.float32), zc, -55)
    assert np.array_equal(got[2 * zc:], x)  # nothing gated
    db = amplitude_to_db(np.array([30.0, 3e-4], np.float32))
    assert db[1] == pytest.approx(db[0] - 80.0)
    got = input_gate(x / np.float32(30.0), np.zeros(4 * zc, np.float32), zc, -55)  # 0 dB max: the clip is at -80
    assert (got[2 * zc:][1800:2600] == 0).all() and np.array_equal(got[2 * zc:][:1000], x[:1000] / np.float32(30.0))


def test_stream_geometry_needs_no_torch_device():
    from rvc_amd.realtime import stream_geometry

    g = stream_geometry(40000)
    assert (g["zc"], g["block_frame"], g["sola_buffer_frame"], g["return_length"]) == (400, 10000, 1600, 30)
