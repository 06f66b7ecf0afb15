"""Fixtures of the realtime GUI block (gui.py:27-49, 934-1090) -> tests/golden/gui_phase_vocoder.npz, gui_stream_<case>.npz.

Only ``phase_vocoder`` is taken from the reference's gui.py (``ast`` extraction + ``exec`` with ``torch`` / ``np`` in the namespace,
as oracle/make_golden.glue_case does).  Inside that namespace ``torch.fft.rfft`` returns ``rfft(x) + 0.0``, which maps the
FFT backend's ``-0.0`` to ``+0.0`` and changes nothing else: an exactly-zero bin then has phase 0, the convention the device
follows.  ``ref64_raw`` keeps the unwrapped function's output for the zero-``a`` case as a record of the
divergence.  Everything else here is the project's own restatement of ``audio_infer`` (gui.py:934-1090 minus noise reduction),
with oracle.glue_oracle's ``frame_rms`` / ``sinc_resample`` for librosa's RMS and torchaudio's resampler (both unpinned).
Seeds are fixed: a rerun writes equal arrays.

    python tools/make_golden_gui.py          (needs the reference tree: RVC_REFERENCE, default as oracle/make_golden.py)
"""
import ast
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import glue_oracle  # noqa: E402
from oracle.make_golden import REF  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def load_phase_vocoder(wrap_rfft: bool = True):
    src = open(os.path.join(REF, "gui.py")).read()
    fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "phase_vocoder")
    code = ast.get_source_segment(src, fn)
    tmod = torch
    if wrap_rfft:
        class _Torch:
            fft = types.SimpleNamespace(rfft=lambda x, *a, **k: torch.fft.rfft(x, *a, **k) + 0.0)

            def __getattr__(self, name):
                return getattr(torch, name)

        tmod = _Torch()
    ns = {"torch": tmod, "np": np}
    exec(code, ns)
    return ns["phase_vocoder"]


def fade_windows(n: int):
    """gui.py:841-855 in fp32 on the CPU."""
    fade_in = torch.sin(0.5 * np.pi * torch.linspace(0.0, 1.0, steps=n, dtype=torch.float32)) ** 2
    return fade_in, 1 - fade_in


def voice(n: int, sr: int, rng, f0: float, noise: float) -> np.ndarray:
    t = np.arange(n) / sr
    ph = 2 * np.pi * f0 * (t + 0.002 * np.sin(2 * np.pi * 3.0 * t))
    x = sum((0.3 / h) * np.sin(h * ph + 0.7 * h) for h in range(1, 9))
    return (x + noise * rng.standard_normal(n)).astype(np.float32)


def wrapped_d_margin(a, b, fo, fi) -> float:
    """Distance of d / 2 pi + 0.5 from the nearest integer over all bins (fp64): how far every bin is from the wrap."""
    w = np.sqrt(fo.astype(np.float64) * fi.astype(np.float64))
    fa, fb = np.fft.rfft(a * w), np.fft.rfft(b * w)
    pa = np.where(np.abs(fa) == 0, 0.0, np.angle(fa))
    pb = np.where(np.abs(fb) == 0, 0.0, np.angle(fb))
    u = (pb - pa) / 2 / np.pi + 0.5
    return float(np.min(np.abs(u - np.round(u))))


# the sizes of the GUI's geometries, then the edges (tests/test_gpu_glue_edges.py): windows that are all zero (n <= 2), odd / even Nyquist
# handling where one bin is a large share of them, the wave and block widths of the kernels +- 1, the size limit and one under it
PV_SIZES = ((1280, 32000), (1600, 40000), (1920, 48000), (1323, 44100))
PV_EDGE_SIZES = tuple((n, 48000) for n in (1, 2, 3, 4, 5, 63, 64, 65, 4095, 4096))


def pv_fixture():
    pv, pv_raw = load_phase_vocoder(True), load_phase_vocoder(False)
    out = {}
    for n, sr in PV_SIZES + PV_EDGE_SIZES:
        fi, fo = fade_windows(n)
        out["n%d_fade_in" % n], out["n%d_fade_out" % n] = fi.numpy(), fo.numpy()
        seed = n
        while True:
            rng = np.random.default_rng(seed)
            a = voice(n, sr, rng, 196.0, 0.05)
            b = voice(n, sr, rng, 203.0, 0.05)
            if wrapped_d_margin(a, b, fo.numpy(), fi.numpy()) > 1e-6 and wrapped_d_margin(np.zeros_like(a), b, fo.numpy(), fi.numpy()) > 1e-6:
                break
            seed += 1000
        for case, (ca, cb) in {"harm": (a, b), "zero_a": (np.zeros_like(a), b), "same": (a, a.copy())}.items():
            key = "n%d_%s" % (n, case)
            ta, tb = torch.from_numpy(ca), torch.from_numpy(cb)
            out[key + "_a"], out[key + "_b"] = ca, cb
            out[key + "_ref32"] = pv(ta, tb, fo, fi).numpy()
            out[key + "_ref64"] = pv(ta.double(), tb.double(), fo.double(), fi.double()).numpy()
            if case == "zero_a":
                out[key + "_ref64_raw"] = pv_raw(ta.double(), tb.double(), fo.double(), fi.double()).numpy()
    np.savez_compressed(os.path.join(GOLD, "gui_phase_vocoder.npz"), **out)
    for k in sorted(out):
        if k.endswith("_ref32"):
            r64 = out[k[:-6] + "_ref64"]
            print("%-22s ref32-ref64 rms %.2e max %.2e" % (k[:-6], np.sqrt(np.mean((out[k] - r64) ** 2)), np.abs(out[k] - r64).max()))


# ---------------------------------------------------------------------------------------------------------------------------
# audio_infer (gui.py:934-1090) restated on the CPU, noise reduction and the "im" mode left out
# ---------------------------------------------------------------------------------------------------------------------------
def amplitude_to_db(s):
    power = np.square(np.abs(s)).astype(np.float32)
    log_spec = (np.float32(10.0) * np.log10(np.maximum(np.float32(1e-10), power))).astype(np.float32)
    return np.maximum(log_spec, log_spec.max() - np.float32(80.0))


class GuiBlock:
    def __init__(self, samplerate, tgt_sr, block_time, crossfade_time, extra_time, threhold, rms_mix_rate, use_pv, pv):
        self.sr, self.tgt_sr, self.threhold, self.rate, self.use_pv, self.pv = samplerate, tgt_sr, threhold, rms_mix_rate, use_pv, pv
        self.zc = zc = samplerate // 100
        self.block_frame = int(np.round(block_time * samplerate / zc)) * zc
        self.block_frame_16k = 160 * self.block_frame // zc
        self.crossfade_frame = int(np.round(crossfade_time * samplerate / zc)) * zc
        self.sola_buffer_frame = min(self.crossfade_frame, 4 * zc)
        self.sola_search_frame = zc
        self.extra_frame = int(np.round(extra_time * samplerate / zc)) * zc
        self.input_wav = torch.zeros(self.extra_frame + self.crossfade_frame + self.sola_search_frame + self.block_frame)
        self.input_wav_res = torch.zeros(160 * self.input_wav.shape[0] // zc)
        self.rms_buffer = np.zeros(4 * zc, dtype="float32")
        self.sola_buffer = torch.zeros(self.sola_buffer_frame)
        self.skip_head = self.extra_frame // zc
        self.return_length = (self.block_frame + self.sola_buffer_frame + self.sola_search_frame) // zc
        self.fade_in_window, self.fade_out_window = fade_windows(self.sola_buffer_frame)

    def step(self, indata, infer):
        zc = self.zc
        indata = np.asarray(indata, np.float32)
        if indata.ndim == 2:
            indata = np.mean(indata.T, axis=0)
        if self.threhold > -60:
            indata = np.append(self.rms_buffer, indata)
            rms = glue_oracle.frame_rms(indata, 4 * zc, zc)[2:]
            self.rms_buffer[:] = indata[-4 * zc:]
            indata = indata[2 * zc - zc // 2:]
            db_threhold = amplitude_to_db(rms) < self.threhold
            for i in range(db_threhold.shape[0]):
                if db_threhold[i]:
                    indata[i * zc: (i + 1) * zc] = 0
            indata = indata[zc // 2:]
        self.input_wav[: -self.block_frame] = self.input_wav[self.block_frame:].clone()
        self.input_wav[-indata.shape[0]:] = torch.from_numpy(indata)
        self.input_wav_res[: -self.block_frame_16k] = self.input_wav_res[self.block_frame_16k:].clone()
        res = glue_oracle.sinc_resample(self.input_wav[-indata.shape[0] - 2 * zc:].numpy(), self.sr, 16000)
        self.input_wav_res[-160 * (indata.shape[0] // zc + 1):] = torch.from_numpy(res)[160:]
        res_in = self.input_wav_res.clone()
        infer_wav = torch.from_numpy(infer(res_in)).clone()
        if self.tgt_sr != self.sr:
            infer_wav = torch.from_numpy(glue_oracle.sinc_resample(infer_wav.numpy(), self.tgt_sr, self.sr))
        if self.rate < 1:
            input_wav = self.input_wav[self.extra_frame:]
            rms1 = torch.from_numpy(glue_oracle.frame_rms(input_wav[: infer_wav.shape[0]].numpy(), 4 * zc, zc)[None])
            rms1 = F.interpolate(rms1.unsqueeze(0), size=infer_wav.shape[0] + 1, mode="linear", align_corners=True)[0, 0, :-1]
            rms2 = torch.from_numpy(glue_oracle.frame_rms(infer_wav.numpy(), 4 * zc, zc)[None])
            rms2 = F.interpolate(rms2.unsqueeze(0), size=infer_wav.shape[0] + 1, mode="linear", align_corners=True)[0, 0, :-1]
            rms2 = torch.max(rms2, torch.zeros_like(rms2) + 1e-3)
            infer_wav *= torch.pow(rms1 / rms2, torch.tensor(1 - self.rate))
        Lb, Ls = self.sola_buffer_frame, self.sola_search_frame
        conv_input = infer_wav[None, None, : Lb + Ls]
        cor_nom = F.conv1d(conv_input, self.sola_buffer[None, None, :])
        cor_den = torch.sqrt(F.conv1d(conv_input ** 2, torch.ones(1, 1, Lb)) + 1e-8)
        ratio = cor_nom[0, 0] / cor_den[0, 0]
        sola_offset = int(torch.argmax(ratio))
        if bool((self.sola_buffer != 0).any()):  # block 0 (zero buffer): every ratio is 0 and argmax takes the first
            top = torch.sort(ratio, descending=True).values
            margin = float((top[0] - top[1]) / top[0].abs())
            if margin < 1e-4:
                raise RuntimeError("SOLA argmax margin %.2e below 1e-4" % margin)
        infer_wav = infer_wav[sola_offset:]
        if not self.use_pv:
            infer_wav[:Lb] *= self.fade_in_window
            infer_wav[:Lb] += self.sola_buffer * self.fade_out_window
        else:
            infer_wav[:Lb] = self.pv(self.sola_buffer, infer_wav[:Lb], self.fade_out_window, self.fade_in_window)
        self.sola_buffer[:] = infer_wav[self.block_frame: self.block_frame + Lb]
        return res_in.numpy(), sola_offset, infer_wav[: self.block_frame].clone().numpy()


STREAM_CASES = {
    "pv40k": dict(samplerate=40000, tgt_sr=40000, crossfade_time=0.05, threhold=-60, rms_mix_rate=0.0, use_pv=True, channels=1),
    "mix48k": dict(samplerate=48000, tgt_sr=40000, crossfade_time=0.05, threhold=-40, rms_mix_rate=0.25, use_pv=False, channels=2),
    "pv44k": dict(samplerate=44100, tgt_sr=48000, crossfade_time=0.03, threhold=-50, rms_mix_rate=1.0, use_pv=True, channels=1),
}
BLOCK_TIME, EXTRA_TIME, K = 0.1, 0.5, 4


def stream_fixture(name, c, pv, seed):
    g = GuiBlock(c["samplerate"], c["tgt_sr"], BLOCK_TIME, c["crossfade_time"], EXTRA_TIME, c["threhold"], c["rms_mix_rate"], c["use_pv"], pv)
    rng = np.random.default_rng(seed)
    sr, tsr, blk = c["samplerate"], c["tgt_sr"], g.block_frame
    # host input: a tone with noise, quiet stretches (-66 dB) for the gate
    n_all = K * blk
    x = voice(n_all, sr, rng, 150.0, 0.02)
    x[int(0.3 * blk): int(0.7 * blk)] *= 0.001
    x[int(2.2 * blk): int(2.5 * blk)] *= 0.001
    blocks = [np.stack([x[j * blk: (j + 1) * blk], 0.5 * x[j * blk: (j + 1) * blk]], 1) if c["channels"] == 2 else x[j * blk: (j + 1) * blk]
              for j in range(K)]
    # the stub's output: windows of one long "voice" at tgt_sr, each block advanced by a block with some jitter, so SOLA has a
    # true offset to find; quiet stretches for the envelope mix's 1e-3 floor
    n_chunk = g.return_length * tsr // 100
    blk_t = blk * tsr // sr
    v = voice(K * blk_t + n_chunk + 1000, tsr, rng, 210.0, 0.1)
    v[int(1.5 * blk_t): int(1.8 * blk_t)] *= 1e-4
    jitter = rng.integers(0, g.sola_search_frame * tsr // sr, size=K)
    chunks = [v[j * blk_t + jitter[j]: j * blk_t + jitter[j] + n_chunk].copy() for j in range(K)]
    res, offs, outs = [], [], []
    for j in range(K):
        r, o, y = g.step(blocks[j], lambda _res, j=j: chunks[j])
        res.append(r)
        offs.append(o)
        outs.append(y)
    np.savez_compressed(os.path.join(GOLD, "gui_stream_%s.npz" % name), indata=np.stack(blocks), chunks=np.stack(chunks),
                        input_wav_res=np.stack(res), offsets=np.array(offs, np.int64), out=np.stack(outs),
                        samplerate=sr, tgt_sr=tsr, block_time=BLOCK_TIME, crossfade_time=c["crossfade_time"], extra_time=EXTRA_TIME,
                        threhold=c["threhold"], rms_mix_rate=c["rms_mix_rate"], use_pv=c["use_pv"], skip_head=g.skip_head,
                        return_length=g.return_length, block_frame_16k=g.block_frame_16k, seed=seed)
    print("gui_stream_%-8s offsets %s  (%d KB)" % (name, offs, os.path.getsize(os.path.join(GOLD, "gui_stream_%s.npz" % name)) // 1024))


def main():
    torch.set_num_threads(1)
    pv_fixture()
    pv = load_phase_vocoder(True)
    for i, (name, c) in enumerate(STREAM_CASES.items()):
        seed = 100 + i
        while True:
            try:
                stream_fixture(name, c, pv, seed)
                break
            except RuntimeError as e:
                print("gui_stream_%s seed %d: %s; next seed" % (name, seed, e))
                seed += 1000


if __name__ == "__main__":
    main()
