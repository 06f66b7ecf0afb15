"""Shared pieces of the RMVPE front-end tests (tests/test_cpu_rmvpe.py, tests/test_gpu_rmvpe.py) and of tools/rmvpe_time.py, tools/rmvpe_parity.py:

  * ``htk_bank``: an HTK-style triangular filter bank (30-8000 Hz at 16 kHz, 128 x 513, Slaney-normalised, what ``librosa.filters.mel(htk=True)``
    builds for rvc/f0/mel.py:27-35) with a seeded per-row gain, and ``dense_bank``: a seeded non-negative matrix with no band structure;
  * ``signal``: the test signals (voiced harmonics 60 dB above their neighbours with an exactly-zero gap, a pure tone, white noise, noise that
    straddles the clamp);
  * ``log_mel``: rvc/f0/mel.py:58-71 (keyshift 0, speed 1, center=True) over rvc/f0/stft.py:165-180 restated in torch, in whatever dtype is
    asked for: fp64 it is the oracle, fp32 it is what the reference executes;
  * ``MelStandIn`` / ``E2EStandIn`` / ``RmvpeStandIn``: objects with the attributes, state-dict keys and call protocol of the reference's
    ``MelSpectrogram``, ``E2E`` and ``RMVPE`` (rvc/f0/mel.py needs librosa, which is not installable; the network is the generic tree of
    tests/unet_cases.py with the ``fc`` of rvc/f0/e2e.py:31-35 behind it).
"""
import numpy as np
import torch
import torch.nn.functional as F

import unet_cases as uc

SR, N_FFT, HOP, N_MELS, CLAMP = 16000, 1024, 160, 128, 1e-5
LENGTHS = (513, 5037, 5120, 48077)  # 4, 32, 33 and 301 frames


def htk_bank(seed=0, fmin=30.0, fmax=8000.0):
    def hz2mel(f):
        return 2595.0 * np.log10(1.0 + f / 700.0)

    def mel2hz(m):
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)

    freqs = np.linspace(0, SR / 2, N_FFT // 2 + 1)
    pts = mel2hz(np.linspace(hz2mel(fmin), hz2mel(fmax), N_MELS + 2))
    d = np.diff(pts)
    ramps = pts[:, None] - freqs[None]
    w = np.zeros((N_MELS, N_FFT // 2 + 1))
    for i in range(N_MELS):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / d[i], ramps[i + 2] / d[i + 1]))
    w *= (2.0 / (pts[2:] - pts[:-2]))[:, None]
    if seed is not None:
        w *= np.random.default_rng(seed).uniform(0.9, 1.1, (N_MELS, 1))
    return torch.from_numpy(w.astype(np.float32))


def dense_bank(seed=1):
    return torch.rand(N_MELS, N_FFT // 2 + 1, generator=torch.Generator().manual_seed(seed)) / 300.0


def signal(kind, n, seed=0):
    """-> float32 [n]"""
    g = torch.Generator().manual_seed(seed + n)
    t = torch.arange(n, dtype=torch.float64) / SR
    if kind == "voiced":
        f0 = 120 + 40 * torch.sin(2 * np.pi * 0.7 * t)
        ph = 2 * np.pi * torch.cumsum(f0, 0) / SR
        x = sum(torch.sin(k * ph) / k for k in range(1, 30)) * 0.1 + 0.003 * torch.randn(n, dtype=torch.float64, generator=g)
        x[n // 3: n // 3 + 4000] = 0
    elif kind == "sine":
        x = 0.9 * torch.sin(2 * np.pi * 440 * t)
    elif kind == "noise":
        x = 0.1 * torch.randn(n, dtype=torch.float64, generator=g)
    elif kind == "quiet":
        x = 1e-4 * torch.randn(n, dtype=torch.float64, generator=g)
    else:
        raise ValueError(kind)
    return x.float()


def zero_frames(x):
    """Frames of the centred, reflect-padded STFT whose whole window is exactly zero.  x [n] -> bool [T]"""
    p = F.pad(x.abs()[None, None], (N_FFT // 2, N_FFT // 2), mode="reflect")[0, 0]
    return p.unfold(0, N_FFT, HOP).sum(-1) == 0


def log_mel(audio, basis, dtype, half, clamp=CLAMP):
    """[B, n] -> log-mel [B, 128, T] as rvc/f0/mel.py:58-71 computes it, evaluated in ``dtype`` (``half``: the ``is_half`` branch)."""
    audio = audio.to(dtype)
    fft = torch.stft(audio, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, window=torch.hann_window(N_FFT, dtype=dtype, device=audio.device),
                     center=True, return_complex=True)
    magnitude = torch.sqrt(fft.real.pow(2) + fft.imag.pow(2))
    mel_output = torch.matmul(basis.to(audio.device, dtype), magnitude)
    if half:
        mel_output = mel_output.half()
    return torch.log(torch.clamp(mel_output, min=clamp))


def padded_layout(logmel, T_pad):
    """[B, 128, T] -> [B, T_pad, 128] with zero frames behind (the ``F.pad`` of rvc/f0/rmvpe.py:141-144 and the transpose of e2e.py:44)."""
    return F.pad(logmel, (0, T_pad - logmel.shape[-1])).transpose(1, 2).contiguous()


def pad32(T):
    return 32 * ((T - 1) // 32 + 1)


def half_ulps(a, b):
    """Distance in fp16 steps between two tensors of fp16-representable values (any float dtype)."""
    def order(v):
        i = v.to(torch.float16).view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)

    return (order(a) - order(b)).abs()


class MelStandIn(torch.nn.Module):
    """The attributes and the forward of rvc/f0/mel.py's ``MelSpectrogram`` (the ``use_torch_stft`` branch)."""

    def __init__(self, is_half, basis=None, n_fft=N_FFT, hop_length=HOP, win_length=N_FFT, clamp=CLAMP):
        super().__init__()
        self.register_buffer("mel_basis", (htk_bank() if basis is None else basis).float())
        self.n_fft, self.hop_length, self.win_length, self.clamp, self.is_half = n_fft, hop_length, win_length, clamp, is_half
        self.calls = 0

    def forward(self, audio, keyshift=0, speed=1, center=True):
        assert keyshift == 0 and speed == 1 and center
        self.calls += 1
        fft = torch.stft(audio, n_fft=self.n_fft, hop_length=self.hop_length, win_length=self.win_length,
                         window=torch.hann_window(self.win_length, device=audio.device), center=True, return_complex=True)
        magnitude = torch.sqrt(fft.real.pow(2) + fft.imag.pow(2))
        mel_output = torch.matmul(self.mel_basis, magnitude)
        if self.is_half:
            mel_output = mel_output.half()
        return torch.log(torch.clamp(mel_output, min=self.clamp))


class _BiGRU(torch.nn.Module):
    def __init__(self, i, h):
        super().__init__()
        self.gru = torch.nn.GRU(i, h, num_layers=1, batch_first=True, bidirectional=True)

    def forward(self, x):
        return self.gru(x)[0]


class E2EStandIn(uc.StandIn):
    """``E2E(4, 1, (2, 2))`` of rvc/f0/e2e.py with seeded weights: the U-Net tree of tests/unet_cases.py (real ``torch.nn`` leaves) and the
    ``fc`` of e2e.py:31-35 under the reference's own state-dict names (``fc.0.gru.*``, ``fc.1.*``).  mel [B, 128, T] -> salience [B, T, 360]."""

    def __init__(self, seed=21, keys=None, gru_hidden=256, n_class=360):
        keys = keys or uc.golden_keys()
        super().__init__(keys, uc.seeded_weights(keys, seed), real_modules=True)
        torch.manual_seed(seed)
        self.fc = torch.nn.Sequential(_BiGRU(3 * N_MELS, gru_hidden), torch.nn.Linear(2 * gru_hidden, n_class), torch.nn.Dropout(0.25), torch.nn.Sigmoid())

    def forward(self, mel):
        return self.fc(super().forward(mel))


class RmvpeStandIn:
    """What ``rvc_amd`` reads of an ``rvc.f0.rmvpe.RMVPE`` instance: ``device``, ``is_half``, ``mel_extractor``, ``model`` and ``_mel2hidden``
    (rvc/f0/rmvpe.py:141-164)."""

    def __init__(self, device, is_half, seed=21, basis=None, model=None):
        self.device, self.is_half = device, is_half
        self.mel_extractor = MelStandIn(is_half, basis).to(device)
        self.model = (model if model is not None else E2EStandIn(seed)).eval().to(device)
        if is_half:
            self.model = self.model.half()
        self.hidden_calls = 0

    def _mel2hidden(self, mel):
        self.hidden_calls += 1
        with torch.no_grad():
            n_frames = mel.shape[-1]
            n_pad = 32 * ((n_frames - 1) // 32 + 1) - n_frames
            if n_pad > 0:
                mel = F.pad(mel, (0, n_pad), mode="constant")
            mel = mel.half() if self.is_half else mel.float()
            hidden = self.model(mel)
            return hidden[:, :n_frames]
