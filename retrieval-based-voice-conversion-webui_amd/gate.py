"""``TorchGate`` (infer/modules/gui/torchgate.py), the realtime GUI's noise reduction, on the device: the same constructor,
defaults, ``smoothing_filter`` buffer and ``forward(x, xn=None)``, computed by one ``glue.spectral_gate`` call (rvcmi.h).

    tg = TorchGateHIP(sr=48000, n_fft=4 * 480, prop_decrease=0.9).to("cuda:0")     # gui.py:869-871
    y = tg(x[None], xn[None])                                                        # gui.py:983-985, 1020-1022

Divergences from the reference: an odd ``n_fft`` raises ``RvcmiError`` (torch accepts it); a ``freq_mask_smooth_hz`` below one bin
raises the ``ValueError`` the reference means to raise (its message formats the missing ``self._n_fft``, so it raises
``AttributeError``, torchgate.py:94-96); the DirectML ``STFT`` branch is not reproduced (the input must be a ROCm tensor).  As
``torch.istft``, a window / hop pair whose overlap-added squared window falls below 1e-11 inside the kept range (``hop_length >
win_length``, or hann with ``hop_length = n_fft``) raises, here a ``ValueError`` from the host before anything is launched.
"""
from __future__ import annotations

from typing import Optional, Union

import torch

from . import _lib, glue


def _linspace(start, stop, num: int = 50, endpoint: bool = True) -> torch.Tensor:
    """utils.py:46-71"""
    if endpoint:
        return torch.linspace(start, stop, num)
    return torch.linspace(start, stop, num + 1)[:-1]


class TorchGateHIP(torch.nn.Module):
    @torch.no_grad()
    def __init__(self, sr: int, nonstationary: bool = False, n_std_thresh_stationary: float = 1.5, n_thresh_nonstationary: float = 1.3,
                 temp_coeff_nonstationary: float = 0.1, n_movemean_nonstationary: int = 20, prop_decrease: float = 1.0, n_fft: int = 1024,
                 win_length: bool = None, hop_length: int = None, freq_mask_smooth_hz: float = 500, time_mask_smooth_ms: float = 50):
        super().__init__()
        self.sr = sr
        self.nonstationary = nonstationary
        assert 0.0 <= prop_decrease <= 1.0
        self.prop_decrease = prop_decrease
        self.n_fft = n_fft
        self.win_length = self.n_fft if win_length is None else win_length
        self.hop_length = self.win_length // 4 if hop_length is None else hop_length
        self.n_std_thresh_stationary = n_std_thresh_stationary
        self.temp_coeff_nonstationary = temp_coeff_nonstationary
        self.n_movemean_nonstationary = n_movemean_nonstationary
        self.n_thresh_nonstationary = n_thresh_nonstationary
        self.freq_mask_smooth_hz = freq_mask_smooth_hz
        self.time_mask_smooth_ms = time_mask_smooth_ms
        self.register_buffer("smoothing_filter", self._generate_mask_smoothing_filter())
        self._windows = {}
        self._ola_checked = set()

    @torch.no_grad()
    def _generate_mask_smoothing_filter(self) -> Union[torch.Tensor, None]:
        """torchgate.py:75-127, in the default dtype as there."""
        if self.freq_mask_smooth_hz is None and self.time_mask_smooth_ms is None:
            return None
        n_grad_freq = 1 if self.freq_mask_smooth_hz is None else int(self.freq_mask_smooth_hz / (self.sr / (self.n_fft / 2)))
        if n_grad_freq < 1:
            raise ValueError(f"freq_mask_smooth_hz needs to be at least {int((self.sr / (self.n_fft / 2)))} Hz")
        n_grad_time = 1 if self.time_mask_smooth_ms is None else int(self.time_mask_smooth_ms / ((self.hop_length / self.sr) * 1000))
        if n_grad_time < 1:
            raise ValueError(f"time_mask_smooth_ms needs to be at least {int((self.hop_length / self.sr) * 1000)} ms")
        if n_grad_time == 1 and n_grad_freq == 1:
            return None
        v_f = torch.cat([_linspace(0, 1, n_grad_freq + 1, endpoint=False), _linspace(1, 0, n_grad_freq + 2)])[1:-1]
        v_t = torch.cat([_linspace(0, 1, n_grad_time + 1, endpoint=False), _linspace(1, 0, n_grad_time + 2)])[1:-1]
        smoothing_filter = torch.outer(v_f, v_t).unsqueeze(0).unsqueeze(0)
        return smoothing_filter / smoothing_filter.sum()

    def _window(self, dev: torch.device) -> torch.Tensor:
        """torch.stft's window: torch.hann_window(win_length) (periodic) zero-padded to n_fft at the centre, in fp64."""
        w = self._windows.get(dev)
        if w is None:
            if not 0 < self.win_length <= self.n_fft:
                raise ValueError("win_length = %d must be in [1, n_fft = %d]" % (self.win_length, self.n_fft))
            w = torch.zeros(self.n_fft, dtype=torch.float64)
            left = (self.n_fft - self.win_length) // 2
            w[left: left + self.win_length] = torch.hann_window(self.win_length, dtype=torch.float64)
            w = self._windows[dev] = w.to(dev)
        return w

    def _check_overlap_add(self, L: int) -> None:
        """torch.istft's check, on the host (no device read-back): the overlap-added squared window of the call's ``1 + L // hop``
        frames must stay above 1e-11 wherever the output is kept, or the division behind the overlap-add gives inf / NaN.  Away from
        both ends the sum has period ``hop_length``, so 2 ceil(n_fft / hop) + 2 frames stand for any larger number."""
        n, hop = self.n_fft, int(self.hop_length)
        if not 0 < hop <= n or n % 2:
            return  # the library refuses these with its own message
        frames = min(1 + L // hop, 2 * -(-n // hop) + 2)
        if frames in self._ola_checked:
            return
        w2 = self._window(torch.device("cpu")) ** 2
        env = torch.zeros(n + hop * (frames - 1), dtype=torch.float64)
        for f in range(frames):
            env[f * hop: f * hop + n] += w2
        kept = env[n // 2: n // 2 + hop * (frames - 1)]
        if kept.numel() and float(kept.min()) < 1e-11:
            raise ValueError("window overlap add min below 1e-11: hann_window(%d) centred in n_fft = %d with hop_length = %d leaves output "
                             "samples that no frame covers (torch.istft refuses this too)" % (self.win_length, n, hop))
        self._ola_checked.add(frames)

    @torch.no_grad()
    def forward(self, x: torch.Tensor, xn: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [B, L] or [L] (``xn`` shaped alike, or None: the noise statistics come from x) on the GPU -> the gated signal,
        ``hop_length * (L // hop_length)`` samples in x's dtype (computed from x rounded to float32)."""
        if x.device.type != "cuda" or (xn is not None and xn.device.type != "cuda"):
            raise _lib.RvcmiError("TorchGateHIP runs on the GPU (got %s); there is no CPU fallback" % x.device)
        squeeze = x.dim() == 1
        x32 = (x[None] if squeeze else x).to(torch.float32).contiguous()
        self._check_overlap_add(int(x32.shape[-1]))
        xn32 = None
        if xn is not None:
            xn32 = (xn[None] if xn.dim() == 1 else xn).to(torch.float32)
            if xn32.shape[0] == 1 and x32.shape[0] > 1:
                xn32 = xn32.expand(x32.shape[0], -1)
            xn32 = xn32.contiguous()
        filt = self.smoothing_filter
        if filt is not None:
            filt = filt.reshape(filt.shape[-2], filt.shape[-1]).to(device=x.device, dtype=torch.float32).contiguous()
        y = glue.spectral_gate(x32, xn32, self.n_fft, self.hop_length, self._window(x.device), filt, nonstationary=self.nonstationary,
                               n_std_thresh=self.n_std_thresh_stationary, n_thresh_ns=self.n_thresh_nonstationary,
                               temp_coeff=self.temp_coeff_nonstationary, n_movemean=self.n_movemean_nonstationary,
                               prop_decrease=self.prop_decrease)
        return (y[0] if squeeze else y).to(x.dtype)


class TorchGateBank:
    """``TorchGateHIP.forward(x, xn)`` for a bank of ``sessions`` talkers whose noise signal ``xn`` is a rolling buffer of ``nn`` samples
    (the realtime GUI's: the whole ``input_wav`` / ``output_buffer``, gui.py:983-985, 1020-1022), with the noise spectra kept from block to
    block: a block rewrites only the tail of ``xn``, so of its ``1 + nn // hop`` STFT frames only the few ``glue.gate_ring_plan`` calls dirty
    are transformed again (29 of 282 at the GUI's geometries).  Every active session's result is BIT-equal to ``tg(x[i][None], xn[i][None])``.

        bank = TorchGateBank(tg, sessions=S, nn=input_wav_len)
        y = bank.forward(x_rows, xn_rows, shift=block_frame, tail=block_frame, active=[True, False, ...])

    It owns the spectrum cache (one ``[S, Fn, K]`` complex128 ring, allocated at the first call with an active session: ``ring_bytes``,
    4.3 MB per session at 48 kHz), the ring's base, the host mirror of every session's state and the device ``mode`` vector (uploaded only
    when it changes).  A session is WARM -- only its dirty frames are transformed -- when it was active in the previous ``forward`` and has
    not been invalidated since; otherwise it is COLD and all its frames are.  The caller vouches that between two ``forward`` calls every
    warm session's ``xn`` row moved left by ``shift`` samples and only its last ``tail`` samples were rewritten; ``invalidate(i)`` after any
    other write.  Only the stationary gate is served (``tg.nonstationary`` raises).  ``RVCMI_GATE_RING=0`` (development) makes every
    active session cold in every call: the same results without the cache."""

    def __init__(self, tg: TorchGateHIP, sessions: int, nn: int):
        if int(sessions) < 1:
            raise ValueError("a bank has at least one session (got %d)" % int(sessions))
        if tg.nonstationary:
            raise ValueError("TorchGateBank serves the stationary gate only: the non-stationary mask ignores the noise signal")
        self.tg, self.S, self.nn = tg, int(sessions), int(nn)
        self.plan0 = glue.gate_ring_plan(self.nn, tg.n_fft, int(tg.hop_length), -1, 0)   # raises on a geometry the library refuses
        self.Fn = self.plan0["Fn"]
        self.ring_bytes = int(_lib.lib().rvcmi_glue_spectral_gate_ring_bytes(self.S, self.nn, tg.n_fft, int(tg.hop_length)))
        self.ring = None
        self.base = 0
        self.valid = [False] * self.S        # session i's ring rows hold the previous forward's spectra
        self._mode_host, self._mode = None, None
        self._scratch = None
        self._filt = None
        self.last_modes = None               # what the last forward ran: a list of 0 / 1 / 2 per session
        self.mode = None                     # the same on the device (uint8 [S])

    def invalidate(self, i: int) -> None:
        """Session ``i``'s cached spectra no longer describe its noise buffer: its next active call is cold."""
        self.valid[int(i)] = False

    def _modes(self, host, dev) -> torch.Tensor:
        if host != self._mode_host or self._mode is None or self._mode.device != dev:
            self._mode_host, self._mode = list(host), torch.tensor(host, dtype=torch.uint8, device=dev)
        return self._mode

    @torch.no_grad()
    def forward(self, x_rows: torch.Tensor, xn_rows: torch.Tensor, shift: int, tail: int, active, out: Optional[torch.Tensor] = None):
        """``x_rows`` [S, n], ``xn_rows`` [S, nn] float32 on the GPU (rows may be slices of longer buffers); ``active``: S booleans.
        -> the gated rows [S, hop * (n // hop)] (``out``, which may be ``x_rows`` itself, or a new tensor whose inactive rows are
        uninitialised); the device ``mode`` vector of this call is ``self.mode``.  With no active session nothing is launched or
        uploaded, ``out`` is returned as given and ``self.mode`` is None -- but the call still counts: every session is stale after it."""
        import os

        active = [bool(a) for a in active]
        if len(active) != self.S:
            raise ValueError("active must hold %d values, got %d" % (self.S, len(active)))
        if xn_rows.dim() != 2 or int(xn_rows.shape[1]) != self.nn:
            raise ValueError("xn_rows must be [%d, %d], got %s" % (self.S, self.nn, tuple(xn_rows.shape)))
        tg, dev = self.tg, x_rows.device
        tg._check_overlap_add(int(x_rows.shape[-1]))
        use_ring = os.environ.get("RVCMI_GATE_RING", "1") != "0"
        host = [0 if not a else (1 if (v and use_ring) else 2) for a, v in zip(active, self.valid)]
        plan = glue.gate_ring_plan(self.nn, tg.n_fft, int(tg.hop_length), shift, tail)
        self.base = (self.base + plan["advance"]) % self.Fn
        self.valid = active
        self.last_modes = host
        if not any(active):   # nothing is launched or uploaded; the sessions go stale
            self.mode = None
            return out
        self.mode = self._modes(host, dev)
        if self.ring is None or self.ring.device != dev:
            self.ring = torch.empty(self.ring_bytes, device=dev, dtype=torch.uint8)
        L = _lib.lib()
        nbytes = int(L.rvcmi_glue_spectral_gate_ring_scratch_bytes(self.S, int(x_rows.shape[1]), tg.n_fft, int(tg.hop_length)))
        if self._scratch is None or self._scratch.numel() < nbytes or self._scratch.device != dev:
            self._scratch = torch.empty(max(nbytes, 1), device=dev, dtype=torch.uint8)
        f = tg.smoothing_filter
        if f is not None and (self._filt is None or self._filt.device != dev):
            self._filt = f.reshape(f.shape[-2], f.shape[-1]).to(device=dev, dtype=torch.float32).contiguous()
        filt = self._filt if f is not None else None
        return glue.spectral_gate_ring(x_rows, xn_rows, shift, tail, self.ring, self.base, self.mode, 2 in host, tg.n_fft, int(tg.hop_length),
                                       tg._window(dev), filt, n_std_thresh=tg.n_std_thresh_stationary, prop_decrease=tg.prop_decrease, out=out,
                                       scratch=self._scratch)
