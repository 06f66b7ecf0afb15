"""ctypes binding of ``include/rvcmi.h`` (librvcmi.so).

There is deliberately NO fallback: if the shared library has not been built, or a call fails,
this module raises.  A silent CPU/PyTorch fallback would void every parity and performance claim.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from typing import List

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RVCMI_LIB") or os.path.join(_HERE, "librvcmi.so")  # RVCMI_LIB: dev A/B builds
CSRC = os.path.join(_HERE, "csrc")
SOURCES = ["error.cpp", "nsf.hip", "rb_stream.hip", "ivf.hip", "front.hip", "glue.hip", "gru.hip", "unet.hip", "rmvpe.hip", "hubert_fe.hip", "hubert_enc.hip"]

RVCMI_MAX_UPS, RVCMI_MAX_RB, RVCMI_MAX_DIL = 8, 4, 4
RVCMI_VERSION = 2  # include/rvcmi.h; the argument lists of SYMBOLS below are those of this ABI version
OPERANDS = {"fp32": 0, "f32": 0, "bf16": 1, "fp16": 2, "f16": 2, "fp16x2": 3}  # fp16x2: the front only (RVCMI_OPERAND_F16X2)


class NsfConfig(C.Structure):
    _fields_ = [
        ("inter_channels", C.c_int),
        ("upsample_initial_channel", C.c_int),
        ("gin_channels", C.c_int),
        ("sr", C.c_int),
        ("use_f0", C.c_int),
        ("n_ups", C.c_int),
        ("upsample_rates", C.c_int * RVCMI_MAX_UPS),
        ("upsample_kernel_sizes", C.c_int * RVCMI_MAX_UPS),
        ("n_resblock_kernels", C.c_int),
        ("resblock_kernel_sizes", C.c_int * RVCMI_MAX_RB),
        ("n_dilations", C.c_int * RVCMI_MAX_RB),
        ("resblock_dilation_sizes", (C.c_int * RVCMI_MAX_DIL) * RVCMI_MAX_RB),
        ("operand", C.c_int),
    ]


class FrontConfig(C.Structure):
    _fields_ = [(n, C.c_int) for n in (
        "in_channels", "inter_channels", "hidden_channels", "filter_channels", "n_heads", "n_layers", "kernel_size",
        "window_size", "gin_channels", "use_f0", "flow_n_flows", "flow_n_layers", "flow_kernel_size", "flow_dilation_rate",
        "operand")]


class Tensor(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("ndim", C.c_int), ("shape", C.c_int64 * 4)]


class ResampleRow(C.Structure):
    """rvcmi_resample_row: one row's descriptor of rvcmi_glue_resample_poly_ragged."""
    _fields_ = [("w_off", C.c_int64), ("n", C.c_int64), ("orig", C.c_int), ("new_", C.c_int), ("K", C.c_int), ("width", C.c_int)]


class F0Row(C.Structure):
    """rvcmi_f0_row: one item's descriptor of rvcmi_glue_rmvpe_f0_ragged."""
    _fields_ = [("out_off", C.c_int64), ("key_mul", C.c_double), ("first_row", C.c_int), ("n", C.c_int), ("p_len", C.c_int), ("reserved_", C.c_int)]


class SessionBlend(C.Structure):
    """rvcmi_session_blend: one session's retrieval controls of rvcmi_ivf_search_blend_expand_sessions."""
    _fields_ = [("index_rate", C.c_float), ("protect", C.c_float), ("slot", C.c_int32), ("protect_on", C.c_int32)]


class SessionMix(C.Structure):
    """rvcmi_session_mix: one session's envelope-mix exponent of rvcmi_glue_envelope_mix_sessions."""
    _fields_ = [("exponent", C.c_float), ("on", C.c_int32)]


class SessionGate(C.Structure):
    """rvcmi_session_gate: one session's cutoffs of rvcmi_glue_input_gate_sessions."""
    _fields_ = [("cut_a", C.c_float), ("cut_b", C.c_float), ("on", C.c_int32), ("reserved_", C.c_int32)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


class NsfStagePlan(C.Structure):  # rvcmi_nsf_stage_plan: ints only
    _fields_ = [(n, C.c_int) for n in ("path", "C", "B", "rows", "x0_half", "y_half", "tile_rows", "tile_waves", "n_rb")] + [
        (n, C.c_int * RVCMI_MAX_RB) for n in ("k", "tiles", "strip_len")] + [
        (n, C.c_int) for n in ("stream_nj", "stream_mfma", "stream_fill_skip", "pair_streamed", "num_cus")]


RB_PATHS = ("F32_CHAIN", "SPLIT", "STREAM", "FULL", "PAIR")  # RVCMI_RB_*


# every symbol include/rvcmi.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("rvcmi_last_error", C.c_char_p, []),
    ("rvcmi_version", C.c_int, []),
    ("rvcmi_nsf_create", C.c_int, [C.POINTER(NsfConfig), C.POINTER(Tensor), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("rvcmi_nsf_destroy", C.c_int, [_P]),
    ("rvcmi_nsf_forward", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P]),
    ("rvcmi_nsf_forward_nres", C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, _P]),
    ("rvcmi_nsf_upp", C.c_int, [_P]),
    ("rvcmi_nsf_workspace_bytes", C.c_size_t, [_P]),
    ("rvcmi_nsf_debug_forward", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.c_char_p, _P, C.c_size_t,
                                          C.POINTER(C.c_int64), _P]),
    ("rvcmi_nsf_set_option", C.c_int, [_P, C.c_char_p, C.c_double]),
    ("rvcmi_nsf_profile_enable", C.c_int, [_P, C.c_int]),
    ("rvcmi_nsf_profile_read", C.c_int, [_P, C.POINTER(KernelStat), C.c_int, C.POINTER(C.c_int), C.c_int]),
    ("rvcmi_nsf_last_plan", C.c_int, [_P, C.POINTER(NsfStagePlan), C.c_int, C.POINTER(C.c_int)]),
    ("rvcmi_front_create", C.c_int, [C.POINTER(FrontConfig), C.POINTER(Tensor), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    ("rvcmi_front_destroy", C.c_int, [_P]),
    ("rvcmi_front_forward", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, _P, _P]),
    ("rvcmi_front_workspace_bytes", C.c_size_t, [_P]),
    ("rvcmi_front_debug_forward", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_int, C.c_char_p, _P, C.c_size_t,
                                            C.POINTER(C.c_int64), _P]),
    ("rvcmi_front_set_option", C.c_int, [_P, C.c_char_p, C.c_double]),
    ("rvcmi_front_profile_enable", C.c_int, [_P, C.c_int]),
    ("rvcmi_front_profile_read", C.c_int, [_P, C.POINTER(KernelStat), C.c_int, C.POINTER(C.c_int), C.c_int]),
    ("rvcmi_ivf_create_from_file", C.c_int, [C.c_char_p, C.c_int, C.POINTER(_P)]),
    ("rvcmi_ivf_build", C.c_int, [C.c_int, C.c_int64, _P, C.c_int64, C.c_int, C.c_uint64, C.c_int, _P, C.POINTER(_P)]),
    ("rvcmi_kmeans", C.c_int, [C.c_int, C.c_int64, _P, C.c_int64, C.c_int, C.c_uint64, C.c_int, _P, _P]),
    ("rvcmi_ivf_train", C.c_int, [C.c_int, C.c_int64, _P, C.c_int64, C.c_int, C.c_uint64, C.c_int, _P, C.POINTER(_P)]),
    ("rvcmi_ivf_add", C.c_int, [_P, C.c_int64, _P, C.c_int, _P]),
    ("rvcmi_ivf_write_file", C.c_int, [_P, C.c_char_p]),
    ("rvcmi_ivf_create", C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, _P, C.c_int, C.POINTER(_P)]),
    ("rvcmi_ivf_destroy", C.c_int, [_P]),
    ("rvcmi_ivf_d", C.c_int, [_P]),
    ("rvcmi_ivf_ntotal", C.c_int64, [_P]),
    ("rvcmi_ivf_nlist", C.c_int64, [_P]),
    ("rvcmi_ivf_nprobe", C.c_int, [_P]),
    ("rvcmi_ivf_set_nprobe", C.c_int, [_P, C.c_int]),
    ("rvcmi_ivf_reserve", C.c_int, [_P, C.c_int64]),
    ("rvcmi_ivf_search", C.c_int, [_P, C.c_int64, _P, C.c_int, _P, _P, _P]),
    ("rvcmi_ivf_search_blend", C.c_int, [_P, C.c_int64, _P, C.c_float, C.c_int, C.c_int, _P]),
    ("rvcmi_ivf_search_blend_expand", C.c_int, [_P, C.c_int64, _P, C.c_float, C.c_int, C.c_int, _P, C.c_float, C.c_int64, _P, _P]),
    ("rvcmi_ivf_search_blend_expand_batch", C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, _P, C.c_float, C.c_int, C.c_int, _P, C.c_float,
                                                      C.c_int64, _P, _P]),
    ("rvcmi_ivf_search_blend_expand_sessions", C.c_int, [_P, C.c_int, C.c_int64, C.c_int, C.c_int64, _P, _P, _P, C.c_int, C.c_int, _P, C.c_int64,
                                                         _P, _P]),
    ("rvcmi_ivf_reconstruct_n", C.c_int, [_P, C.c_int64, C.c_int64, _P]),
    ("rvcmi_ivf_blob", C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    ("rvcmi_ivf_centroids", C.c_int, [_P, _P]),
    ("rvcmi_ivf_blob_copy", C.c_int, [_P, _P, C.c_size_t, _P]),
    ("rvcmi_ivf_create_from_blob", C.c_int, [_P, C.c_size_t, C.c_int, C.c_int, C.POINTER(_P)]),
    ("rvcmi_ivf_set_option", C.c_int, [_P, C.c_char_p, C.c_double]),
    ("rvcmi_ivf_profile_enable", C.c_int, [_P, C.c_int]),
    ("rvcmi_ivf_profile_read", C.c_int, [_P, C.POINTER(KernelStat), C.c_int, C.POINTER(C.c_int), C.c_int]),
    ("rvcmi_glue_expand_protect", C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P, C.c_float, C.c_int64, _P, _P]),
    ("rvcmi_glue_rmvpe_f0", C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, _P, _P, _P, _P]),
    ("rvcmi_glue_f0_post", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P]),
    ("rvcmi_glue_rmvpe_f0_key", C.c_int, [_P, C.c_int, C.c_int, C.c_float, C.c_int, C.c_double, _P, _P, _P, _P]),
    ("rvcmi_glue_f0_post_key", C.c_int, [_P, C.c_int, C.c_double, _P, _P, _P]),
    ("rvcmi_glue_f0_key_mul", C.c_double, [C.c_double]),
    ("rvcmi_glue_rmvpe_f0_ragged", C.c_int, [_P, C.c_int64, C.c_int, C.c_int, _P, _P, C.c_float, _P, _P, _P, C.c_int64, _P]),
    ("rvcmi_glue_input_gate_scratch_floats", C.c_size_t, [C.c_int, C.c_int]),
    ("rvcmi_glue_input_gate_batch", C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_float, _P, _P]),
    ("rvcmi_glue_input_gate_sessions", C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, _P, _P, _P]),
    ("rvcmi_glue_envelope_mix_sessions", C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, _P]),
    ("rvcmi_glue_change_rms", C.c_int, [_P, C.c_int64, C.c_int, _P, C.c_int64, C.c_int, C.c_float, _P, _P]),
    ("rvcmi_glue_scale_int16_range", C.c_int, [_P, C.c_int64, _P, _P]),
    ("rvcmi_glue_resample_poly", C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, _P]),
    ("rvcmi_glue_sola", C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P]),
    ("rvcmi_glue_phase_vocoder", C.c_int, [_P, _P, _P, _P, C.c_int, _P, _P, _P]),
    ("rvcmi_glue_sola_pv", C.c_int, [_P, C.c_int64, _P, C.c_int, C.c_int, _P, _P, C.c_int, _P, _P, _P, _P]),
    ("rvcmi_glue_envelope_mix", C.c_int, [_P, _P, C.c_int64, C.c_int, C.c_double, _P, _P]),
    ("rvcmi_glue_resample_poly_batch", C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int64, C.c_int64, _P]),
    ("rvcmi_glue_resample_poly_ragged", C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, C.c_int64, C.c_int64, _P]),
    ("rvcmi_glue_sola_batch", C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int64, _P, _P]),
    ("rvcmi_glue_sola_pv_batch", C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, _P, C.c_int, _P, C.c_int64, _P, _P,
                                           _P]),
    ("rvcmi_glue_envelope_mix_batch", C.c_int, [C.c_int, _P, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int, C.c_double, _P, _P]),
    ("rvcmi_glue_expand_protect_batch", C.c_int, [C.c_int, _P, C.c_int64, C.c_int, C.c_int, _P, C.c_float, C.c_int64, _P, _P]),
    ("rvcmi_glue_spectral_gate", C.c_int, [_P, C.c_int, C.c_int64, _P, C.c_int64, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                           C.c_double, C.c_double, C.c_double, C.c_int, C.c_double, _P, _P, C.c_size_t, _P]),
    ("rvcmi_glue_spectral_gate_scratch_bytes", C.c_size_t, [C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int]),
    ("rvcmi_glue_spectral_gate_ring_batch", C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int64,
                                                      _P, C.c_size_t, C.c_int64, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                                      C.c_double, C.c_double, _P, C.c_size_t, _P]),
    ("rvcmi_glue_spectral_gate_ring_scratch_bytes", C.c_size_t, [C.c_int, C.c_int64, C.c_int, C.c_int]),
    ("rvcmi_glue_spectral_gate_ring_bytes", C.c_size_t, [C.c_int, C.c_int64, C.c_int, C.c_int]),
    ("rvcmi_glue_gate_ring_plan", C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int)]),
    ("rvcmi_glue_nr_stitch_batch", C.c_int, [C.c_int, _P, C.c_int64, C.c_int, C.c_int64, _P, _P, _P, C.c_int64, _P, C.c_int64, C.c_int64, _P, C.c_int64,
                                             _P, _P]),
    ("rvcmi_glue_masked_write_batch", C.c_int, [C.c_int, _P, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64, C.c_int64, _P, C.c_int64, C.c_int64,
                                                C.c_int64, _P, _P]),
    ("rvcmi_glue_cut_points", C.c_int, [_P, C.c_int64, C.c_int, C.c_int64, C.c_int64, _P, C.c_int64, _P, _P, _P]),
    ("rvcmi_glue_cut_points_scratch_bytes", C.c_size_t, [C.c_int64, C.c_int, C.c_int64, C.c_int64]),
    ("rvcmi_glue_filtfilt", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int64, C.c_int64, _P, _P, _P, C.c_int, C.c_int, _P, _P, C.c_int64, _P,
                                      C.c_size_t, _P]),
    ("rvcmi_glue_filtfilt_scratch_bytes", C.c_size_t, [C.c_int, C.c_int64, C.c_int]),
    ("rvcmi_gru_create", C.c_int, [C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.POINTER(_P)]),
    ("rvcmi_gru_destroy", C.c_int, [_P]),
    ("rvcmi_gru_forward", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P]),
    ("rvcmi_gru_forward_ragged", C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("rvcmi_unet_create", C.c_int, [C.POINTER(Tensor), C.c_int, C.c_int, C.POINTER(_P)]),
    ("rvcmi_unet_destroy", C.c_int, [_P]),
    ("rvcmi_unet_head_channels", C.c_int, [_P]),
    ("rvcmi_unet_workspace_bytes", C.c_size_t, [_P, C.c_int, C.c_int]),
    ("rvcmi_unet_forward", C.c_int, [_P, C.c_int, C.c_int, _P, _P, _P, _P]),
    ("rvcmi_unet_workspace_bytes_ragged", C.c_size_t, [_P, C.c_int, _P]),
    ("rvcmi_unet_forward_ragged", C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("rvcmi_unet_debug_op", C.c_int, [C.c_int] * 7 + [_P, _P, _P, C.c_int, C.c_float, C.c_float, _P, _P, _P, _P, C.c_int, C.c_int, _P]),
    ("rvcmi_mel_create", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_float, C.c_int, C.POINTER(_P)]),
    ("rvcmi_mel_destroy", C.c_int, [_P]),
    ("rvcmi_mel_frames", C.c_int64, [_P, C.c_int64]),
    ("rvcmi_mel_forward", C.c_int, [_P, C.c_int, C.c_int64, _P, C.c_int, C.c_int, _P, _P]),
    ("rvcmi_rmvpe_head", C.c_int, [_P, C.c_int, _P, _P, C.c_int, _P, _P]),
    ("rvcmi_hubert_fe_create", C.c_int, [C.POINTER(Tensor), C.c_int, C.c_int, C.POINTER(_P)]),
    ("rvcmi_hubert_fe_destroy", C.c_int, [_P]),
    ("rvcmi_hubert_fe_frames", C.c_int64, [C.c_int64]),
    ("rvcmi_hubert_fe_workspace_bytes", C.c_size_t, [_P, C.c_int, C.c_int64]),
    ("rvcmi_hubert_fe_forward", C.c_int, [_P, C.c_int, C.c_int64, _P, C.c_int, _P, _P, _P]),
    ("rvcmi_hubert_fe_workspace_bytes_ragged", C.c_size_t, [_P, C.c_int, C.c_int64]),
    ("rvcmi_hubert_fe_forward_ragged", C.c_int, [_P, C.c_int, C.c_int64, _P, _P, _P, C.c_int, _P, _P, _P]),
    ("rvcmi_hubert_fe_debug_conv", C.c_int, [C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_int, _P]),
    ("rvcmi_hubert_enc_create", C.c_int, [C.POINTER(Tensor), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(_P)]),
    ("rvcmi_hubert_enc_destroy", C.c_int, [_P]),
    ("rvcmi_hubert_enc_workspace_bytes", C.c_size_t, [_P, C.c_int, C.c_int]),
    ("rvcmi_hubert_enc_forward", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, _P, _P, _P]),
]


class RvcmiError(RuntimeError):
    """``code``: the C ABI's return value (include/rvcmi.h: -1 invalid, -2 HIP, -3 IO / not an IVF-Flat L2 file, -4 no memory,
    -5 missing weight); None for errors raised on the Python side."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


ERR_INVALID, ERR_IO, ERR_NOMEM = -1, -3, -4


_lib = None


def _unit_deps(src: str) -> List[str]:
    """`src` and every local header it includes, transitively (`#include "x.hpp"` next to it, `rvcmi.h` under include/)."""
    import re

    seen, todo = [], [src]
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(f):
            continue
        seen.append(f)
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(f, errors="replace").read(), re.M):
            for base in (os.path.dirname(f), os.path.join(_HERE, "..", "include")):
                cand = os.path.normpath(os.path.join(base, inc))
                if os.path.exists(cand):
                    todo.append(cand)
                    break
    return seen


def build(verbose: bool = True, force: bool = False) -> str:
    """Compile librvcmi.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    deps = srcs + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    deps.append(os.path.join(_HERE, "..", "include", "rvcmi.h"))
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in deps):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objs = []
    procs = []
    flags_key = " ".join([os.environ.get(k, "") for k in ("RVCMI_DEFINES", "RVCMI_DEV_STAMPS", "RVCMI_NO_MFMA_VGPR_FORM", "HIPCC")])
    stamp = os.path.join(CSRC, ".build_flags")
    same_flags = os.path.exists(stamp) and open(stamp).read() == flags_key
    for s in srcs:  # compile the translation units in parallel; a unit whose object is newer than it and every header it includes is kept
        o = os.path.join(CSRC, os.path.basename(s) + ".o")
        objs.append(o)
        if not force and same_flags and os.path.exists(o) and all(os.path.getmtime(o) >= os.path.getmtime(d) for d in _unit_deps(s)):
            continue
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", s, "-o", o]
        if not os.environ.get("RVCMI_NO_MFMA_VGPR_FORM"):
            # MFMA results in VGPRs wherever the 256 architectural VGPRs allow it: by default LLVM puts every accumulator in an
            # AGPR and copies it out with v_accvgpr_read for each VALU use (publish, bias, residual) -- 21 000 such copies in
            # nsf.hip alone, none with this option; the 512-register kernels keep their overflow in AGPRs
            cmd[1:1] = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
        for d_ in os.environ.get("RVCMI_DEFINES", "").split():
            cmd.insert(1, "-D" + d_)  # dev: compile-time defaults, e.g. RVCMI_DEFINES="RS_MFMA_DEFAULT=32"
        if os.environ.get("RVCMI_DEV_STAMPS"):
            cmd.insert(1, "-DRVCMI_DEV_STAMPS")  # per-phase s_memtime stamps in the fused kernels (RVCMI_DBG=32)
        if verbose:
            print("[rvcmi build]", " ".join(cmd), file=sys.stderr)
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode:
            raise RvcmiError("hipcc failed: %s\n%s" % (" ".join(cmd), out.decode(errors="replace")))
    with open(stamp, "w") as f:
        f.write(flags_key)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
    if verbose:
        print("[rvcmi build]", " ".join(cmd), file=sys.stderr)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode:
        raise RvcmiError("link failed:\n" + r.stdout.decode(errors="replace"))
    return LIB_PATH


def lib() -> C.CDLL:
    """The loaded library; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RvcmiError(
                "librvcmi.so is not built (%s).  Run `python __graft_entry__.py build`.  "
                "There is no CPU fallback for the HIP hot path." % LIB_PATH)
        l = C.CDLL(LIB_PATH)
        for name, res, args in SYMBOLS:
            f = getattr(l, name)  # AttributeError if the header and the library drift apart
            f.restype = res
            f.argtypes = args
        v = l.rvcmi_version()
        if v != RVCMI_VERSION:  # a stale .so against a newer header shifts pointer arguments: garbage reads, not an error
            raise RvcmiError("%s implements ABI version %d, this binding is written against %d (include/rvcmi.h); rebuild with "
                             "`python __graft_entry__.py build`" % (LIB_PATH, v, RVCMI_VERSION))
        _lib = l
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().rvcmi_last_error()
        raise RvcmiError("rvcmi error %d: %s" % (rc, msg.decode(errors="replace") if msg else "?"), code=int(rc))


def device_index(dev) -> int:
    """The ordinal of a CUDA (ROCm) device; ``cuda`` without an index means the current device."""
    import torch

    dev = torch.device(dev)
    return dev.index if dev.index is not None else torch.cuda.current_device()


# ---- what every wrapper of a handle shares ----------------------------------------------------------------------

def cuda_device(device, who: str):
    """``device`` as ``torch.device("cuda", i)`` with the index filled in; anything that is not a GPU raises."""
    import torch

    dev = torch.device(device)
    if dev.type != "cuda":
        raise RvcmiError("%s needs a GPU device (got %s); there is no CPU fallback" % (who, device))
    return torch.device("cuda", device_index(dev))


def ptr(t) -> C.c_void_p:
    """The data pointer of a tensor; ``None`` is the null pointer."""
    return C.c_void_p(t.data_ptr() if t is not None else None)


def stream_ptr(dev) -> C.c_void_p:
    """torch's current stream on ``dev``: every launch of the library goes on the caller's stream."""
    import torch

    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def require_on(t, device, who: str) -> None:
    """``t`` must be a tensor on the GPU ``device`` (normalised, as ``cuda_device`` returns it).  The library launches on the handle's
    device with ``t``'s pointer and ``t``'s stream, so a mismatch must not get through."""
    import torch

    if not torch.is_tensor(t) or t.device.type != "cuda":
        raise RvcmiError("%s input must live on the GPU (got %s); there is no CPU fallback" % (who, getattr(t, "device", type(t))))
    if t.device != device:
        raise RvcmiError("%s: the input is on %s, the weights on %s" % (who, t.device, device))


def on_gpu(t, what: str):
    """The argument ``what`` of a stateless entry point (the glue): on any GPU -> its device, which is where the call launches."""
    if t.device.type != "cuda":
        raise RvcmiError("%s must live on the GPU (got %s); the glue has no CPU fallback" % (what, t.device))
    return t.device


def workspace_ptr(workspace, need: int, device, who: str) -> C.c_void_p:
    """A caller's workspace as a pointer: it must hold ``need`` (> 0) uint8 on ``device``."""
    import torch

    if workspace.device != device or workspace.dtype != torch.uint8 or workspace.numel() < need or need == 0:
        raise RvcmiError("%s: the workspace must be %d uint8 on %s" % (who, need, device), code=ERR_INVALID)
    return ptr(workspace)


def pack_tensors(named):
    """(name, fp32 contiguous CPU tensor) pairs -> the ``rvcmi_tensor`` array a create call reads.  The array keeps the encoded names and
    the tensors alive (``.keep``), so it is valid for as long as the caller holds it."""
    import torch

    keep = [(k.encode(), t) for k, t in named]
    arr = (Tensor * len(keep))()
    for a, (kb, t) in zip(arr, keep):
        if t.device.type != "cpu" or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() > 4:
            raise ValueError("pack_tensors: '%s' must be a contiguous fp32 CPU tensor of at most 4 dimensions" % kb.decode())
        a.name, a.data, a.ndim = kb, t.data_ptr(), t.dim()
        a.shape[:t.dim()] = list(t.shape)
    arr.keep = keep
    return arr


class Handle:
    """Owns one ``rvcmi_*`` handle and the NAME of its destroy function (looked up at close: at interpreter shutdown the library may be
    gone, and then there is nothing left to free).  Truthy while open; passes to ctypes as the pointer."""

    def __init__(self, destroy: str, pointer: C.c_void_p):
        self._destroy, self._as_parameter_ = destroy, pointer

    def __bool__(self) -> bool:
        return bool(self._as_parameter_)

    def close(self) -> None:
        p, self._as_parameter_ = self._as_parameter_, C.c_void_p(None)
        if p:
            getattr(lib(), self._destroy)(p)

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa  (interpreter shutdown)
            pass


class Switch:
    """An opt-in of the integration layer.  Its value IS the module global ``name`` of ``ns`` (what ``install()`` and the tests set), so the
    global keeps its name and meaning; the environment variable ``env`` = ``"1"`` / ``"0"`` overrides it per call, any other value is
    ignored.  ``base``: a switch this one is effective only together with."""

    def __init__(self, env: str, ns: dict, name: str, base: "Switch" = None):
        self.env, self._ns, self.name, self.base = env, ns, name, base

    @property
    def value(self):
        return self._ns[self.name]

    @value.setter
    def value(self, v) -> None:
        self._ns[self.name] = v

    def on(self) -> bool:
        env = os.environ.get(self.env)
        return (self.base is None or self.base.on()) and (env == "1" if env in ("0", "1") else bool(self.value))


def once(obj, attr: str, fn):
    """``fn()`` once per object: the result is remembered on ``obj`` as ``attr`` and returned from then on.  An object that cannot hold
    it (no ``__dict__``) has ``fn`` run again next time."""
    got = getattr(obj, attr, None)
    if got is None:
        got = fn()
        try:
            object.__setattr__(obj, attr, got)
        except Exception:  # noqa
            pass
    return got


def set_option(fn, handle, key: str, value) -> None:
    """Dev / test option of one handle (include/rvcmi.h rvcmi_*_set_option); ``value=None`` restores the default."""
    check(fn(handle, key.encode(), float("nan") if value is None else float(value)))


def read_stats(read_fn, handle, reset: bool = True) -> List[dict]:
    n = C.c_int(0)
    buf = (KernelStat * 64)()
    check(read_fn(handle, buf, 64, C.byref(n), 1 if reset else 0))
    return [dict(name=buf[i].name.decode(), launches=int(buf[i].launches), ms=float(buf[i].ms),
                 flops=float(buf[i].flops), bytes=float(buf[i].bytes)) for i in range(min(n.value, 64))]
