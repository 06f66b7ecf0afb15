// Host-only checks and plans of the per-session entry points of a realtime bank (no HIP here: tests/host/session_rows_main.cpp compiles
// this with a plain C++ compiler):
//   rvcmi_ivf_search_blend_expand_sessions   rvcmi_session_blend [S]
//   rvcmi_glue_envelope_mix_sessions         rvcmi_session_mix [S]
//   rvcmi_glue_input_gate_sessions           rvcmi_session_gate [S]
// The kernels read the device copy of what is checked here; everything that could take a block out of its buffers is refused before
// anything is launched (and the kernels bound a slot by the active count they are launched with, whatever the device copy says).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rvcmi.h"

namespace rvcmi {

constexpr int SESSIONS_MAX_S = 65535;  // a session is blockIdx.y

struct SessionBlendPlan {
    int active;          // sessions that are searched and blended: the packed slots are 0 .. active - 1, in session order
    int64_t rows;        // active * (nq - skip_rows): the rows of the one search
    int any_protect;     // some session's protect mix applies
};

// nullptr when the descriptors are fine (then *plan is filled), else what is wrong with them.  has_index: a handle was passed; has_pitchf:
// pitchf_dev is not NULL.
inline const char* session_blend_check(const rvcmi_session_blend* sess, int S, int64_t nq, int64_t skip_rows, int64_t p_len, bool has_index,
                                       bool has_pitchf, SessionBlendPlan* plan) {
    if (S < 1 || S > SESSIONS_MAX_S) return "S outside [1, 65535]";
    if (!sess) return "no host copy of the per-session values";
    if (nq < 1 || nq > 0x7fffffff || skip_rows < 0 || skip_rows > nq) return "nq outside [1, 2^31) or skip_rows outside [0, nq]";
    if (p_len < 0 || p_len > 2 * nq) return "p_len outside [0, 2 nq]";
    int next = 0, any_protect = 0;
    for (int s = 0; s < S; ++s) {
        const rvcmi_session_blend& c = sess[s];
        if (!std::isfinite(c.index_rate) || !std::isfinite(c.protect)) return "an index_rate or a protect that is not finite";
        if (c.slot >= 0) {
            if (!has_index) return "a session is to be blended, and there is no index";
            if (c.slot != next) return "the packed slots of the blending sessions must count up from 0 in session order";
            ++next;
        } else if (c.slot != -1) {
            return "the slot of a session that is not blended is -1";
        }
        if (c.protect_on != 0 && c.protect_on != 1) return "protect_on is 0 or 1";
        if (c.protect_on && !has_pitchf) return "a session's protect mix applies, and there is no pitchf";
        any_protect |= c.protect_on;
    }
    plan->active = next;
    plan->rows = (int64_t)next * (nq - skip_rows);
    plan->any_protect = any_protect;
    return nullptr;
}

// -> the number of sessions that are on through *active.
inline const char* session_mix_check(const rvcmi_session_mix* sess, int S, int* active) {
    if (S < 1 || S > SESSIONS_MAX_S) return "S outside [1, 65535]";
    if (!sess) return "no host copy of the per-session values";
    int n = 0;
    for (int s = 0; s < S; ++s) {
        if (sess[s].on != 0 && sess[s].on != 1) return "on is 0 or 1";
        if (!std::isfinite(sess[s].exponent)) return "an exponent float32(1 - rate) that is not finite";
        n += sess[s].on;
    }
    *active = n;
    return nullptr;
}

inline const char* session_gate_check(const rvcmi_session_gate* sess, int S, int* active) {
    if (S < 1 || S > SESSIONS_MAX_S) return "S outside [1, 65535]";
    if (!sess) return "no host copy of the per-session values";
    int n = 0;
    for (int s = 0; s < S; ++s) {
        const rvcmi_session_gate& c = sess[s];
        if (c.on != 0 && c.on != 1) return "on is 0 or 1";
        if (c.reserved_ != 0) return "reserved_ is 0";
        // the cutoffs are RMS values: >= 0, +inf allowed (realtime.input_gate_cutoffs), never NaN
        if (c.cut_a != c.cut_a || c.cut_b != c.cut_b || c.cut_a < 0.f || c.cut_b < 0.f) return "the cutoffs are RMS values (>= 0, not NaN)";
        n += c.on;
    }
    *active = n;
    return nullptr;
}

}  // namespace rvcmi
