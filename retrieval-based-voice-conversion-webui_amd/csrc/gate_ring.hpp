// The host side of rvcmi_glue_spectral_gate_ring_batch: which noise frames of a rolled buffer must be transformed again, where a
// frame's spectrum lives in the caller's cache, how the launch is tiled, and the scratch / cache sizes.  Host-only like
// ivf_format.hpp and weights.hpp: no HIP here, so the stand-alone test program (tests/host/gate_ring_main.cpp) builds it with a plain
// C++ compiler and sanitizers, and Python reads the same rule through rvcmi_glue_gate_ring_plan.
//
// The noise signal xn [nn] is a rolling buffer: between two calls it moved left by `shift` samples and its last `tail` samples
// were rewritten.  k_gate_stft sums every frame in an order that does not depend on the frame's place in its tile, so a frame whose
// n_fft samples (zero padding included) equal those of frame f + shift / hop of the previous call has that frame's spectrum bit for
// bit.  Frame f of the Fn = 1 + nn / hop frames covers samples [f hop - n_fft / 2, f hop + n_fft / 2) and is CLEAN iff
//   shift >= 0, shift % hop == 0, tail <= nn                                      (else every frame is dirty: the cold arithmetic), and
//   shift > 0:   f hop - n_fft / 2 >= 0  and  f hop + n_fft / 2 <= nn - max(tail, shift)
//   shift == 0:  tail == 0  or  f hop + n_fft / 2 <= nn - tail                    (the frame keeps its slot, its zero padding included)
// (a roll by `shift` rewrites at least `shift` samples, so a smaller tail counts as `shift`).  The dirty frames are therefore a head
// [0, head) and a back [back, Fn); the clean ones in between are not touched.
#pragma once
#include <cstddef>
#include <cstdint>

#include "weights.hpp"

namespace rvcmi {

constexpr int GATE_RING_FT = 8;          // frames per block of the transforms (GATE_FT of gate_kernels.hpp; glue.hip asserts they agree)
constexpr int GATE_RING_MAX_NFFT = 4096;  // RVCMI_GATE_MAX_NFFT
constexpr int GATE_RING_MAX_S = 65535;    // RVCMI_BANK_MAX_S

struct GateRingPlan {
    int Fn, K;          // noise frames, bins
    int head, back;     // dirty: logical frames [0, head) and [back, Fn); head == Fn (and back == Fn) when every frame is dirty
    int advance;        // what the caller adds to the previous call's ring_base to get this call's: shift / hop; 0 when every frame is dirty
    int n_dirty;        // head + Fn - back
    int tiles_dirty;    // ceil(n_dirty / GATE_RING_FT): noise tiles of a launch without a cold session
    int tiles_cold;     // ceil(Fn / GATE_RING_FT): noise tiles of a launch with one
};

inline bool gate_ring_geometry_ok(int64_t nn, int n_fft, int hop) {
    return nn >= 1 && n_fft >= 2 && !(n_fft & 1) && n_fft <= GATE_RING_MAX_NFFT && hop >= 1 && hop <= n_fft && nn / hop < 65535 * (int64_t)GATE_RING_FT - 1;
}

// false: the geometry is out of range.  Any shift / tail is served (what the rule cannot use makes every frame dirty).
inline bool gate_ring_plan(int64_t nn, int n_fft, int hop, int64_t shift, int64_t tail, GateRingPlan* p) {
    if (!gate_ring_geometry_ok(nn, n_fft, hop)) return false;
    const int64_t Fn = 1 + nn / hop, h = n_fft / 2;
    int64_t head = Fn, back = Fn, adv = 0;
    if (shift >= 0 && shift % hop == 0 && tail <= nn && shift <= nn) {
        if (tail < 0) tail = 0;
        if (tail < shift) tail = shift;
        int64_t lo, hi;  // clean: lo <= f <= hi
        if (shift == 0) {
            lo = 0;
            hi = tail == 0 ? Fn - 1 : (nn - tail - h >= 0 ? (nn - tail - h) / hop : -1);
        } else {
            lo = (h + hop - 1) / hop;
            hi = nn - tail - h >= 0 ? (nn - tail - h) / hop : -1;
        }
        if (hi > Fn - 1) hi = Fn - 1;
        if (hi >= lo) head = lo, back = hi + 1, adv = shift / hop;
    }
    p->Fn = (int)Fn;
    p->K = n_fft / 2 + 1;
    p->head = (int)head;
    p->back = (int)back;
    p->advance = (int)(adv % Fn);
    p->n_dirty = (int)(head + Fn - back);
    p->tiles_dirty = (p->n_dirty + GATE_RING_FT - 1) / GATE_RING_FT;
    p->tiles_cold = ((int)Fn + GATE_RING_FT - 1) / GATE_RING_FT;
    return true;
}

inline bool gate_ring_is_dirty(const GateRingPlan& p, int f) { return f < p.head || f >= p.back; }

// The j-th frame a warm session transforms (0 <= j < n_dirty), in logical order: the head, then the back.
inline int gate_ring_dirty_frame(const GateRingPlan& p, int j) { return j < p.head ? j : p.back + (j - p.head); }

// Slot of logical frame f in a session's [Fn][K] cache.  ring_base may be any value (negative too).
inline int gate_ring_slot(int64_t ring_base, int f, int Fn) {
    int64_t b = ring_base % Fn;
    if (b < 0) b += Fn;
    return (int)((b + f) % Fn);
}

// The cache: [S][Fn][K] double2.  0: out of range.
inline size_t gate_ring_bytes(int S, int64_t nn, int n_fft, int hop) {
    if (S < 1 || S > GATE_RING_MAX_S || !gate_ring_geometry_ok(nn, n_fft, hop)) return 0;
    return (size_t)S * (size_t)(1 + nn / hop) * (size_t)(n_fft / 2 + 1) * 16;
}

// Scratch of rvcmi_glue_spectral_gate_ring_batch, in this order (each part 256-byte aligned):
//   X [S][F][K] double2 | xmax, thresh [S][K] double | mask [S][F][K] float | frames [S][F][n_fft] double,   F = 1 + n / hop
struct GateRingLayout {
    size_t x, xmax, thresh, mask, frames, total;
    int F, K, tiles_x;
};
inline bool gate_ring_layout(int S, int64_t n, int n_fft, int hop, GateRingLayout* g) {
    if (S < 1 || S > GATE_RING_MAX_S || n < 1 || !gate_ring_geometry_ok(1, n_fft, hop)) return false;
    const int64_t F = 1 + n / hop, K = n_fft / 2 + 1;
    if (F > 65535) return false;
    Carve c;
    g->x = c.take((size_t)S * F * K * 16);
    g->xmax = c.take((size_t)S * K * 8);
    g->thresh = c.take((size_t)S * K * 8);
    g->mask = c.take((size_t)S * F * K * 4);
    g->frames = c.take((size_t)S * F * n_fft * 8);
    g->total = c.off;
    g->F = (int)F;
    g->K = (int)K;
    g->tiles_x = (int)((F + GATE_RING_FT - 1) / GATE_RING_FT);
    return true;
}

}  // namespace rvcmi
