// C entry points of the device-resident glue; kernels in glue_kernels.hpp.
#include <atomic>
#include <cmath>

#include "common.hpp"
#include "cut_kernels.hpp"
#include "f0_rows.hpp"
#include "filt_kernels.hpp"
#include "gate_kernels.hpp"
#include "gate_ring.hpp"
#include "glue_kernels.hpp"
#include "session_rows.hpp"

using namespace rvcmi;

// one once-flag per kernel that needs more dynamic LDS than the default
static std::atomic<unsigned long long> g_attr_f0{0}, g_attr_sola{0}, g_attr_sola_search{0}, g_attr_pv_spec{0}, g_attr_pv_synth{0},
    g_attr_gate_stft{0}, g_attr_gate_idft{0}, g_attr_gate_stft_r{0}, g_attr_gate_idft_r{0}, g_attr_f0_ragged{0};

#define RVCMI_BANK_MAX_S 65535  // a session is blockIdx.y (or blockIdx.x of a one-block-per-session launch)
static_assert(GATE_RING_FT == GATE_FT && GATE_RING_MAX_NFFT == RVCMI_GATE_MAX_NFFT && GATE_RING_MAX_S == RVCMI_BANK_MAX_S,
              "gate_ring.hpp restates the tile and the limits of the kernels");

// Scratch of rvcmi_glue_spectral_gate, in this order (each part 256-byte aligned):
//   X [B][F][K] double2 | XN [B][Fn][K] double2 (nn > 0) | xmax, thresh [B][K] double | mask [B][F][K] float | frames [B][F][n_fft] double
struct GateLayout {
    size_t x, xn, xmax, thresh, mask, frames, total;
};
static bool gate_layout(int B, int64_t n, int64_t nn, int n_fft, int hop, GateLayout* g) {
    if (B < 1 || n < 1 || nn < 0 || n_fft < 2 || (n_fft & 1) || n_fft > RVCMI_GATE_MAX_NFFT || hop < 1 || hop > n_fft) return false;
    const int64_t F = 1 + n / hop, Fn = nn > 0 ? 1 + nn / hop : 0, K = n_fft / 2 + 1;
    const int64_t tiles = (F + GATE_FT - 1) / GATE_FT + (Fn + GATE_FT - 1) / GATE_FT;
    if (F > 65535 || tiles > 65535 || (int64_t)B > 65535) return false;
    Carve c;
    g->x = c.take((size_t)B * F * K * 16);
    g->xn = c.take((size_t)B * Fn * K * 16);
    g->xmax = c.take((size_t)B * K * 8);
    g->thresh = c.take((size_t)B * K * 8);
    g->mask = c.take((size_t)B * F * K * 4);
    g->frames = c.take((size_t)B * F * n_fft * 8);
    g->total = c.off;
    return true;
}

// rvcmi_glue_filtfilt: one launch per pass; the kernel is instantiated per filter order (zero-padded coefficients would add
// +-0 terms to the chain, which is not scipy's arithmetic) and per input type.
template <typename T>
static void launch_filtfilt(int order, const T* x, const int64_t* offsets, int64_t total, int64_t max_len, const FiltCoef& c, int padlen,
                            int warm, double* y1, double* out, double* out_pad, int64_t pad, dim3 grid, hipStream_t st) {
#define RVCMI_FILT_CASE(O)                                                                                                                \
    case O:                                                                                                                               \
        hipLaunchKernelGGL((k_filt_pass<O, T, false>), grid, dim3(FILT_WAVE), 0, st, x, offsets, total, max_len, c, padlen, warm, y1,    \
                           (double*)nullptr, (double*)nullptr, (int64_t)0);                                                               \
        hipLaunchKernelGGL((k_filt_pass<O, T, true>), grid, dim3(FILT_WAVE), 0, st, x, offsets, total, max_len, c, padlen, warm, y1, out, \
                           out_pad, pad);                                                                                                 \
        break;
    switch (order) {
        RVCMI_FILT_CASE(1) RVCMI_FILT_CASE(2) RVCMI_FILT_CASE(3) RVCMI_FILT_CASE(4) RVCMI_FILT_CASE(5) RVCMI_FILT_CASE(6) RVCMI_FILT_CASE(7)
        RVCMI_FILT_CASE(8)
    }
#undef RVCMI_FILT_CASE
}

extern "C" {

size_t rvcmi_glue_filtfilt_scratch_bytes(int B, int64_t total, int order) {
    if (B < 1 || B > 65535 || total < 1 || order < 1 || order > RVCMI_FILT_MAX_ORDER) return 0;
    return (size_t)(total + 2 * 3 * (int64_t)(order + 1) * B) * sizeof(double);
}

int rvcmi_glue_filtfilt(const void* x, int x_is_f64, const int64_t* offsets, int B, int64_t max_len, int64_t total, const double* b,
                        const double* a, const double* zi, int order, int warmup, double* out, double* out_pad, int64_t pad, void* scratch,
                        size_t scratch_bytes, void* stream) {
    return guarded([&] {
        if (order < 1 || order > RVCMI_FILT_MAX_ORDER)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "filtfilt: filter order %d outside [1, %d]", order, RVCMI_FILT_MAX_ORDER);
        if (!x || !offsets || !b || !a || !zi || !out || !scratch) RVCMI_FAIL(RVCMI_ERR_INVALID, "filtfilt: null pointer");
        if (a[0] != 1.0) RVCMI_FAIL(RVCMI_ERR_INVALID, "filtfilt: a[0] = %g, the coefficients must be normalised to a[0] = 1", a[0]);
        const int padlen = 3 * (order + 1);
        if (B < 1 || B > 65535 || max_len <= padlen || max_len > RVCMI_FILT_MAX_LEN || total < max_len)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "filtfilt: B = %d in [1, 65535], longest item %lld in (padlen = %d, 2^28], total %lld >= longest item", B,
                       (long long)max_len, padlen, (long long)total);
        if (warmup < 0 || warmup % FILT_LANE || warmup > (1 << 20))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "filtfilt: warm-up of %d samples must be a multiple of %d in [0, 2^20]", warmup, FILT_LANE);
        if (out_pad && (pad < 0 || pad >= max_len)) RVCMI_FAIL(RVCMI_ERR_INVALID, "filtfilt: reflection pad %lld outside [0, longest item)", (long long)pad);
        const size_t need = rvcmi_glue_filtfilt_scratch_bytes(B, total, order);
        if (scratch_bytes < need) RVCMI_FAIL(RVCMI_ERR_INVALID, "filtfilt: scratch of %zu bytes, %zu needed", scratch_bytes, need);
        const int64_t lanes = (max_len + 2 * padlen + FILT_LANE - 1) / FILT_LANE;
        const int64_t gx = (lanes + FILT_WAVE - 1) / FILT_WAVE;
        FiltCoef c = {};
        for (int k = 0; k <= order; ++k) c.b[k] = b[k], c.a[k] = a[k];
        for (int k = 0; k < order; ++k) c.zi[k] = zi[k];
        const dim3 grid((unsigned)gx, (unsigned)B);
        hipStream_t st = (hipStream_t)stream;
        double* y1 = static_cast<double*>(scratch);
        if (x_is_f64)
            launch_filtfilt(order, static_cast<const double*>(x), offsets, total, max_len, c, padlen, warmup, y1, out, out_pad, pad, grid, st);
        else
            launch_filtfilt(order, static_cast<const float*>(x), offsets, total, max_len, c, padlen, warmup, y1, out, out_pad, pad, grid, st);
        HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"

// Geometry of rvcmi_glue_cut_points: false when the arguments are out of range.  cuts = len(range(t_center, n, t_center)).
static bool cut_layout(int64_t n, int window, int64_t t_center, int64_t t_query, int64_t* cuts, int* tiles) {
    if (window < 2 || (window & 1) || window > RVCMI_CUT_MAX_WINDOW || n <= window || t_center < 1 || t_query < 1 || t_query > t_center)
        return false;
    const int64_t nt = (2 * t_query + CUT_TILE - 1) / CUT_TILE;
    *cuts = n > t_center ? (n - 1) / t_center : 0;
    if (nt > 0x7fffffff || *cuts > 65535) return false;
    *tiles = (int)nt;
    return true;
}

extern "C" {

size_t rvcmi_glue_cut_points_scratch_bytes(int64_t n, int window, int64_t t_center, int64_t t_query) {
    int64_t cuts;
    int tiles;
    if (!cut_layout(n, window, t_center, t_query, &cuts, &tiles)) return 0;
    return (size_t)cuts * tiles * sizeof(CutBest);
}

int rvcmi_glue_cut_points(const double* audio, int64_t n, int window, int64_t t_center, int64_t t_query, int64_t* cuts_out, int64_t max_cuts,
                          double* sums, void* scratch, void* stream) {
    return guarded([&] {
        int64_t cuts;
        int tiles;
        if (!cut_layout(n, window, t_center, t_query, &cuts, &tiles))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "cut_points: window = %d must be even and in [2, %d], n = %lld > window, 1 <= t_query = %lld <= t_center = %lld, "
                       "at most 65535 cuts", window, RVCMI_CUT_MAX_WINDOW, (long long)n, (long long)t_query, (long long)t_center);
        if (cuts > max_cuts) RVCMI_FAIL(RVCMI_ERR_INVALID, "cut_points: %lld cuts, room for %lld", (long long)cuts, (long long)max_cuts);
        if (!cuts) return;
        if (!audio || !cuts_out || !scratch) RVCMI_FAIL(RVCMI_ERR_INVALID, "cut_points: null pointer");
        hipStream_t st = (hipStream_t)stream;
        CutBest* best = static_cast<CutBest*>(scratch);
        hipLaunchKernelGGL(k_cut_sums, dim3((unsigned)tiles, (unsigned)cuts), dim3(CUT_THREADS), 0, st, audio, n, window, t_center, t_query, tiles,
                           best, sums);
        hipLaunchKernelGGL(k_cut_pick, dim3((unsigned)cuts), dim3(CUT_THREADS), 0, st, (const CutBest*)best, tiles, t_center, t_query, cuts_out);
        HIP_CHECK(hipGetLastError());
    });
}


size_t rvcmi_glue_spectral_gate_scratch_bytes(int B, int64_t n, int64_t nn, int n_fft, int hop) {
    GateLayout g;
    return gate_layout(B, n, nn, n_fft, hop, &g) ? g.total : 0;
}

int rvcmi_glue_spectral_gate(const float* x, int B, int64_t n, const float* xn, int64_t nn, int n_fft, int hop, const double* window,
                             const float* filter, int nf, int nt, int nonstationary, double n_std_thresh, double n_thresh_ns,
                             double temp_coeff, int n_movemean, double prop_decrease, float* out, void* scratch, size_t scratch_bytes,
                             void* stream) {
    return guarded([&] {
        if (!x || !window || !out || !scratch) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: null pointer");
        if (n_fft < 2 || n_fft > RVCMI_GATE_MAX_NFFT || (n_fft & 1))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: n_fft = %d must be even and in [2, %d]", n_fft, RVCMI_GATE_MAX_NFFT);
        if (hop < 1 || hop > n_fft) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: hop = %d outside [1, n_fft = %d]", hop, n_fft);
        if (B < 1 || n < 1 || (xn && nn < 1)) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: empty input");
        if (filter && (nf < 1 || nt < 1 || (int64_t)nf * nt > (1 << 20)))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: smoothing filter %d x %d", nf, nt);
        if (!(prop_decrease >= 0.0 && prop_decrease <= 1.0)) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: prop_decrease outside [0, 1]");
        if (nonstationary && n_movemean < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: n_movemean < 1");
        const bool use_xn = xn && !nonstationary;  // the non-stationary mask looks at x alone (torchgate.py:246-247)
        GateLayout g;
        if (!gate_layout(B, n, use_xn ? nn : 0, n_fft, hop, &g)) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: too many frames");
        if (scratch_bytes < g.total)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate: scratch of %zu bytes, %zu needed", scratch_bytes, g.total);
        char* s = static_cast<char*>(scratch);
        double2* X = reinterpret_cast<double2*>(s + g.x);
        double2* XN = use_xn ? reinterpret_cast<double2*>(s + g.xn) : nullptr;
        double* xmax = reinterpret_cast<double*>(s + g.xmax);
        double* thresh = reinterpret_cast<double*>(s + g.thresh);
        float* mraw = reinterpret_cast<float*>(s + g.mask);
        double* z = reinterpret_cast<double*>(s + g.frames);
        const int F = (int)(1 + n / hop), Fn = use_xn ? (int)(1 + nn / hop) : 0, K = n_fft / 2 + 1;
        const int tiles_x = (F + GATE_FT - 1) / GATE_FT, tiles_n = (Fn + GATE_FT - 1) / GATE_FT;
        const int64_t Lout = (int64_t)hop * (n / hop);
        const int lds = gate_lds_bytes(n_fft);
        hipStream_t st = (hipStream_t)stream;
        ensure_dyn_lds((const void*)k_gate_stft, gate_lds_bytes(RVCMI_GATE_MAX_NFFT), g_attr_gate_stft);
        ensure_dyn_lds((const void*)k_gate_idft, gate_lds_bytes(RVCMI_GATE_MAX_NFFT), g_attr_gate_idft);
        hipLaunchKernelGGL(k_gate_stft, dim3((unsigned)((K + 63) / 64), (unsigned)(tiles_x + tiles_n), (unsigned)B), dim3(256), (size_t)lds, st,
                           x, n, F, X, use_xn ? xn : x, use_xn ? nn : n, Fn, XN, tiles_x, n_fft, hop, window);
        hipLaunchKernelGGL(k_gate_stats, dim3((unsigned)((K + 63) / 64), (unsigned)B), dim3(1024), 0, st, (const double2*)X, F,
                           (const double2*)XN, Fn, K, nonstationary ? 0 : 1, n_std_thresh, xmax, thresh);
        hipLaunchKernelGGL(k_gate_mask, dim3((unsigned)((K + 255) / 256), (unsigned)F, (unsigned)B), dim3(256), 0, st, (const double2*)X, F, K,
                           (const double*)xmax, (const double*)thresh, nonstationary ? 1 : 0, n_thresh_ns, temp_coeff, n_movemean,
                           (float)prop_decrease, mraw);
        hipLaunchKernelGGL(k_gate_smooth, dim3((unsigned)((K + 255) / 256), (unsigned)F, (unsigned)B), dim3(256), 0, st, X, F, K,
                           (const float*)mraw, filter, nf, nt);
        hipLaunchKernelGGL(k_gate_idft, dim3((unsigned)((n_fft + 63) / 64), (unsigned)tiles_x, (unsigned)B), dim3(256), (size_t)lds, st,
                           (const double2*)X, F, n_fft, window, z);
        if (Lout > 0)
            hipLaunchKernelGGL(k_gate_ola, dim3((unsigned)((Lout + 255) / 256), (unsigned)B), dim3(256), 0, st, (const double*)z, F, n_fft, hop,
                               window, Lout, out);
        HIP_CHECK(hipGetLastError());
    });
}


size_t rvcmi_glue_spectral_gate_ring_scratch_bytes(int S, int64_t n, int n_fft, int hop) {
    GateRingLayout g;
    return gate_ring_layout(S, n, n_fft, hop, &g) ? g.total : 0;
}

size_t rvcmi_glue_spectral_gate_ring_bytes(int S, int64_t nn, int n_fft, int hop) { return gate_ring_bytes(S, nn, n_fft, hop); }

int rvcmi_glue_gate_ring_plan(int64_t nn, int n_fft, int hop, int64_t shift, int64_t tail, int* plan_out) {
    return guarded([&] {
        GateRingPlan p;
        if (!plan_out) RVCMI_FAIL(RVCMI_ERR_INVALID, "gate_ring_plan: null pointer");
        if (!gate_ring_plan(nn, n_fft, hop, shift, tail, &p))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "gate_ring_plan: nn = %lld >= 1, n_fft = %d even and in [2, %d], hop = %d in [1, n_fft]", (long long)nn, n_fft,
                       RVCMI_GATE_MAX_NFFT, hop);
        plan_out[0] = p.Fn, plan_out[1] = p.K, plan_out[2] = p.head, plan_out[3] = p.back, plan_out[4] = p.advance, plan_out[5] = p.n_dirty;
    });
}

int rvcmi_glue_spectral_gate_ring_batch(int S, const float* x, int64_t x_stride, int64_t n, const float* xn, int64_t xn_stride, int64_t nn,
                                        float* out, int64_t out_stride, int64_t shift, int64_t tail, void* ring, size_t ring_bytes,
                                        int64_t ring_base, const uint8_t* mode, int any_cold, int n_fft, int hop, const double* window,
                                        const float* filter, int nf, int nt, int nonstationary, double n_std_thresh, double prop_decrease,
                                        void* scratch, size_t scratch_bytes, void* stream) {
    return guarded([&] {
        if (S < 1 || S > RVCMI_BANK_MAX_S) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: S = %d outside [1, %d]", S, RVCMI_BANK_MAX_S);
        if (!x || !xn || !out || !ring || !mode || !window || !scratch) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: null pointer");
        if (nonstationary) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: only the stationary gate with a noise signal is served");
        if (n_fft < 2 || n_fft > RVCMI_GATE_MAX_NFFT || (n_fft & 1))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: n_fft = %d must be even and in [2, %d]", n_fft, RVCMI_GATE_MAX_NFFT);
        if (hop < 1 || hop > n_fft) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: hop = %d outside [1, n_fft = %d]", hop, n_fft);
        if (n < 1 || nn < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: empty input");
        const int64_t Lout = (int64_t)hop * (n / hop);
        if (x_stride < n || xn_stride < nn || out_stride < Lout)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: row stride %lld / %lld / %lld shorter than the row %lld / %lld / %lld", (long long)x_stride,
                       (long long)xn_stride, (long long)out_stride, (long long)n, (long long)nn, (long long)Lout);
        if (filter && (nf < 1 || nt < 1 || (int64_t)nf * nt > (1 << 20)))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: smoothing filter %d x %d", nf, nt);
        if (!(prop_decrease >= 0.0 && prop_decrease <= 1.0)) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: prop_decrease outside [0, 1]");
        GateRingLayout g;
        GateRingPlan p;
        if (!gate_ring_layout(S, n, n_fft, hop, &g) || !gate_ring_plan(nn, n_fft, hop, shift, tail, &p))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: too many frames");
        const int tiles_n = any_cold ? p.tiles_cold : p.tiles_dirty;
        if (g.tiles_x + tiles_n > 65535) RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: too many frames");
        const size_t need_ring = gate_ring_bytes(S, nn, n_fft, hop);
        if (scratch_bytes < g.total || ring_bytes < need_ring)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "spectral_gate_ring: scratch of %zu bytes, %zu needed; cache of %zu bytes, %zu needed", scratch_bytes, g.total,
                       ring_bytes, need_ring);
        char* s = static_cast<char*>(scratch);
        double2* X = reinterpret_cast<double2*>(s + g.x);
        double2* R = static_cast<double2*>(ring);
        double* xmax = reinterpret_cast<double*>(s + g.xmax);
        double* thresh = reinterpret_cast<double*>(s + g.thresh);
        float* mraw = reinterpret_cast<float*>(s + g.mask);
        double* z = reinterpret_cast<double*>(s + g.frames);
        const int F = g.F, K = g.K, Fn = p.Fn;
        const int base = gate_ring_slot(ring_base, 0, Fn);
        const int lds = gate_lds_bytes(n_fft);
        hipStream_t st = (hipStream_t)stream;
        ensure_dyn_lds((const void*)k_gate_stft_ring, gate_lds_bytes(RVCMI_GATE_MAX_NFFT), g_attr_gate_stft_r);
        ensure_dyn_lds((const void*)k_gate_idft_ring, gate_lds_bytes(RVCMI_GATE_MAX_NFFT), g_attr_gate_idft_r);
        hipLaunchKernelGGL(k_gate_stft_ring, dim3((unsigned)((K + 63) / 64), (unsigned)(g.tiles_x + tiles_n), (unsigned)S), dim3(256), (size_t)lds, st,
                           x, x_stride, n, F, X, xn, xn_stride, nn, Fn, R, g.tiles_x, n_fft, hop, window, mode, p.head, p.back, base);
        hipLaunchKernelGGL(k_gate_stats_ring, dim3((unsigned)((K + 63) / 64), (unsigned)S), dim3(1024), 0, st, (const double2*)X, F,
                           (const double2*)R, Fn, K, n_std_thresh, xmax, thresh, base, mode);
        hipLaunchKernelGGL(k_gate_mask_ring, dim3((unsigned)((K + 255) / 256), (unsigned)F, (unsigned)S), dim3(256), 0, st, (const double2*)X, F, K,
                           (const double*)xmax, (const double*)thresh, 0, 0.0, 1.0, 1, (float)prop_decrease, mraw, mode);
        hipLaunchKernelGGL(k_gate_smooth_ring, dim3((unsigned)((K + 255) / 256), (unsigned)F, (unsigned)S), dim3(256), 0, st, X, F, K,
                           (const float*)mraw, filter, nf, nt, mode);
        hipLaunchKernelGGL(k_gate_idft_ring, dim3((unsigned)((n_fft + 63) / 64), (unsigned)g.tiles_x, (unsigned)S), dim3(256), (size_t)lds, st,
                           (const double2*)X, F, n_fft, window, z, mode);
        if (Lout > 0)
            hipLaunchKernelGGL(k_gate_ola_ring, dim3((unsigned)((Lout + 255) / 256), (unsigned)S), dim3(256), 0, st, (const double*)z, F, n_fft, hop,
                               window, Lout, out, out_stride, mode);
        HIP_CHECK(hipGetLastError());
    });
}

int rvcmi_glue_nr_stitch_batch(int S, const float* g, int64_t g_stride, int Lb, int64_t block_frame, const float* fade_in, const float* fade_out,
                               float* nr_buffer, int64_t nr_stride, float* denoise, int64_t den_stride, int64_t den_len, const float* den_prev,
                               int64_t prev_stride, const uint8_t* mode, void* stream) {
    return guarded([&] {
        if (S < 1 || S > RVCMI_BANK_MAX_S) RVCMI_FAIL(RVCMI_ERR_INVALID, "nr_stitch_batch: S = %d outside [1, %d]", S, RVCMI_BANK_MAX_S);
        if (!g || !fade_in || !fade_out || !nr_buffer || !denoise || !mode) RVCMI_FAIL(RVCMI_ERR_INVALID, "nr_stitch_batch: null pointer");
        if (Lb < 1 || block_frame < Lb || den_len < block_frame)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "nr_stitch_batch: 1 <= Lb = %d <= block_frame = %lld <= the rolling buffer's %lld samples", Lb,
                       (long long)block_frame, (long long)den_len);
        if (g_stride < block_frame + Lb || nr_stride < Lb || den_stride < den_len || (den_prev && prev_stride < den_len - block_frame))
            RVCMI_FAIL(RVCMI_ERR_INVALID, "nr_stitch_batch: a row stride is shorter than its row");
        if ((den_len + 255) / 256 > 0x7fffffff) RVCMI_FAIL(RVCMI_ERR_INVALID, "nr_stitch_batch: buffer too long");
        hipLaunchKernelGGL(k_nr_stitch_batch, dim3((unsigned)((den_len + 255) / 256), (unsigned)S), dim3(256), 0, (hipStream_t)stream, g, g_stride, Lb,
                           block_frame, fade_in, fade_out, nr_buffer, nr_stride, denoise, den_stride, den_len, den_prev, prev_stride, mode);
        HIP_CHECK(hipGetLastError());
    });
}

int rvcmi_glue_masked_write_batch(int S, float* dst, int64_t dst_stride, int64_t dst_len, const float* a, int64_t a_stride, int64_t off_a, int64_t na,
                                  const float* b, int64_t b_stride, int64_t off_b, int64_t nb, const uint8_t* mode, void* stream) {
    return guarded([&] {
        if (S < 1 || S > RVCMI_BANK_MAX_S) RVCMI_FAIL(RVCMI_ERR_INVALID, "masked_write_batch: S = %d outside [1, %d]", S, RVCMI_BANK_MAX_S);
        if (!dst || !a || !mode) RVCMI_FAIL(RVCMI_ERR_INVALID, "masked_write_batch: null pointer");
        if (!b) nb = 0, off_b = 0, b_stride = 0;
        if (dst_len < 1 || dst_stride < dst_len || na < 1 || nb < 0 || off_a < 0 || off_b < 0 || off_a > dst_len - na || off_b > dst_len - nb ||
            a_stride < na || b_stride < nb)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "masked_write_batch: a range leaves its row, or a row stride is shorter than its row");
        const int64_t nmax = na > nb ? na : nb;
        if ((nmax + 255) / 256 > 0x7fffffff) RVCMI_FAIL(RVCMI_ERR_INVALID, "masked_write_batch: row too long");
        hipLaunchKernelGGL(k_masked_write_batch, dim3((unsigned)((nmax + 255) / 256), (unsigned)S), dim3(256), 0, (hipStream_t)stream, dst, dst_stride, a,
                           a_stride, off_a, na, b, b_stride, off_b, nb, mode);
        HIP_CHECK(hipGetLastError());
    });
}

// np.multiply(f0, pow(2, f0_up_key / 12)) (rvc/f0/gen.py:18): the python expression in fp64 (an integral key: the same double as
// (double)int / 12.0).  The one place the factor is computed, for the single entries and for the descriptors of the ragged one.
double rvcmi_glue_f0_key_mul(double f0_up_key) {
    if (!std::isfinite(f0_up_key)) return std::nan("");
    return std::pow(2.0, f0_up_key / 12.0);
}

int rvcmi_glue_rmvpe_f0(const float* salience, int n, int nbins, float thred, int p_len, int f0_up_key, double* scratch,
                        int64_t* pitch, float* pitchf, void* stream) {
    return rvcmi_glue_rmvpe_f0_key(salience, n, nbins, thred, p_len, (double)f0_up_key, scratch, pitch, pitchf, stream);
}

int rvcmi_glue_rmvpe_f0_key(const float* salience, int n, int nbins, float thred, int p_len, double f0_up_key, double* scratch,
                            int64_t* pitch, float* pitchf, void* stream) {
    return guarded([&] {
        if (!std::isfinite(f0_up_key)) RVCMI_FAIL(RVCMI_ERR_INVALID, "rmvpe_f0: the key is not finite");
        if (!salience || !scratch || !pitch || !pitchf || n < 1 || nbins < 1 || p_len < 1)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "rmvpe_f0: bad argument");
        // work arrays: LDS when (n + p_len) doubles fit, else global (scratch in place + the pitch buffer) -- no length limit
        size_t smem = (size_t)(n + p_len) * sizeof(double);
        const bool in_lds = smem <= F0_LDS_BYTES;
        if (!in_lds) smem = 0;
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(k_rmvpe_decode, dim3((n + 3) / 4), dim3(256), 0, st, salience, n, nbins, thred, scratch);
        ensure_dyn_lds((const void*)k_f0_post, (int)F0_LDS_BYTES, g_attr_f0);
        // the host evaluates the scalars exactly as the reference does (python floats / math.log, rvc/f0/gen.py:18, 70-73)
        const double key_mul = rvcmi_glue_f0_key_mul(f0_up_key);
        const double mel_min = 1127.0 * std::log(1.0 + 50.0 / 700.0), mel_max = 1127.0 * std::log(1.0 + 1100.0 / 700.0);
        hipLaunchKernelGGL(k_f0_post, dim3(1), dim3(256), smem, st, scratch, n, p_len, 1, 1, key_mul, mel_min, mel_max, pitch, pitchf,
                           in_lds ? nullptr : scratch, in_lds ? nullptr : reinterpret_cast<double*>(pitch));
        HIP_CHECK(hipGetLastError());
    });
}

int rvcmi_glue_f0_post(const double* f0, int n, int f0_up_key, int64_t* pitch, float* pitchf, void* stream) {
    return rvcmi_glue_f0_post_key(f0, n, (double)f0_up_key, pitch, pitchf, stream);
}

int rvcmi_glue_f0_post_key(const double* f0, int n, double f0_up_key, int64_t* pitch, float* pitchf, void* stream) {
    return guarded([&] {
        if (!f0 || !pitch || !pitchf || n < 1 || !std::isfinite(f0_up_key)) RVCMI_FAIL(RVCMI_ERR_INVALID, "f0_post: bad argument");
        size_t smem = (size_t)(2 * n) * sizeof(double);
        const bool in_lds = smem <= F0_LDS_BYTES;
        if (!in_lds) smem = 0;
        ensure_dyn_lds((const void*)k_f0_post, (int)F0_LDS_BYTES, g_attr_f0);
        const double key_mul = rvcmi_glue_f0_key_mul(f0_up_key);
        const double mel_min = 1127.0 * std::log(1.0 + 50.0 / 700.0), mel_max = 1127.0 * std::log(1.0 + 1100.0 / 700.0);
        hipLaunchKernelGGL(k_f0_post, dim3(1), dim3(256), smem, (hipStream_t)stream, f0, n, n, 0, 0, key_mul, mel_min, mel_max, pitch, pitchf,
                           (double*)nullptr, in_lds ? nullptr : reinterpret_cast<double*>(pitch));
        HIP_CHECK(hipGetLastError());
    });
}

int rvcmi_glue_rmvpe_f0_ragged(const float* salience, int64_t R, int nbins, int nseq, const rvcmi_f0_row* rows_host, const rvcmi_f0_row* rows_dev,
                               float thred, double* scratch, int64_t* pitch, float* pitchf, int64_t out_len, void* stream) {
    return guarded([&] {
        if (!salience || !rows_host || !rows_dev || !scratch || !pitch || !pitchf || nbins < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "rmvpe_f0_ragged: bad argument");
        F0RowsPlan plan;
        if (const char* why = f0_rows_check(rows_host, nseq, R, out_len, &plan)) RVCMI_FAIL(RVCMI_ERR_INVALID, "rmvpe_f0_ragged: %s", why);
        hipStream_t st = (hipStream_t)stream;
        // launch 1: the decode is per frame and knows nothing of items; rows between items decode to values nobody reads
        hipLaunchKernelGGL(k_rmvpe_decode, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, salience, (int)R, nbins, thred, scratch);
        ensure_dyn_lds((const void*)k_f0_post_ragged, (int)F0_LDS_BYTES, g_attr_f0_ragged);
        const double mel_min = 1127.0 * std::log(1.0 + 50.0 / 700.0), mel_max = 1127.0 * std::log(1.0 + 1100.0 / 700.0);
        // launch 2: one block per item
        hipLaunchKernelGGL(k_f0_post_ragged, dim3((unsigned)nseq), dim3(256), plan.lds_doubles * sizeof(double), st, scratch, R, rows_dev,
                           plan.use_global ? 1 : 0, (int)plan.lds_doubles, mel_min, mel_max, pitch, pitchf, out_len);
        HIP_CHECK(hipGetLastError());
    });
}

int rvcmi_glue_scale_int16_range(float* audio, int64_t n, float* scratch256, void* stream) {
    return guarded([&] {
        if (!audio || !scratch256 || n < 0) RVCMI_FAIL(RVCMI_ERR_INVALID, "scale_int16_range: bad argument");
        if (!n) return;
        const int nb = (int)std::min<int64_t>(256, (n + 255) / 256);
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(k_absmax_partial, dim3(nb), dim3(256), 0, st, audio, n, scratch256);
        hipLaunchKernelGGL(k_scale_int16_range, dim3(nb), dim3(256), 0, st, audio, n, scratch256, nb);
        HIP_CHECK(hipGetLastError());
    });
}

// ---- the block DSP: ONE recipe per step, for a bank of S sessions (session index in the grid, every per-session array with a row
// stride; glue_kernels.hpp).  The single-stream entry of a step is the same recipe at S = 1 with strides equal to the row lengths;
// `who` is the entry's name in its messages. ---------------------------------------------------------------------------------------------

static void check_sessions(const char* who, int S) {
    if (S < 1 || S > RVCMI_BANK_MAX_S) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: S = %d outside [1, %d]", who, S, RVCMI_BANK_MAX_S);
}

static void expand_protect_rows(const char* who, int S, const float* feats, int64_t nq, int d, int reps, const float* pitchf, float protect,
                                int64_t p_len, float* out, hipStream_t st) {
    check_sessions(who, S);
    if (!feats || !out || nq < 0 || d < 1 || reps < 1 || p_len < 0 || p_len > nq * reps)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: bad argument (nq %lld d %d reps %d p_len %lld)", who, (long long)nq, d, reps, (long long)p_len);
    if (!nq || !p_len) return;
    hipLaunchKernelGGL(k_blend_expand_batch, dim3((unsigned)nq, (unsigned)S), dim3(256), 0, st, feats, nullptr, nullptr, nullptr, d, 0, (int64_t)0,
                       0.f, 0.f, nullptr, 0, nq, (int64_t)0, pitchf, protect, p_len, reps, out);
    HIP_CHECK(hipGetLastError());
}

int rvcmi_glue_expand_protect(const float* feats, int64_t nq, int d, int reps, const float* pitchf, float protect, int64_t p_len,
                              float* out, void* stream) {
    return guarded([&] { expand_protect_rows("expand_protect", 1, feats, nq, d, reps, pitchf, protect, p_len, out, (hipStream_t)stream); });
}

// The bank's retrieval-free expansion (index_rate == 0 / no index).
int rvcmi_glue_expand_protect_batch(int S, const float* feats, int64_t nq, int d, int reps, const float* pitchf, float protect, int64_t p_len,
                                    float* out, void* stream) {
    return guarded([&] { expand_protect_rows("expand_protect_batch", S, feats, nq, d, reps, pitchf, protect, p_len, out, (hipStream_t)stream); });
}

static void resample_rows(const char* who, int S, const float* x, int64_t x_stride, int64_t n, const float* kernel, int orig, int new_, int K,
                          int width, float* out, int64_t out_stride, int64_t n_out, hipStream_t st) {
    check_sessions(who, S);
    if (!x || !kernel || !out || n < 1 || orig < 1 || new_ < 1 || K < 1 || width < 0 || n_out < 0) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: bad argument", who);
    if (x_stride < n || out_stride < n_out)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: row stride %lld / %lld shorter than the row %lld / %lld", who, (long long)x_stride, (long long)out_stride,
                   (long long)n, (long long)n_out);
    if (n_out == 0) return;
    hipLaunchKernelGGL(k_resample_poly_batch, dim3((unsigned)((n_out + 255) / 256), (unsigned)S), dim3(256), 0, st, x, x_stride, n, kernel, orig, new_,
                       K, width, out, out_stride, n_out);
    HIP_CHECK(hipGetLastError());
}

int rvcmi_glue_resample_poly(const float* x, int64_t n, const float* kernel, int orig, int new_, int K, int width, float* out, int64_t n_out,
                             void* stream) {
    return guarded([&] { resample_rows("resample", 1, x, n, n, kernel, orig, new_, K, width, out, n_out, n_out, (hipStream_t)stream); });
}

int rvcmi_glue_resample_poly_batch(int S, const float* x, int64_t x_stride, int64_t n, const float* kernel, int orig, int new_, int K, int width,
                                   float* out, int64_t out_stride, int64_t n_out, void* stream) {
    return guarded([&] {
        resample_rows("resample_batch", S, x, x_stride, n, kernel, orig, new_, K, width, out, out_stride, n_out, (hipStream_t)stream);
    });
}

int rvcmi_glue_resample_poly_ragged(int S, const float* x, int64_t x_stride, int64_t n_max, const float* kernels, int64_t kernels_floats,
                                    const rvcmi_resample_row* rows, float* out, int64_t out_stride, int64_t n_out, void* stream) {
    return guarded([&] {
        const char* who = "resample_ragged";
        check_sessions(who, S);
        if (!x || !kernels || !rows || !out || n_max < 1 || kernels_floats < 1 || n_out < 0) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: bad argument", who);
        if (x_stride < n_max || out_stride < n_out)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: row stride %lld / %lld shorter than the row %lld / %lld", who, (long long)x_stride, (long long)out_stride,
                       (long long)n_max, (long long)n_out);
        if (n_out == 0) return;
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(k_resample_poly_ragged, dim3((unsigned)((n_out + 255) / 256), (unsigned)S), dim3(256), 0, st, x, x_stride, kernels,
                           kernels_floats, rows, n_max, out, out_stride, n_out);
        HIP_CHECK(hipGetLastError());
    });
}

// What both stitches check, in this order (rest_ok: the caller's further pointers are non-null); the LDS limit (2 Lb + Ls floats of
// dynamic LDS <= 150 KB, + 2 KB static) comes last, after the phase vocoder's size limit.
static void check_sola_rows(const char* who, int S, const float* infer_wav, int64_t wav_stride, int64_t n, const float* sola_buffer, int64_t buf_stride,
                            int Lb, int Ls, const float* fade_in, const float* fade_out, int block_frame, const float* out_block, int64_t out_stride,
                            bool rest_ok) {
    check_sessions(who, S);
    if (!infer_wav || !sola_buffer || !fade_in || !fade_out || !out_block || !rest_ok || Lb < 1 || Ls < 0 || block_frame < 1)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: bad argument", who);
    if ((int64_t)Ls + block_frame + Lb > n)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: chunk of %lld samples is shorter than search %d + block %d + buffer %d", who, (long long)n, Ls, block_frame, Lb);
    if (wav_stride < n || buf_stride < Lb || out_stride < block_frame)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: a row stride (%lld, %lld, %lld) is shorter than its row (%lld, %d, %d)", who, (long long)wav_stride,
                   (long long)buf_stride, (long long)out_stride, (long long)n, Lb, block_frame);
}
static size_t sola_lds_bytes(const char* who, int Lb, int Ls) {
    const size_t smem = (size_t)(2 * (int64_t)Lb + Ls) * sizeof(float);
    if (smem > 150 * 1024) RVCMI_FAIL(RVCMI_ERR_NOMEM, "%s: buffer + search window too large", who);
    return smem;
}

// One block per session; offset_out [S] contiguous, or null.
static void sola_rows(const char* who, int S, const float* infer_wav, int64_t wav_stride, int64_t n, float* sola_buffer, int64_t buf_stride, int Lb,
                      int Ls, const float* fade_in, const float* fade_out, int block_frame, float* out_block, int64_t out_stride, int* offset_out,
                      hipStream_t st) {
    check_sola_rows(who, S, infer_wav, wav_stride, n, sola_buffer, buf_stride, Lb, Ls, fade_in, fade_out, block_frame, out_block, out_stride, true);
    const size_t smem = sola_lds_bytes(who, Lb, Ls);
    ensure_dyn_lds((const void*)k_sola_batch, 150 * 1024, g_attr_sola);
    hipLaunchKernelGGL(k_sola_batch, dim3((unsigned)S), dim3(256), smem, st, infer_wav, wav_stride, sola_buffer, buf_stride, Lb, Ls, fade_in, fade_out,
                       block_frame, out_block, out_stride, offset_out);
    HIP_CHECK(hipGetLastError());
}

int rvcmi_glue_sola(const float* infer_wav, int64_t n, float* sola_buffer, int Lb, int Ls, const float* fade_in, const float* fade_out,
                    int block_frame, float* out_block, int* offset_out, void* stream) {
    return guarded([&] {
        sola_rows("sola", 1, infer_wav, n, n, sola_buffer, Lb, Lb, Ls, fade_in, fade_out, block_frame, out_block, block_frame, offset_out,
                  (hipStream_t)stream);
    });
}

int rvcmi_glue_sola_batch(int S, const float* infer_wav, int64_t wav_stride, int64_t n, float* sola_buffer, int64_t buf_stride, int Lb, int Ls,
                          const float* fade_in, const float* fade_out, int block_frame, float* out_block, int64_t out_stride, int* offset_out,
                          void* stream) {
    return guarded([&] {
        sola_rows("sola_batch", S, infer_wav, wav_stride, n, sola_buffer, buf_stride, Lb, Ls, fade_in, fade_out, block_frame, out_block, out_stride,
                  offset_out, (hipStream_t)stream);
    });
}

// The phase vocoder's two launches on device-resident rows: out row s <- phase_vocoder(a row s, b row s at its offset).  b_off: the rows'
// device offsets into b, off_stride ints apart, or null (offset 0; off_stride = 0 then).  bins: 3 (n/2 + 1) doubles per row.  out may not
// alias a or b.
static void launch_pv_rows(int S, const float* a, int64_t a_stride, const float* b, int64_t b_stride, const int* b_off, int64_t off_stride,
                           const float* fade_out, const float* fade_in, int n, double* bins, int64_t bins_stride, float* out, int64_t out_stride,
                           hipStream_t st) {
    const int nb = n / 2 + 1;
    ensure_dyn_lds((const void*)k_pv_spectrum_batch, 32 * RVCMI_PV_MAX_N, g_attr_pv_spec);
    ensure_dyn_lds((const void*)k_pv_synth_batch, 8 * (3 * (RVCMI_PV_MAX_N / 2 + 1) + 16 * 64), g_attr_pv_synth);
    hipLaunchKernelGGL(k_pv_spectrum_batch, dim3((unsigned)std::min(256, (nb + 3) / 4), (unsigned)S), dim3(256), (size_t)32 * n, st, a, a_stride, b,
                       b_stride, b_off, off_stride, fade_out, fade_in, n, bins, bins_stride);
    hipLaunchKernelGGL(k_pv_synth_batch, dim3((unsigned)((n + 63) / 64), (unsigned)S), dim3(1024), (size_t)8 * (3 * nb + 16 * 64), st, a, a_stride, b,
                       b_stride, b_off, off_stride, fade_out, fade_in, n, (const double*)bins, bins_stride, out, out_stride);
}

int rvcmi_glue_phase_vocoder(const float* a, const float* b, const float* fade_out, const float* fade_in, int n, float* out, double* scratch,
                             void* stream) {
    return guarded([&] {
        if (!a || !b || !fade_out || !fade_in || !out || !scratch || n < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "phase_vocoder: bad argument");
        if (n > RVCMI_PV_MAX_N) RVCMI_FAIL(RVCMI_ERR_INVALID, "phase_vocoder: n = %d exceeds %d", n, RVCMI_PV_MAX_N);
        launch_pv_rows(1, a, n, b, n, nullptr, 0, fade_out, fade_in, n, scratch, 3 * (n / 2 + 1), out, n, (hipStream_t)stream);
        HIP_CHECK(hipGetLastError());
    });
}

// Four launches: search -> pv spectrum -> pv synthesis (into scratch) -> stitch.
// scratch: S slices of P = 3 nb + Lb/2 + 1 doubles (nb = Lb/2 + 1), session s at s * P, each laid out as
//   bins [3 nb] doubles | pv result [Lb] floats | offset (one int, used when offset_out is null)
static void sola_pv_rows(const char* who, int S, const float* infer_wav, int64_t wav_stride, int64_t n, float* sola_buffer, int64_t buf_stride, int Lb,
                         int Ls, const float* fade_in, const float* fade_out, int block_frame, float* out_block, int64_t out_stride, int* offset_out,
                         double* scratch, hipStream_t st) {
    check_sola_rows(who, S, infer_wav, wav_stride, n, sola_buffer, buf_stride, Lb, Ls, fade_in, fade_out, block_frame, out_block, out_stride,
                    scratch != nullptr);
    if (Lb > RVCMI_PV_MAX_N) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: cross-fade buffer of %d samples exceeds %d", who, Lb, RVCMI_PV_MAX_N);
    const size_t smem = sola_lds_bytes(who, Lb, Ls);
    const int nb = Lb / 2 + 1;
    const int64_t per = 3 * (int64_t)nb + Lb / 2 + 1;
    float* pv = reinterpret_cast<float*>(scratch + 3 * nb);
    int* off = offset_out ? offset_out : reinterpret_cast<int*>(pv + Lb);
    const int64_t off_stride = offset_out ? 1 : 2 * per;  // in ints
    ensure_dyn_lds((const void*)k_sola_search_batch, 150 * 1024, g_attr_sola_search);
    hipLaunchKernelGGL(k_sola_search_batch, dim3((unsigned)S), dim3(256), smem, st, infer_wav, wav_stride, (const float*)sola_buffer, buf_stride, Lb, Ls,
                       off, off_stride);
    // a = the session's sola_buffer row, b = its chunk at its own offset, which never leaves the device
    launch_pv_rows(S, sola_buffer, buf_stride, infer_wav, wav_stride, off, off_stride, fade_out, fade_in, Lb, scratch, per, pv, 2 * per, st);
    hipLaunchKernelGGL(k_sola_pv_stitch_batch, dim3((unsigned)((block_frame + Lb + 255) / 256), (unsigned)S), dim3(256), 0, st, infer_wav, wav_stride,
                       (const int*)off, off_stride, (const float*)pv, 2 * per, Lb, block_frame, out_block, out_stride, sola_buffer, buf_stride);
    HIP_CHECK(hipGetLastError());
}

int rvcmi_glue_sola_pv(const float* infer_wav, int64_t n, float* sola_buffer, int Lb, int Ls, const float* fade_in, const float* fade_out,
                       int block_frame, float* out_block, int* offset_out, double* scratch, void* stream) {
    return guarded([&] {
        sola_pv_rows("sola_pv", 1, infer_wav, n, n, sola_buffer, Lb, Lb, Ls, fade_in, fade_out, block_frame, out_block, block_frame, offset_out, scratch,
                     (hipStream_t)stream);
    });
}

int rvcmi_glue_sola_pv_batch(int S, const float* infer_wav, int64_t wav_stride, int64_t n, float* sola_buffer, int64_t buf_stride, int Lb, int Ls,
                             const float* fade_in, const float* fade_out, int block_frame, float* out_block, int64_t out_stride, int* offset_out,
                             double* scratch, void* stream) {
    return guarded([&] {
        sola_pv_rows("sola_pv_batch", S, infer_wav, wav_stride, n, sola_buffer, buf_stride, Lb, Ls, fade_in, fade_out, block_frame, out_block, out_stride,
                     offset_out, scratch, (hipStream_t)stream);
    });
}

// scratch [S][2][nf] floats, nf = 1 + n / zc: session s's input envelope, then its output envelope.
static void envelope_mix_rows(const char* who, int S, const float* input, int64_t in_stride, float* wav, int64_t wav_stride, int64_t n, int zc,
                              double rate, float* scratch, hipStream_t st) {
    check_sessions(who, S);
    if (!input || !wav || !scratch || n < 1 || zc < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: bad argument", who);
    if (in_stride < n || wav_stride < n)
        RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: row stride %lld / %lld shorter than the row %lld", who, (long long)in_stride, (long long)wav_stride,
                   (long long)n);
    const int64_t nf64 = 1 + n / zc;
    if (nf64 > (1 << 30)) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: too many frames", who);
    const int nf = (int)nf64;
    hipLaunchKernelGGL(k_frame_rms_batch, dim3(nf, (unsigned)S), dim3(256), 0, st, input, in_stride, n, 4 * zc, zc, nf, scratch, (int64_t)2 * nf);
    hipLaunchKernelGGL(k_frame_rms_batch, dim3(nf, (unsigned)S), dim3(256), 0, st, (const float*)wav, wav_stride, n, 4 * zc, zc, nf, scratch + nf,
                       (int64_t)2 * nf);
    // torch.pow(rms1 / rms2, torch.tensor(1 - rate)): the exponent is the python double rounded to float32
    const float e = (float)(1.0 - rate);
    hipLaunchKernelGGL(k_envelope_mix_batch, dim3((unsigned)((n + 255) / 256), (unsigned)S), dim3(256), 0, st, wav, wav_stride, n,
                       (const float*)scratch, nf, e);
    HIP_CHECK(hipGetLastError());
}

int rvcmi_glue_envelope_mix(const float* input, float* wav, int64_t n, int zc, double rate, float* scratch, void* stream) {
    return guarded([&] { envelope_mix_rows("envelope_mix", 1, input, n, wav, n, n, zc, rate, scratch, (hipStream_t)stream); });
}

int rvcmi_glue_envelope_mix_batch(int S, const float* input, int64_t in_stride, float* wav, int64_t wav_stride, int64_t n, int zc, double rate,
                                  float* scratch, void* stream) {
    return guarded([&] { envelope_mix_rows("envelope_mix_batch", S, input, in_stride, wav, wav_stride, n, zc, rate, scratch, (hipStream_t)stream); });
}

size_t rvcmi_glue_input_gate_scratch_floats(int zc, int blk) {
    if (zc < 1 || blk < zc || blk % zc || zc > (1 << 20) || blk > (1 << 28)) return 0;
    return (size_t)4 * zc + blk + blk / zc + 5;
}

// Per session in scratch: x = rms_buffer | block [4 zc + blk], then its blk / zc + 5 frame RMS values (the gate reads frames 2 ..).
int rvcmi_glue_input_gate_batch(int S, const float* block, int64_t block_stride, float* rms_buffer, int64_t rms_stride, float* dst,
                                int64_t dst_stride, int zc, int blk, float cut_a, float cut_b, float* scratch, void* stream) {
    return guarded([&] {
        const char* who = "input_gate_batch";
        check_sessions(who, S);
        if (!block || !rms_buffer || !dst || !scratch) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: null pointer", who);
        const size_t per = rvcmi_glue_input_gate_scratch_floats(zc, blk);
        if (!per) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: a block of %d samples must be a whole number (>= 1) of hops of zc = %d >= 1 samples", who, blk, zc);
        if (cut_a != cut_a || cut_b != cut_b || cut_a < 0.f || cut_b < 0.f) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: the cutoffs are RMS values (>= 0, not NaN)", who);
        if (block_stride < blk || rms_stride < 4 * (int64_t)zc || dst_stride < (int64_t)blk + 2 * zc)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: a row stride (%lld, %lld, %lld) is shorter than its row (%d, %d, %d)", who, (long long)block_stride,
                       (long long)rms_stride, (long long)dst_stride, blk, 4 * zc, blk + 2 * zc);
        const int nx = 4 * zc + blk, nfr = blk / zc + 5, nout = std::max(blk + 2 * zc, 4 * zc);
        float* rms = scratch + nx;
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(k_gate_stage_batch, dim3((unsigned)((nx + 255) / 256), (unsigned)S), dim3(256), 0, st, block, block_stride,
                           (const float*)rms_buffer, rms_stride, zc, blk, scratch, (int64_t)per);
        hipLaunchKernelGGL(k_frame_rms_batch, dim3((unsigned)nfr, (unsigned)S), dim3(256), 0, st, (const float*)scratch, (int64_t)per, (int64_t)nx,
                           4 * zc, zc, nfr, rms, (int64_t)per);
        hipLaunchKernelGGL(k_input_gate_batch, dim3((unsigned)((nout + 255) / 256), (unsigned)S), dim3(256), 0, st, (const float*)scratch, (int64_t)per,
                           (const float*)rms, (int64_t)per, zc, blk, cut_a, cut_b, dst, dst_stride, rms_buffer, rms_stride);
        HIP_CHECK(hipGetLastError());
    });
}

// envelope_mix_rows with the exponent and an on / off flag per session (session_rows.hpp checks the host copy; the kernels read the device
// copy).  The same scratch layout; a session that is off has neither its wav row nor its scratch written.
int rvcmi_glue_envelope_mix_sessions(int S, const float* input, int64_t in_stride, float* wav, int64_t wav_stride, int64_t n, int zc,
                                     const rvcmi_session_mix* sess_host, const rvcmi_session_mix* sess_dev, float* scratch, void* stream) {
    return guarded([&] {
        const char* who = "envelope_mix_sessions";
        int active = 0;
        if (const char* why = session_mix_check(sess_host, S, &active)) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: %s", who, why);
        if (!input || !wav || !scratch || !sess_dev || n < 1 || zc < 1) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: bad argument", who);
        if (in_stride < n || wav_stride < n)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: row stride %lld / %lld shorter than the row %lld", who, (long long)in_stride, (long long)wav_stride,
                       (long long)n);
        const int64_t nf64 = 1 + n / zc;
        if (nf64 > (1 << 30)) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: too many frames", who);
        if (!active) return;
        const int nf = (int)nf64;
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(k_frame_rms_sessions<rvcmi_session_mix>, dim3(nf, (unsigned)S), dim3(256), 0, st, input, in_stride, n, 4 * zc, zc, nf,
                           scratch, (int64_t)2 * nf, sess_dev);
        hipLaunchKernelGGL(k_frame_rms_sessions<rvcmi_session_mix>, dim3(nf, (unsigned)S), dim3(256), 0, st, (const float*)wav, wav_stride, n, 4 * zc,
                           zc, nf, scratch + nf, (int64_t)2 * nf, sess_dev);
        hipLaunchKernelGGL(k_envelope_mix_sessions, dim3((unsigned)((n + 255) / 256), (unsigned)S), dim3(256), 0, st, wav, wav_stride, n,
                           (const float*)scratch, nf, sess_dev);
        HIP_CHECK(hipGetLastError());
    });
}

// rvcmi_glue_input_gate_batch with the cutoffs and an on / off flag per session; the same scratch layout per session.
int rvcmi_glue_input_gate_sessions(int S, const float* block, int64_t block_stride, float* rms_buffer, int64_t rms_stride, float* dst,
                                   int64_t dst_stride, int zc, int blk, const rvcmi_session_gate* sess_host, const rvcmi_session_gate* sess_dev,
                                   float* scratch, void* stream) {
    return guarded([&] {
        const char* who = "input_gate_sessions";
        int active = 0;
        if (const char* why = session_gate_check(sess_host, S, &active)) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: %s", who, why);
        if (!block || !rms_buffer || !dst || !scratch || !sess_dev) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: null pointer", who);
        const size_t per = rvcmi_glue_input_gate_scratch_floats(zc, blk);
        if (!per) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: a block of %d samples must be a whole number (>= 1) of hops of zc = %d >= 1 samples", who, blk, zc);
        if (block_stride < blk || rms_stride < 4 * (int64_t)zc || dst_stride < (int64_t)blk + 2 * zc)
            RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: a row stride (%lld, %lld, %lld) is shorter than its row (%d, %d, %d)", who, (long long)block_stride,
                       (long long)rms_stride, (long long)dst_stride, blk, 4 * zc, blk + 2 * zc);
        const int nx = 4 * zc + blk, nfr = blk / zc + 5, nout = std::max(blk + 2 * zc, 4 * zc);
        float* rms = scratch + nx;
        hipStream_t st = (hipStream_t)stream;
        if (active) {
            hipLaunchKernelGGL(k_gate_stage_sessions, dim3((unsigned)((nx + 255) / 256), (unsigned)S), dim3(256), 0, st, block, block_stride,
                               (const float*)rms_buffer, rms_stride, zc, blk, scratch, (int64_t)per, sess_dev);
            hipLaunchKernelGGL(k_frame_rms_sessions<rvcmi_session_gate>, dim3((unsigned)nfr, (unsigned)S), dim3(256), 0, st, (const float*)scratch,
                               (int64_t)per, (int64_t)nx, 4 * zc, zc, nfr, rms, (int64_t)per, sess_dev);
        }
        hipLaunchKernelGGL(k_input_gate_sessions, dim3((unsigned)((nout + 255) / 256), (unsigned)S), dim3(256), 0, st, (const float*)scratch,
                           (int64_t)per, (const float*)rms, (int64_t)per, zc, blk, sess_dev, block, block_stride, dst, dst_stride, rms_buffer,
                           rms_stride);
        HIP_CHECK(hipGetLastError());
    });
}

int rvcmi_glue_change_rms(const float* data1, int64_t n1, int sr1, float* data2, int64_t n2, int sr2, float rate, float* scratch,
                          void* stream) {
    return guarded([&] {
        if (!data1 || !data2 || !scratch || n1 < 1 || n2 < 1 || sr1 < 2 || sr2 < 2) RVCMI_FAIL(RVCMI_ERR_INVALID, "change_rms: bad argument");
        const int h1 = sr1 / 2, h2 = sr2 / 2;
        const int nf1 = 1 + (int)(n1 / h1), nf2 = 1 + (int)(n2 / h2);
        hipStream_t st = (hipStream_t)stream;
        hipLaunchKernelGGL(k_frame_rms_batch, dim3(nf1, 1), dim3(256), 0, st, data1, n1, n1, 2 * h1, h1, nf1, scratch, (int64_t)nf1);
        hipLaunchKernelGGL(k_frame_rms_batch, dim3(nf2, 1), dim3(256), 0, st, (const float*)data2, n2, n2, 2 * h2, h2, nf2, scratch + nf1,
                           (int64_t)nf2);
        // torch.pow(rms, torch.tensor(1 - rate)): the exponent is the python double rounded to float32
        const float e1 = (float)(1.0 - (double)rate), e2 = (float)((double)rate - 1.0);
        hipLaunchKernelGGL(k_change_rms, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, data2, n2, scratch, nf1, scratch + nf1, nf2, e1, e2);
        HIP_CHECK(hipGetLastError());
    });
}

}  // extern "C"
