// The realtime GUI's noise reduction: TorchGate (infer/modules/gui/torchgate.py, utils.py), the spectral gate that gui.py
// builds as TorchGate(sr, n_fft = 4 zc, prop_decrease = 0.9) and calls on the input (gui.py:974-992) and on the output
// (gui.py:1015-1022).  Five launches on the caller's stream:
//
//   k_gate_stft     windowed STFT of x and of the noise signal xn (torch.stft, center=True, zero padding, onesided)
//   k_gate_stats    per (row, bin): amp_to_db, its max over frames, and the noise threshold mean + n_std * std (unbiased);
//                   16 waves per 64 bins split the frames
//   k_gate_mask     per (row, frame, bin): the stationary (X_db > thresh) or non-stationary (moving-mean sigmoid) mask,
//                   prop_decrease * (mask.float() - 1) + 1 in fp32
//   k_gate_smooth   conv2d(mask, smoothing_filter, padding="same") over (bin, frame) in fp32, in torch's CPU accumulation
//                   order; Y = X * mask in place
//   k_gate_idft     per frame: window * irfft(Y)          k_gate_ola: overlap-add / sum of squared windows, centre trim
//
// The transforms are direct DFTs in fp64 with an LDS table of the n twiddles and exact integer argument reduction (k m) mod n,
// as k_pv_spectrum_batch does: any even n_fft <= 4096 (the GUI's are 880..1920, none a power of two), no plan, no workspace beyond
// the spectra.  A block owns 64 bins (or 64 samples) of GATE_FT consecutive frames; its 4 waves split the inner sum, staged
// through LDS in chunks, and add their partial sums in a fixed order, so every output depends only on its own row's data.
//
// Every kernel is a thin __global__ around a __device__ body.  The k_gate_*_ring kernels call the same bodies for a bank of sessions
// (rvcmi_glue_spectral_gate_ring_batch): rows with strides, a per-session mode byte, and the noise spectra in a rolling cache of which
// only the frames the last block rewrote are transformed again (gate_ring.hpp has the rule) -- the same instructions per frame, so the
// same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "exact_fp.hpp"
#include <stdint.h>

namespace rvcmi {

#define RVCMI_GATE_MAX_NFFT 4096
constexpr int GATE_FT = 8;       // frames per block
constexpr int GATE_CHUNK = 512;  // samples (forward) or bins (inverse) staged per LDS round

// dynamic LDS of k_gate_stft / k_gate_idft: the twiddle table [n] double2 + the staged chunk, 32 KB (later the waves' partial sums)
__host__ __device__ constexpr int gate_lds_bytes(int n) { return 16 * n + 8 * GATE_CHUNK * GATE_FT; }

__device__ __forceinline__ void gate_twiddles(double2* tw, int n) {
    for (int m = threadIdx.x; m < n; m += 256) {
        double s, c;
        sincospi((double)(2 * m) / (double)n, &s, &c);
        tw[m] = make_double2(c, s);
    }
}

__device__ __forceinline__ double gate_db(double2 v) {
    // amp_to_db (utils.py:5-25) before its clamp: 20 log10(|X| + float64 eps)
    return 20.0 * log10(sqrt(v.x * v.x + v.y * v.y) + 2.220446049250313e-16);
}

// Forward: spec[b][f][k] = sum_m win[m] xpad[f hop + m] e^{-2 pi i k m / n}, xpad = x zero-padded by n/2 on both sides.
// One tile: work items f0 .. f0 + GATE_FT - 1 of the row's F.  Item j is frame j, stored at row j of sp; with RING it is logical
// frame src = j < head ? j : j + skip, stored at row (base + src) % mod of a rolling cache (0 <= base < mod).  Every frame is summed
// in an order that depends on neither its slot in the tile nor the mapping, so a frame's spectrum is a function of its samples alone.
struct GateFrameMap {
    int head, skip, base, mod;
};
template <bool RING>
__device__ __forceinline__ void gate_stft_tile(const float* __restrict__ x, int64_t L, int F, double2* __restrict__ sp, int f0, int n, int hop,
                                               const double* __restrict__ win, double* gate_sm, GateFrameMap map) {
    double2* tw = reinterpret_cast<double2*>(gate_sm);  // [n]
    double* xs = gate_sm + 2 * n;                        // [GATE_CHUNK][GATE_FT]; then the partial sums
    const int K = n / 2 + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane;
    const int kk = k < K ? k : 0;
    gate_twiddles(tw, n);
    double re[GATE_FT], im[GATE_FT];
#pragma unroll
    for (int f = 0; f < GATE_FT; ++f) re[f] = im[f] = 0.0;
    for (int c0 = 0; c0 < n; c0 += GATE_CHUNK) {
        __syncthreads();
        for (int e = threadIdx.x; e < GATE_CHUNK * GATE_FT; e += 256) {
            const int c = e / GATE_FT, f = e % GATE_FT, m = c0 + c;
            double v = 0.0;
            if (m < n && f0 + f < F) {
                int src = f0 + f;
                if (RING && src >= map.head) src += map.skip;
                const int64_t p = (int64_t)src * hop + m - n / 2;
                if (p >= 0 && p < L) v = win[m] * (double)x[p];
            }
            xs[e] = v;
        }
        __syncthreads();
        const int mb = c0 + w * (GATE_CHUNK / 4);
        const int me = min(mb + GATE_CHUNK / 4, n);
        int idx = (int)(((int64_t)kk * mb) % n);
        for (int m = mb; m < me; ++m) {
            const double2 t = tw[idx];
            const double* xv = xs + (m - c0) * GATE_FT;
#pragma unroll
            for (int f = 0; f < GATE_FT; ++f) {
                re[f] += xv[f] * t.x;
                im[f] -= xv[f] * t.y;
            }
            idx += kk;
            if (idx >= n) idx -= n;
        }
    }
    __syncthreads();
    double2* part = reinterpret_cast<double2*>(xs);  // [3][GATE_FT][64]: waves 1..3
    if (w > 0) {
#pragma unroll
        for (int f = 0; f < GATE_FT; ++f) part[((w - 1) * GATE_FT + f) * 64 + lane] = make_double2(re[f], im[f]);
    }
    __syncthreads();
    if (w == 0 && k < K) {
#pragma unroll
        for (int f = 0; f < GATE_FT; ++f) {
            double r = re[f], i = im[f];
            for (int q = 0; q < 3; ++q) {
                const double2 v = part[(q * GATE_FT + f) * 64 + lane];
                r += v.x;
                i += v.y;
            }
            if (f0 + f < F) {
                int dst = f0 + f;
                if (RING) {
                    if (dst >= map.head) dst += map.skip;
                    dst += map.base;
                    if (dst >= map.mod) dst -= map.mod;
                }
                sp[(int64_t)dst * K + k] = make_double2(r, i);
            }
        }
    }
}

// grid (ceil(K / 64), tiles_a + tiles_b, B): the first tiles_a frame tiles are signal a, the rest signal b (the noise).
static __global__ void __launch_bounds__(256) k_gate_stft(const float* __restrict__ xa, int64_t La, int Fa, double2* __restrict__ spa,
                                                          const float* __restrict__ xb, int64_t Lb, int Fb, double2* __restrict__ spb,
                                                          int tiles_a, int n, int hop, const double* __restrict__ win) {
    extern __shared__ __attribute__((aligned(16))) double gate_sm[];
    const int K = n / 2 + 1;
    const bool is_a = (int)blockIdx.y < tiles_a;
    const float* x = is_a ? xa : xb;
    const int64_t L = is_a ? La : Lb;
    const int F = is_a ? Fa : Fb;
    double2* sp = is_a ? spa : spb;
    const int f0 = (is_a ? (int)blockIdx.y : (int)blockIdx.y - tiles_a) * GATE_FT;
    gate_stft_tile<false>(x + (int64_t)blockIdx.z * L, L, F, sp + (int64_t)blockIdx.z * F * K, f0, n, hop, win, gate_sm, GateFrameMap{0, 0, 0, 0});
}

// The same for a bank of sessions whose noise spectra live in a rolling cache (rvcmi_glue_spectral_gate_ring_batch, gate_ring.hpp).
// Rows carry strides.  mode[s] == 0: the session's blocks leave at once.  1 (warm): of the noise frames only the n_dirty dirty ones --
// logical frames [0, head) and [back, Fn), packed densely into tiles -- are transformed.  2 (cold): all Fn.  Logical frame f is stored
// at row (base + f) % Fn of the session's cache.  grid (ceil(K / 64), tiles_a + tiles_n, S) with tiles_n the cold tile count when any
// session is cold, else the dirty one; a warm session's surplus tiles leave at once.  Every exit is uniform per block and precedes the
// first barrier.
static __global__ void __launch_bounds__(256) k_gate_stft_ring(const float* __restrict__ x, int64_t x_stride, int64_t L, int F,
                                                               double2* __restrict__ spx, const float* __restrict__ xn, int64_t xn_stride,
                                                               int64_t Ln, int Fn, double2* __restrict__ ring, int tiles_a, int n, int hop,
                                                               const double* __restrict__ win, const uint8_t* __restrict__ mode, int head,
                                                               int back, int base) {
    extern __shared__ __attribute__((aligned(16))) double gate_sm[];
    const int K = n / 2 + 1;
    const int s = blockIdx.z;
    const int md = mode[s];
    if (md == 0) return;
    if ((int)blockIdx.y < tiles_a) {
        gate_stft_tile<false>(x + (int64_t)s * x_stride, L, F, spx + (int64_t)s * F * K, (int)blockIdx.y * GATE_FT, n, hop, win, gate_sm,
                              GateFrameMap{0, 0, 0, 0});
        return;
    }
    const int f0 = ((int)blockIdx.y - tiles_a) * GATE_FT;
    const bool cold = md == 2;
    const int items = cold ? Fn : head + Fn - back;
    if (f0 >= items) return;
    const GateFrameMap map = {cold ? Fn : head, cold ? 0 : back - head, base, Fn};
    gate_stft_tile<true>(xn + (int64_t)s * xn_stride, Ln, items, ring + (int64_t)s * Fn * K, f0, n, hop, win, gate_sm, map);
}

// Per (row b, bin k): xmax = max_f X_db; the stationary threshold from the noise frames (or from X's own when spn == nullptr):
// XN_db clamped at its max - 40, thresh = mean + n_std * std (torch.std_mean, unbiased: NaN for a single frame, as torch).
// grid (ceil(K / 64), B), block 1024: lane = bin of the group, wave w takes frames w, w + 16, ...; the 16 partial maxima / sums are
// combined in a fixed order through LDS (every thread forms the same total).
template <bool RING>
__device__ __forceinline__ int gate_row(int f, int base, int Fn) {
    if (!RING) return f;
    const int r = base + f;
    return r >= Fn ? r - Fn : r;
}

__device__ __forceinline__ double gate_combine(double v, bool is_max, double (*red)[64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    red[w][lane] = v;
    __syncthreads();
    double r = red[0][lane];
    for (int q = 1; q < 16; ++q) r = is_max ? fmax(r, red[q][lane]) : r + red[q][lane];
    return r;
}

// RING: logical noise frame f is row (base + f) % Fn of spn (0 <= base < Fn); the sums run over the logical frames in the same order.
template <bool RING>
__device__ __forceinline__ void gate_stats_body(const double2* __restrict__ spx, int F, const double2* __restrict__ spn, int Fn, int K,
                                                int stationary, double n_std, double* __restrict__ xmax, double* __restrict__ thresh, int base,
                                                double (*red)[64]) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane;
    const int kk = k < K ? k : K - 1;
    const int b = blockIdx.y;
    const double2* X = spx + (int64_t)b * F * K + kk;
    double mx = -INFINITY;
    for (int f = w; f < F; f += 16) mx = fmax(mx, gate_db(X[(int64_t)f * K]));
    mx = gate_combine(mx, true, red);
    if (w == 0 && k < K) xmax[(int64_t)b * K + k] = mx;
    if (!stationary) return;
    const double2* N = X;
    double nmax = mx;
    if (spn) {
        N = spn + (int64_t)b * Fn * K + kk;
        nmax = -INFINITY;
        for (int f = w; f < Fn; f += 16) nmax = fmax(nmax, gate_db(N[(int64_t)gate_row<RING>(f, base, Fn) * K]));
        nmax = gate_combine(nmax, true, red);
    } else {
        Fn = F;
    }
    const double floor_db = nmax - 40.0;
    double s = 0.0;
    for (int f = w; f < Fn; f += 16) s += fmax(gate_db(N[(int64_t)gate_row<RING>(f, base, Fn) * K]), floor_db);
    const double mean = gate_combine(s, false, red) / (double)Fn;
    double ss = 0.0;
    for (int f = w; f < Fn; f += 16) {
        const double d = fmax(gate_db(N[(int64_t)gate_row<RING>(f, base, Fn) * K]), floor_db) - mean;
        ss += d * d;
    }
    ss = gate_combine(ss, false, red);
    const double sd = sqrt(ss / (double)(Fn - 1));
    if (w == 0 && k < K) thresh[(int64_t)b * K + k] = mean + sd * n_std;
}

static __global__ void __launch_bounds__(1024) k_gate_stats(const double2* __restrict__ spx, int F, const double2* __restrict__ spn, int Fn, int K,
                                                            int stationary, double n_std, double* __restrict__ xmax,
                                                            double* __restrict__ thresh) {
    __shared__ double red[16][64];
    gate_stats_body<false>(spx, F, spn, Fn, K, stationary, n_std, xmax, thresh, 0, red);
}

// The bank's: stationary, the noise frames in the rolling cache; a session with mode 0 is skipped (uniform per block).
static __global__ void __launch_bounds__(1024) k_gate_stats_ring(const double2* __restrict__ spx, int F, const double2* __restrict__ ring, int Fn,
                                                                 int K, double n_std, double* __restrict__ xmax, double* __restrict__ thresh,
                                                                 int base, const uint8_t* __restrict__ mode) {
    __shared__ double red[16][64];
    if (mode[blockIdx.y] == 0) return;
    gate_stats_body<true>(spx, F, ring, Fn, K, 1, n_std, xmax, thresh, base, red);
}

// Per (b, f, k): the mask before smoothing, in fp32 as the reference's `sig_mask.float()`; prop_decrease * (m - 1) + 1 in fp32.
// Non-stationary: m = sigmoid(((|X| - s) / (s + 1e-6) - n_thresh) / temp), s = conv1d(|X|, ones(nmm), padding="same") / nmm
// over frames (left pad (nmm - 1) / 2), evaluated in fp64 and rounded once.  grid (ceil(K / 256), F, B).
__device__ __forceinline__ void gate_mask_body(const double2* __restrict__ spx, int F, int K, const double* __restrict__ xmax,
                                                          const double* __restrict__ thresh, int nonstationary, double n_thresh,
                                                          double temp, int nmm, float prop, float* __restrict__ mraw) {
#pragma clang fp contract(off)
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int f = blockIdx.y, b = blockIdx.z;
    const double2* X = spx + (int64_t)b * F * K + k;
    float m;
    if (!nonstationary) {
        const double db = fmax(gate_db(X[(int64_t)f * K]), xmax[(int64_t)b * K + k] - 40.0);
        m = db > thresh[(int64_t)b * K + k] ? 1.0f : 0.0f;
    } else {
        const int lo = f - (nmm - 1) / 2;
        double s = 0.0;
        for (int j = 0; j < nmm; ++j) {
            const int g = lo + j;
            if (g >= 0 && g < F) {
                const double2 v = X[(int64_t)g * K];
                s += sqrt(v.x * v.x + v.y * v.y);
            }
        }
        s = s / (double)nmm;
        const double2 v = X[(int64_t)f * K];
        const double a = sqrt(v.x * v.x + v.y * v.y);
        const double r = ((a - s) / (s + 1e-6) - n_thresh) / temp;
        m = (float)(1.0 / (1.0 + exp(-r)));
    }
    mraw[((int64_t)b * F + f) * K + k] = add_rn(mul_rn(prop, sub_rn(m, 1.0f)), 1.0f);
}

static __global__ void __launch_bounds__(256) k_gate_mask(const double2* __restrict__ spx, int F, int K, const double* __restrict__ xmax,
                                                          const double* __restrict__ thresh, int nonstationary, double n_thresh,
                                                          double temp, int nmm, float prop, float* __restrict__ mraw) {
    gate_mask_body(spx, F, K, xmax, thresh, nonstationary, n_thresh, temp, nmm, prop, mraw);
}

// The bank's: a session with mode 0 is skipped (uniform per block).
static __global__ void __launch_bounds__(256) k_gate_mask_ring(const double2* __restrict__ spx, int F, int K, const double* __restrict__ xmax,
                                                          const double* __restrict__ thresh, int nonstationary, double n_thresh,
                                                          double temp, int nmm, float prop, float* __restrict__ mraw, const uint8_t* __restrict__ mode) {
    if (mode[blockIdx.z] == 0) return;
    gate_mask_body(spx, F, K, xmax, thresh, nonstationary, n_thresh, temp, nmm, prop, mraw);
}

// Per (b, f, k): mask = conv2d(mraw, filt [nf][nt], padding="same") over (bin, frame) -- a cross-correlation, left pads
// (nf - 1) / 2 and (nt - 1) / 2, zeros outside (a zero term leaves the sum unchanged, so it is skipped) -- in fp32 as the reference's
// fp32 mask is: one fused multiply-add per tap, bins outer, frames inner.  That is the order torch's CPU conv2d accumulates in for
// this shape (bit-identical masks on every fixture), so the device's mask equals the reference's and only the spectra differ.
// filt == nullptr: no smoothing.  Then Y = X * mask, in place on the spectrum.  grid (ceil(K / 256), F, B).
__device__ __forceinline__ void gate_smooth_body(double2* __restrict__ spx, int F, int K, const float* __restrict__ mraw,
                                                            const float* __restrict__ filt, int nf, int nt) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const int f = blockIdx.y, b = blockIdx.z;
    const float* M = mraw + (int64_t)b * F * K;
    float msk;
    if (filt) {
        const int k0 = k - (nf - 1) / 2, g0 = f - (nt - 1) / 2;
        float s = 0.0f;
        for (int i = 0; i < nf; ++i) {
            const int kk = k0 + i;
            if (kk < 0 || kk >= K) continue;
            for (int j = 0; j < nt; ++j) {
                const int g = g0 + j;
                if (g >= 0 && g < F) s = __builtin_fmaf(filt[i * nt + j], M[(int64_t)g * K + kk], s);
            }
        }
        msk = s;
    } else {
        msk = M[(int64_t)f * K + k];
    }
    double2* Y = spx + ((int64_t)b * F + f) * K + k;
    const double2 v = *Y;
    *Y = make_double2(v.x * (double)msk, v.y * (double)msk);
}

static __global__ void __launch_bounds__(256) k_gate_smooth(double2* __restrict__ spx, int F, int K, const float* __restrict__ mraw,
                                                            const float* __restrict__ filt, int nf, int nt) {
    gate_smooth_body(spx, F, K, mraw, filt, nf, nt);
}

// The bank's: a session with mode 0 is skipped (uniform per block).
static __global__ void __launch_bounds__(256) k_gate_smooth_ring(double2* __restrict__ spx, int F, int K, const float* __restrict__ mraw,
                                                            const float* __restrict__ filt, int nf, int nt, const uint8_t* __restrict__ mode) {
    if (mode[blockIdx.z] == 0) return;
    gate_smooth_body(spx, F, K, mraw, filt, nf, nt);
}

// Inverse, per frame: z[b][f][m] = win[m] * irfft(Y[b][f])[m] = win[m] / n * (Y_0 + (-1)^m Y_{n/2} + 2 sum_{0<k<n/2} Re(Y_k e^{2 pi i k m / n}));
// the imaginary parts of the DC and Nyquist bins are ignored, as a c2r transform does.  grid (ceil(n / 64), ceil(F / GATE_FT), B).
__device__ __forceinline__ void gate_idft_body(const double2* __restrict__ spx, int F, int n, const double* __restrict__ win,
                                               double* __restrict__ z, double* gate_sm) {
    double2* tw = reinterpret_cast<double2*>(gate_sm);       // [n]
    double2* ys = tw + n;                                    // [KC][GATE_FT]: a chunk of bins; then the partial sums
    constexpr int KC = GATE_CHUNK / 2;                       // bins per LDS round (double2: the same 32 KB as the forward chunk)
    const int K = n / 2 + 1, h = n / 2;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int m = blockIdx.x * 64 + lane;
    const int mm = m < n ? m : 0;
    const int f0 = blockIdx.y * GATE_FT;
    const double2* Y = spx + (int64_t)blockIdx.z * F * K;
    gate_twiddles(tw, n);
    double acc[GATE_FT];
#pragma unroll
    for (int f = 0; f < GATE_FT; ++f) acc[f] = 0.0;
    for (int c0 = 0; c0 < K; c0 += KC) {
        __syncthreads();
        for (int e = threadIdx.x; e < KC * GATE_FT; e += 256) {
            const int c = e / GATE_FT, f = e % GATE_FT, kb = c0 + c;
            double2 v = make_double2(0.0, 0.0);
            if (kb < K && f0 + f < F) {
                v = Y[(int64_t)(f0 + f) * K + kb];
                if (kb == 0 || kb == h) v = make_double2(v.x, 0.0);
                else v = make_double2(2.0 * v.x, 2.0 * v.y);
            }
            ys[e] = v;
        }
        __syncthreads();
        const int kb0 = c0 + w * (KC / 4);
        const int ke = min(kb0 + KC / 4, K);
        int idx = (int)(((int64_t)mm * kb0) % n);
        for (int kb = kb0; kb < ke; ++kb) {
            const double2 t = tw[idx];
            const double2* yv = ys + (kb - c0) * GATE_FT;
#pragma unroll
            for (int f = 0; f < GATE_FT; ++f) acc[f] += yv[f].x * t.x - yv[f].y * t.y;
            idx += mm;
            if (idx >= n) idx -= n;
        }
    }
    __syncthreads();
    double* part = reinterpret_cast<double*>(ys);  // [3][GATE_FT][64]
    if (w > 0) {
#pragma unroll
        for (int f = 0; f < GATE_FT; ++f) part[((w - 1) * GATE_FT + f) * 64 + lane] = acc[f];
    }
    __syncthreads();
    if (w == 0 && m < n) {
        const double wm = win[m];
#pragma unroll
        for (int f = 0; f < GATE_FT; ++f) {
            double s = acc[f];
            for (int q = 0; q < 3; ++q) s += part[(q * GATE_FT + f) * 64 + lane];
            if (f0 + f < F) z[((int64_t)blockIdx.z * F + f0 + f) * n + m] = wm * (s / (double)n);
        }
    }
}

static __global__ void __launch_bounds__(256) k_gate_idft(const double2* __restrict__ spx, int F, int n, const double* __restrict__ win,
                                                          double* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) double gate_sm[];
    gate_idft_body(spx, F, n, win, z, gate_sm);
}

// The bank's: a session with mode 0 is skipped (uniform per block, before the first barrier).
static __global__ void __launch_bounds__(256) k_gate_idft_ring(const double2* __restrict__ spx, int F, int n, const double* __restrict__ win,
                                                               double* __restrict__ z, const uint8_t* __restrict__ mode) {
    extern __shared__ __attribute__((aligned(16))) double gate_sm[];
    if (mode[blockIdx.z] == 0) return;
    gate_idft_body(spx, F, n, win, z, gate_sm);
}

// Overlap-add of the windowed frames, divided by the summed squared window, the first n/2 samples trimmed (torch.istft, center=True):
// out[b][o] = sum_f z[b][f][t - f hop] / sum_f win[t - f hop]^2, t = o + n/2, over the frames that cover t; one rounding to fp32.
// grid (ceil(Lout / 256), B).  It reads the frames alone, so `out` may be the memory the gated signal came from.
__device__ __forceinline__ void gate_ola_body(const double* __restrict__ z, int F, int n, int hop, const double* __restrict__ win, int64_t Lout,
                                              float* __restrict__ out, int64_t out_stride) {
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= Lout) return;
    const int b = blockIdx.y;
    const int64_t t = o + n / 2;
    const int64_t fl = t - n + 1 <= 0 ? 0 : (t - n + 1 + hop - 1) / hop;
    const int64_t fh = min((int64_t)F - 1, t / hop);
    double s = 0.0, env = 0.0;
    for (int64_t f = fl; f <= fh; ++f) {
        const int m = (int)(t - f * hop);
        s += z[((int64_t)b * F + f) * n + m];
        env += win[m] * win[m];
    }
    out[(int64_t)b * out_stride + o] = (float)(s / env);
}

static __global__ void __launch_bounds__(256) k_gate_ola(const double* __restrict__ z, int F, int n, int hop, const double* __restrict__ win,
                                                         int64_t Lout, float* __restrict__ out) {
    gate_ola_body(z, F, n, hop, win, Lout, out, Lout);
}

// The bank's: output rows with a stride; a session with mode 0 is skipped (uniform per block).
static __global__ void __launch_bounds__(256) k_gate_ola_ring(const double* __restrict__ z, int F, int n, int hop, const double* __restrict__ win,
                                                              int64_t Lout, float* __restrict__ out, int64_t out_stride,
                                                              const uint8_t* __restrict__ mode) {
    if (mode[blockIdx.y] == 0) return;
    gate_ola_body(z, F, n, hop, win, Lout, out, out_stride);
}

// The GUI's cross-fade of the gated input into its rolling copy (gui.py:986-990), per session with mode != 0, g [S rows of blk + Lb]:
//   g[:Lb] = g[:Lb] * fade_in + nr * fade_out;   den[-blk:] = g[:blk];   nr = g[blk:]        (blk >= Lb)
// and, with den_prev (a copy of den[blk:] rows, den_len - blk samples each), the roll den[:-blk] = den_prev.  Three fp32 roundings per
// faded sample, as torch's mul_, mul and add_ make them.  The thread that reads nr[i] is the one that rewrites it.
// grid (ceil(den_len / 256), S).
static __global__ void __launch_bounds__(256) k_nr_stitch_batch(const float* __restrict__ g, int64_t g_stride, int Lb, int64_t blk,
                                                                const float* __restrict__ fade_in, const float* __restrict__ fade_out,
                                                                float* __restrict__ nr, int64_t nr_stride, float* __restrict__ den,
                                                                int64_t den_stride, int64_t den_len, const float* __restrict__ den_prev,
                                                                int64_t prev_stride, const uint8_t* __restrict__ mode) {
    const int64_t s = blockIdx.y;
    if (mode[s] == 0) return;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= den_len) return;
    float* d = den + s * den_stride;
    const int64_t keep = den_len - blk;
    if (q < keep) {
        if (den_prev) d[q] = den_prev[s * prev_stride + q];
        return;
    }
    const int64_t i = q - keep;
    const float* gs = g + s * g_stride;
    float v = gs[i];
    if (i < Lb) {
        float* r = nr + s * nr_stride;
        v = add_rn(mul_rn(v, fade_in[i]), mul_rn(r[i], fade_out[i]));
        r[i] = gs[blk + i];
    }
    d[q] = v;
}

// Per session: mode != 0 takes a's row (na samples, written at dst + off_a), any other session b's (nb samples at off_b; b == nullptr:
// the row stays as it is).  grid (ceil(max(na, nb) / 256), S).
static __global__ void __launch_bounds__(256) k_masked_write_batch(float* __restrict__ dst, int64_t dst_stride, const float* __restrict__ a,
                                                                   int64_t a_stride, int64_t off_a, int64_t na, const float* __restrict__ b,
                                                                   int64_t b_stride, int64_t off_b, int64_t nb,
                                                                   const uint8_t* __restrict__ mode) {
    const int64_t s = blockIdx.y, q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float* d = dst + s * dst_stride;
    if (mode[s] != 0) {
        if (q < na) d[off_a + q] = a[s * a_stride + q];
    } else if (b) {
        if (q < nb) d[off_b + q] = b[s * b_stride + q];
    }
}

}  // namespace rvcmi
