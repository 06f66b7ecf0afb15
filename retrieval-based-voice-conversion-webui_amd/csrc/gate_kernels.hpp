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
// as k_pv_spectrum does: any even n_fft <= 4096 (the GUI's are 880..1920, none a power of two), no plan, no workspace beyond
// the spectra.  A block owns 64 bins (or 64 samples) of GATE_FT consecutive frames; its 4 waves split the inner sum, staged
// through LDS in chunks, and add their partial sums in a fixed order, so every output depends only on its own row's data.
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
// grid (ceil(K / 64), tiles_a + tiles_b, B): the first tiles_a frame tiles are signal a, the rest signal b (the noise).
static __global__ void __launch_bounds__(256) k_gate_stft(const float* __restrict__ xa, int64_t La, int Fa, double2* __restrict__ spa,
                                                          const float* __restrict__ xb, int64_t Lb, int Fb, double2* __restrict__ spb,
                                                          int tiles_a, int n, int hop, const double* __restrict__ win) {
    extern __shared__ __attribute__((aligned(16))) double gate_sm[];
    double2* tw = reinterpret_cast<double2*>(gate_sm);  // [n]
    double* xs = gate_sm + 2 * n;                        // [GATE_CHUNK][GATE_FT]; then the partial sums
    const int K = n / 2 + 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + lane;
    const int kk = k < K ? k : 0;
    const bool is_a = (int)blockIdx.y < tiles_a;
    const float* x = is_a ? xa : xb;
    const int64_t L = is_a ? La : Lb;
    const int F = is_a ? Fa : Fb;
    double2* sp = is_a ? spa : spb;
    const int f0 = (is_a ? (int)blockIdx.y : (int)blockIdx.y - tiles_a) * GATE_FT;
    x += (int64_t)blockIdx.z * L;
    sp += (int64_t)blockIdx.z * F * K;
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
                const int64_t p = (int64_t)(f0 + f) * hop + m - n / 2;
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
            if (f0 + f < F) sp[(int64_t)(f0 + f) * K + k] = make_double2(r, i);
        }
    }
}

// Per (row b, bin k): xmax = max_f X_db; the stationary threshold from the noise frames (or from X's own when spn == nullptr):
// XN_db clamped at its max - 40, thresh = mean + n_std * std (torch.std_mean, unbiased: NaN for a single frame, as torch).
// grid (ceil(K / 64), B), block 1024: lane = bin of the group, wave w takes frames w, w + 16, ...; the 16 partial maxima / sums are
// combined in a fixed order through LDS (every thread forms the same total).
__device__ __forceinline__ double gate_combine(double v, bool is_max, double (*red)[64]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    __syncthreads();
    red[w][lane] = v;
    __syncthreads();
    double r = red[0][lane];
    for (int q = 1; q < 16; ++q) r = is_max ? fmax(r, red[q][lane]) : r + red[q][lane];
    return r;
}

static __global__ void __launch_bounds__(1024) k_gate_stats(const double2* __restrict__ spx, int F, const double2* __restrict__ spn, int Fn, int K,
                                                            int stationary, double n_std, double* __restrict__ xmax,
                                                            double* __restrict__ thresh) {
#pragma clang fp contract(off)
    __shared__ double red[16][64];
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
        for (int f = w; f < Fn; f += 16) nmax = fmax(nmax, gate_db(N[(int64_t)f * K]));
        nmax = gate_combine(nmax, true, red);
    } else {
        Fn = F;
    }
    const double floor_db = nmax - 40.0;
    double s = 0.0;
    for (int f = w; f < Fn; f += 16) s += fmax(gate_db(N[(int64_t)f * K]), floor_db);
    const double mean = gate_combine(s, false, red) / (double)Fn;
    double ss = 0.0;
    for (int f = w; f < Fn; f += 16) {
        const double d = fmax(gate_db(N[(int64_t)f * K]), floor_db) - mean;
        ss += d * d;
    }
    ss = gate_combine(ss, false, red);
    const double sd = sqrt(ss / (double)(Fn - 1));
    if (w == 0 && k < K) thresh[(int64_t)b * K + k] = mean + sd * n_std;
}

// Per (b, f, k): the mask before smoothing, in fp32 as the reference's `sig_mask.float()`; prop_decrease * (m - 1) + 1 in fp32.
// Non-stationary: m = sigmoid(((|X| - s) / (s + 1e-6) - n_thresh) / temp), s = conv1d(|X|, ones(nmm), padding="same") / nmm
// over frames (left pad (nmm - 1) / 2), evaluated in fp64 and rounded once.  grid (ceil(K / 256), F, B).
static __global__ void __launch_bounds__(256) k_gate_mask(const double2* __restrict__ spx, int F, int K, const double* __restrict__ xmax,
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

// Per (b, f, k): mask = conv2d(mraw, filt [nf][nt], padding="same") over (bin, frame) -- a cross-correlation, left pads
// (nf - 1) / 2 and (nt - 1) / 2, zeros outside (a zero term leaves the sum unchanged, so it is skipped) -- in fp32 as the reference's
// fp32 mask is: one fused multiply-add per tap, bins outer, frames inner.  That is the order torch's CPU conv2d accumulates in for
// this shape (bit-identical masks on every fixture), so the device's mask equals the reference's and only the spectra differ.
// filt == nullptr: no smoothing.  Then Y = X * mask, in place on the spectrum.  grid (ceil(K / 256), F, B).
static __global__ void __launch_bounds__(256) k_gate_smooth(double2* __restrict__ spx, int F, int K, const float* __restrict__ mraw,
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

// Inverse, per frame: z[b][f][m] = win[m] * irfft(Y[b][f])[m] = win[m] / n * (Y_0 + (-1)^m Y_{n/2} + 2 sum_{0<k<n/2} Re(Y_k e^{2 pi i k m / n}));
// the imaginary parts of the DC and Nyquist bins are ignored, as a c2r transform does.  grid (ceil(n / 64), ceil(F / GATE_FT), B).
static __global__ void __launch_bounds__(256) k_gate_idft(const double2* __restrict__ spx, int F, int n, const double* __restrict__ win,
                                                          double* __restrict__ z) {
    extern __shared__ __attribute__((aligned(16))) double gate_sm[];
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

// Overlap-add of the windowed frames, divided by the summed squared window, the first n/2 samples trimmed (torch.istft, center=True):
// out[b][o] = sum_f z[b][f][t - f hop] / sum_f win[t - f hop]^2, t = o + n/2, over the frames that cover t; one rounding to fp32.
// grid (ceil(Lout / 256), B).
static __global__ void __launch_bounds__(256) k_gate_ola(const double* __restrict__ z, int F, int n, int hop, const double* __restrict__ win,
                                                         int64_t Lout, float* __restrict__ out) {
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
    out[(int64_t)b * Lout + o] = (float)(s / env);
}

}  // namespace rvcmi
