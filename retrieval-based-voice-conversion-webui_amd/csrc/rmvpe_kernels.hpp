// Kernels of csrc/rmvpe.hip: the log-mel front end of the RMVPE f0 network (rvc/f0/mel.py:58-71 over rvc/f0/stft.py:165-180) and its
// Linear(512, 360) + sigmoid head (rvc/f0/e2e.py:33-35), for gfx950.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rvcmi {

constexpr int MEL_NFFT = 1024;             // n_fft == win_length
constexpr int MEL_BINS = MEL_NFFT / 2 + 1;
constexpr int MEL_NMELS = 128;
constexpr int MEL_FT = 4;                  // frames of one block: two complex transforms of two real frames each
constexpr int HEAD_K = 512, HEAD_N = 360;

typedef _Float16 rm_half8 __attribute__((ext_vector_type(8)));
typedef float rm_f32x16 __attribute__((ext_vector_type(16)));
typedef float rm_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double2 rm_cmul(double2 a, double2 w) { return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }

// One block = MEL_FT consecutive frames of one batch row, 256 threads, 64 KiB of LDS.
//   1. frames 2p and 2p + 1 of the tile are staged as the real and imaginary part of ONE complex sequence z_p (window applied, the reflection
//      of torch.stft(center=True) done by indexing; a frame at or past T is zeros);
//   2. z_p goes through a 1024-point radix-4 Stockham transform in LDS, five passes, ping-pong between two buffers; a thread owns butterfly
//      `tid` of both sequences and reads its three twiddles once per pass (table exp(-2 pi i t / 1024), fp64, computed by the host);
//   3. the two spectra are separated (X_a[k] = (Z[k] + conj Z[N - k]) / 2, X_b[k] = (Z[k] - conj Z[N - k]) / 2i), their magnitudes stay in LDS;
//   4. thread (m, h) sums mel row m over its band [lo, hi) for frames 2h and 2h + 1 (filter bank transposed, [bin][mel]: consecutive threads
//      read consecutive floats), clamps, takes the log and writes out[b][t][m]; frames T .. T_pad - 1 are written as zeros.
// Everything up to the mel sum is fp64: the test signals' quiet bins sit 60 dB under their neighbours, and with an fp32 transform one element
// in ~10^4 lands on the other side of an fp16 rounding boundary than the exact value (the reference's own fp32 path does, tests/test_cpu_rmvpe.py).
// The transform is 0.4 MFLOP per frame; the U-Net behind it is 4 GFLOP per 32 frames.
static __global__ void __launch_bounds__(256) k_rmvpe_logmel(const float* __restrict__ wav, int64_t n, int hop, int T, int T_pad,
                                                             const double* __restrict__ window, const double2* __restrict__ tw,
                                                             const float* __restrict__ basisT, const int2* __restrict__ band, float clampv,
                                                             int round_half, float* __restrict__ out) {
    __shared__ double2 buf[MEL_FT / 2][2][MEL_NFFT];
    const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * MEL_FT;
    float* o = out + ((size_t)b * T_pad + t0) * MEL_NMELS;
    const int rows = min(MEL_FT, T_pad - t0), nf = min(MEL_FT, T - t0);
    if (nf <= 0) {  // a tile of nothing but pad frames
        for (int i = tid; i < rows * MEL_NMELS; i += 256) o[i] = 0.f;
        return;
    }
    const float* x = wav + (size_t)b * n;
    for (int i = tid; i < MEL_NFFT; i += 256) {
        const double w = window[i];
        double v[MEL_FT];
#pragma unroll
        for (int f = 0; f < MEL_FT; ++f) {
            v[f] = 0.0;
            if (f < nf) {
                int64_t j = (int64_t)(t0 + f) * hop + i - MEL_NFFT / 2;
                if (j < 0) j = -j;
                if (j >= n) j = 2 * (n - 1) - j;  // (n > n_fft / 2: one reflection is enough on either side)
                v[f] = (double)x[j] * w;
            }
        }
#pragma unroll
        for (int p = 0; p < MEL_FT / 2; ++p) buf[p][0][i] = make_double2(v[2 * p], v[2 * p + 1]);
    }
    __syncthreads();
    int src = 0;
#pragma unroll
    for (int ls = 0; ls < 10; ls += 2) {  // stride s = 4^pass, sub-transform length nn = 1024 / s
        const int s = 1 << ls, n1 = (MEL_NFFT >> ls) >> 2;
        const int p = tid >> ls, q = tid & (s - 1);
        const double2 w1 = tw[p * s], w2 = tw[2 * p * s], w3 = tw[3 * p * s];
        const int i0 = q + s * p, o0 = q + s * 4 * p;
#pragma unroll
        for (int z = 0; z < MEL_FT / 2; ++z) {
            const double2* in = buf[z][src];
            double2* y = buf[z][src ^ 1];
            const double2 a = in[i0], bb = in[i0 + s * n1], c = in[i0 + 2 * s * n1], d = in[i0 + 3 * s * n1];
            const double2 apc = make_double2(a.x + c.x, a.y + c.y), amc = make_double2(a.x - c.x, a.y - c.y);
            const double2 bpd = make_double2(bb.x + d.x, bb.y + d.y), jbmd = make_double2(-(bb.y - d.y), bb.x - d.x);  // i (b - d)
            y[o0] = make_double2(apc.x + bpd.x, apc.y + bpd.y);
            y[o0 + s] = rm_cmul(make_double2(amc.x - jbmd.x, amc.y - jbmd.y), w1);
            y[o0 + 2 * s] = rm_cmul(make_double2(apc.x - bpd.x, apc.y - bpd.y), w2);
            y[o0 + 3 * s] = rm_cmul(make_double2(amc.x + jbmd.x, amc.y + jbmd.y), w3);
        }
        __syncthreads();
        src ^= 1;
    }
    // five passes: the spectra are in buf[.][1]; buf[.][0] is free and takes the magnitudes, mag[f][k] at ((double*)buf[f / 2][0])[(f & 1) * MEL_BINS + k]
    for (int k = tid; k < MEL_BINS; k += 256) {
#pragma unroll
        for (int z = 0; z < MEL_FT / 2; ++z) {
            const double2 zk = buf[z][1][k], zn = buf[z][1][(MEL_NFFT - k) & (MEL_NFFT - 1)];
            const double ar = 0.5 * (zk.x + zn.x), ai = 0.5 * (zk.y - zn.y), br = 0.5 * (zk.y + zn.y), bi = 0.5 * (zn.x - zk.x);
            double* mag = reinterpret_cast<double*>(buf[z][0]);
            mag[k] = sqrt(ar * ar + ai * ai);
            mag[MEL_BINS + k] = sqrt(br * br + bi * bi);
        }
    }
    __syncthreads();
    const int m = tid & (MEL_NMELS - 1), h = tid >> 7;
    const double* mag0 = reinterpret_cast<const double*>(buf[h][0]);
    const int2 bd = band[m];
    double acc0 = 0.0, acc1 = 0.0;
    for (int k = bd.x; k < bd.y; ++k) {
        const double w = (double)basisT[(size_t)k * MEL_NMELS + m];
        acc0 = fma(w, mag0[k], acc0);
        acc1 = fma(w, mag0[MEL_BINS + k], acc1);
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int f = 2 * h + e;
        if (f >= rows) break;
        float r = 0.f;  // a pad frame inside a tile that also holds data
        if (f < nf) {
            // the reference's mel value is an fp32 number: round the sum to fp32 first, THEN (round_half) to fp16 -- torch's `.half()` rounds an
            // fp64 tensor through fp32 as well, so a direct fp64 -> fp16 conversion differs from it on one element in 2^13 (the ties of the
            // second rounding), and a log near 0 turns that one fp16 step into several
            const float v = (float)(e ? acc1 : acc0);
            if (round_half) {  // mel.half(), clamp and log on fp16 tensors: torch evaluates the log in fp32 and rounds the result
                const _Float16 v16 = (_Float16)v, c16 = (_Float16)clampv;
                r = (float)(_Float16)logf((float)(v16 < c16 ? c16 : v16));
            } else {
                r = logf(v < clampv ? clampv : v);
            }
        }
        o[(size_t)f * MEL_NMELS + m] = r;
    }
}

// salience[row][f] = sigmoid(sum_k y[row][k] * w[f][k] + bias[f]): Linear(512, 360) + sigmoid as ONE MFMA GEMM, operands straight from global
// memory in their row-major fp32 layouts (rounded to fp16 in registers when HALF), a wave = one 32 x 32 tile over the whole K, a block = 4 waves
// = 32 rows x 128 features.  Bias and sigmoid are evaluated in fp64 on the sum and the result is rounded once.
template <bool HALF>
static __global__ void __launch_bounds__(256) k_rmvpe_head(const float* __restrict__ y, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ out, int M) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, hl = lane >> 5, col = lane & 31;
    const int row0 = blockIdx.x * 32, f0 = (blockIdx.y * 4 + wave) * 32;
    if (f0 >= HEAD_N) return;
    const float* ya = y + (size_t)min(row0 + col, M - 1) * HEAD_K;       // (clamped rows and features: unconditional loads)
    const float* wa = w + (size_t)min(f0 + col, HEAD_N - 1) * HEAD_K;
    // K in 16 chunks of 32: a chunk is accumulated by the MFMA in fp32 from zero, the chunk sums are carried in fp64 -- the rounding of a
    // 512-term fp32 chain (2e-7 on a sum of 0.3) would otherwise be the largest error of the fp32 path
    double sum[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) sum[e] = 0.0;
    for (int k0 = 0; k0 < HEAD_K; k0 += 32) {
        rm_f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        if (HALF) {
#pragma unroll
            for (int k = k0 + 8 * hl; k < k0 + 32; k += 16) {
                const rm_f32x4 w0 = *(const rm_f32x4*)(wa + k), w1 = *(const rm_f32x4*)(wa + k + 4);
                const rm_f32x4 y0 = *(const rm_f32x4*)(ya + k), y1 = *(const rm_f32x4*)(ya + k + 4);
                rm_half8 wh, yh;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    wh[e] = (_Float16)w0[e];
                    wh[e + 4] = (_Float16)w1[e];
                    yh[e] = (_Float16)y0[e];
                    yh[e + 4] = (_Float16)y1[e];
                }
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh, yh, acc, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int k = k0 + hl; k < k0 + 32; k += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[k], ya[k], acc, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) sum[e] += (double)acc[e];
    }
    const int row = row0 + col;
    if (row >= M) return;
    float* o = out + (size_t)row * HEAD_N;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int f = f0 + 8 * g + 4 * hl;  // (HEAD_N is a multiple of 4: a group of four features is inside or outside as a whole)
        if (f >= HEAD_N) continue;
        const rm_f32x4 bv = *(const rm_f32x4*)(bias + f);
        rm_f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (float)(1.0 / (1.0 + exp(-(sum[4 * g + e] + (double)bv[e]))));
        *(rm_f32x4*)(o + f) = v;
    }
}

}  // namespace rvcmi
