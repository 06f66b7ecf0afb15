// Device kernels of HuBERT's convolutional feature extractor (csrc/hubert_fe.hip).  Activations are fp16, channels-last ([B][L][512]),
// accumulation and every epilogue fp32, the GroupNorm statistics fp64.
//
//   k_hfe_stats        layer 0 is linear in ONE input channel, so the per-(item, channel) mean and variance of its output follow from the
//                      input alone: frame t reads x[5 t + k], k < 10, and with m_k = mean_t x[5 t + k] and Cov_jk the CENTRED covariance of
//                      those ten strided views, mean_c = w_c . m and var_c = w_c' Cov w_c.  A block takes a chunk of ST_FRAMES frames: the
//                      ten sums, then (second pass over the same, cached, samples) the 55 co-moments about the chunk's own means.
//   k_hfe_stats_final  merges the chunks in chunk order with the exact identity
//                          Cov_jk = sum_i [M2_i,jk + n_i (m_i,j - m_j)(m_i,k - m_k)] / n
//                      (every term centred: no E[y^2] - mean^2), then per channel scale = gamma / sqrt(var + eps) and the shift.
//   k_hfe_conv0        conv (10 taps on x - m_k, so a DC offset never reaches the sum) + GroupNorm + exact GELU in one pass; the pre-norm tensor
//                      is never stored.
//   k_hfe_gemm         layers 1 - 6.  Channels-last makes a stride-2 convolution of 3 (2) taps a GEMM: row t of the activation operand is the
//                      contiguous 1536 (1024) halves that start at input row 2 t, so rows overlap by one (not at all).  128 frames x 128 output
//                      channels per block on mfma_f32_16x16x32_f16, K in steps of 64 through LDS with the next step's global loads in flight.
//                      The weight fragment is the MFMA's A operand, so a lane ends with 4 consecutive output channels of one frame.
//
// No atomics anywhere and every reduction in a fixed order: results are bit-identical from run to run.
//
// RAGGED = true (rvcmi_hubert_fe_forward_ragged): item b is the first lens[b] samples of its row of a [B][N_max] batch, and every buffer keeps
// the strides of N_max.  Each kernel takes the item's OWN row count from lens[b] where the dense one takes the launch's: the statistics chunks
// and their merge, layer 0 and every GEMM row then see exactly what a lone call of that item sees (a chunk's content and the merge order depend
// on the item's L0 alone, a GEMM output row on no other row of its tile, the K order is fixed), so the valid rows are bit-equal to that call.
// Nothing behind an item's end is read; the last layer writes zeros there.  RAGGED = false compiles to the dense kernels unchanged.
#pragma once
#include <hip/hip_runtime.h>

namespace rvcmi {
namespace hubert {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HC = 512;           // channels of every layer
constexpr int K0 = 10, S0 = 5;    // layer 0: taps, stride
constexpr int ST_FRAMES = 2048;   // frames per statistics chunk
constexpr int NCOV = 55;          // upper triangle of the 10 x 10 covariance
constexpr int ST_VALS = K0 + NCOV;
constexpr int F0_BLK = 32;        // frames per block of k_hfe_conv0
constexpr int GM = 128, GN = 128, GK = 64, GPAD = 8;  // k_hfe_gemm: frames, channels, K per step, LDS row padding (halves)

__host__ __device__ inline int tri(int j, int k) { return j * K0 - j * (j - 1) / 2 + (k - j); }  // j <= k

// rows after layer l (0 .. 6) of an n-sample input (n >= 400): 10 taps stride 5, then 3, 3, 3, 3, 2, 2 taps stride 2
__host__ __device__ inline int rows_after(int n, int l) {
    int L = (n - K0) / S0 + 1;
    for (int i = 1; i <= l; ++i) L = (L - (i <= 4 ? 3 : 2)) / 2 + 1;
    return L;
}

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

// sum over the block's 256 threads, in a fixed order: lanes by shuffle, then the four waves in wave order.  sh: [4] doubles.
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();  // (sh is reused from one call to the next)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// part [B][nchunk][ST_VALS]: the chunk's ten means, then its 55 co-moments about them.  grid (nchunk, B).  RAGGED: L0 is the item's own, and a
// chunk wholly behind its end is skipped (it has no frames to average; k_hfe_stats_final does not read it).
template <typename T, bool RAGGED>
__global__ void __launch_bounds__(256) k_hfe_stats(const T* __restrict__ x, size_t N, int L0, double* __restrict__ part, const int* __restrict__ lens) {
    __shared__ double sh[4];
    if (RAGGED) L0 = rows_after(lens[blockIdx.y], 0);
    const int f0 = blockIdx.x * ST_FRAMES, f1 = min(L0, f0 + ST_FRAMES);
    if (RAGGED && f0 >= L0) return;
    const T* xb = x + (size_t)blockIdx.y * N;
    double s[K0];
#pragma unroll
    for (int k = 0; k < K0; ++k) s[k] = 0.0;
    for (int f = f0 + (int)threadIdx.x; f < f1; f += 256) {
        const T* p = xb + (size_t)f * S0;
#pragma unroll
        for (int k = 0; k < K0; ++k) s[k] += (double)(float)p[k];
    }
    const double inv = 1.0 / (double)(f1 - f0);
    double m[K0];
#pragma unroll
    for (int k = 0; k < K0; ++k) m[k] = block_sum(s[k], sh) * inv;
    double c[NCOV];
#pragma unroll
    for (int i = 0; i < NCOV; ++i) c[i] = 0.0;
    for (int f = f0 + (int)threadIdx.x; f < f1; f += 256) {
        const T* p = xb + (size_t)f * S0;
        double d[K0];
#pragma unroll
        for (int k = 0; k < K0; ++k) d[k] = (double)(float)p[k] - m[k];
#pragma unroll
        for (int j = 0; j < K0; ++j)
#pragma unroll
            for (int k = j; k < K0; ++k) c[tri(j, k)] = fma(d[j], d[k], c[tri(j, k)]);
    }
    double* o = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * ST_VALS;
#pragma unroll
    for (int k = 0; k < K0; ++k)
        if (threadIdx.x == 0) o[k] = m[k];
#pragma unroll
    for (int i = 0; i < NCOV; ++i) {
        const double t = block_sum(c[i], sh);
        if (threadIdx.x == 0) o[K0 + i] = t;
    }
}

// w0 [512][10] (the fp16-rounded weights as floats), gamma / beta [512].  -> meanf [B][10] (the input means as the floats k_hfe_conv0 subtracts),
// scale / shift [B][512]: layer 0's output before the GELU is scale * sum_k w_k (x_k - meanf_k) + shift.  grid (B), 512 threads.
// RAGGED: nchunk is the stride of ``part`` (the longest item's chunks); the item merges its own ceil(L0 / ST_FRAMES) and divides by its own L0.
template <bool RAGGED>
__global__ void __launch_bounds__(512) k_hfe_stats_final(const double* __restrict__ part, int nchunk, int L0, const float* __restrict__ w0,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, double eps,
                                                         float* __restrict__ meanf, float* __restrict__ scale, float* __restrict__ shift,
                                                         const int* __restrict__ lens) {
    __shared__ double mean[K0], cov[K0 * K0];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* pb = part + (size_t)b * nchunk * ST_VALS;
    if (RAGGED) {
        L0 = rows_after(lens[b], 0);
        nchunk = (L0 + ST_FRAMES - 1) / ST_FRAMES;
    }
    auto rows = [&](int i) { return (double)(min(L0, (i + 1) * ST_FRAMES) - i * ST_FRAMES); };
    if (tid < K0) {
        double s = 0.0;
        for (int i = 0; i < nchunk; ++i) s = fma(rows(i), pb[(size_t)i * ST_VALS + tid], s);
        mean[tid] = s / (double)L0;
        meanf[b * K0 + tid] = (float)mean[tid];
    }
    __syncthreads();
    if (tid < K0 * K0) {
        const int j = tid / K0, k = tid - j * K0, t = j <= k ? tri(j, k) : tri(k, j);
        double s = 0.0;
        for (int i = 0; i < nchunk; ++i) {
            const double* p = pb + (size_t)i * ST_VALS;
            s += p[K0 + t] + rows(i) * (p[j] - mean[j]) * (p[k] - mean[k]);
        }
        cov[tid] = s / (double)L0;  // biased, as GroupNorm takes it
    }
    __syncthreads();
    double w[K0], mu = 0.0, mu_f = 0.0, var = 0.0;
#pragma unroll
    for (int k = 0; k < K0; ++k) {
        w[k] = (double)w0[tid * K0 + k];
        mu = fma(w[k], mean[k], mu);
        mu_f = fma(w[k], (double)(float)mean[k], mu_f);
    }
#pragma unroll
    for (int j = 0; j < K0; ++j) {
        double r = 0.0;
#pragma unroll
        for (int k = 0; k < K0; ++k) r = fma(cov[j * K0 + k], w[k], r);
        var = fma(w[j], r, var);
    }
    const double sc = (double)gamma[tid] / sqrt(fmax(var, 0.0) + eps);
    scale[(size_t)b * HC + tid] = (float)sc;
    shift[(size_t)b * HC + tid] = (float)((double)beta[tid] - (mu - mu_f) * sc);  // (what rounding the means to float left behind)
}

// out [B][L0][512] fp16.  grid (ceil(L0 / F0_BLK), B); thread: 8 channels (tid & 63) of 8 frames.  RAGGED: L0 stays the row stride of ``out``,
// the item stops at its own count.
template <typename T, bool RAGGED>
__global__ void __launch_bounds__(256) k_hfe_conv0(const T* __restrict__ x, size_t N, int L0, const float* __restrict__ w0, const float* __restrict__ meanf,
                                                   const float* __restrict__ scale, const float* __restrict__ shift, _Float16* __restrict__ out,
                                                   const int* __restrict__ lens) {
    const int oct = threadIdx.x & 63, fl = threadIdx.x >> 6, b = blockIdx.y;
    const int Lb = RAGGED ? rows_after(lens[b], 0) : L0;
    if (RAGGED && (int)blockIdx.x * F0_BLK >= Lb) return;
    const T* xb = x + (size_t)b * N;
    float w[8][K0], sc[8], sh[8], m[K0];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int c = oct * 8 + r;
#pragma unroll
        for (int k = 0; k < K0; ++k) w[r][k] = w0[c * K0 + k];
        sc[r] = scale[(size_t)b * HC + c];
        sh[r] = shift[(size_t)b * HC + c];
    }
#pragma unroll
    for (int k = 0; k < K0; ++k) m[k] = meanf[b * K0 + k];
    for (int i = 0; i < F0_BLK / 4; ++i) {
        const int f = blockIdx.x * F0_BLK + fl * (F0_BLK / 4) + i;
        if (f >= Lb) break;
        const T* p = xb + (size_t)f * S0;
        float d[K0];
#pragma unroll
        for (int k = 0; k < K0; ++k) d[k] = (float)p[k] - m[k];
        half8 hv;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < K0; ++k) a = fmaf(w[r][k], d[k], a);
            hv[r] = (_Float16)gelu_erf(fmaf(a, sc[r], sh[r]));
        }
        *(half8*)(out + ((size_t)b * L0 + f) * HC + oct * 8) = hv;
    }
}

// x [B][Lin][512] fp16, w [512][K] fp16 (K = taps * 512, tap-major), Lout = (Lin - taps) / 2 + 1.  OUT32 = false: out fp16 [B][Lout][512] =
// GELU(conv); OUT32 = true (the test hook): out fp32, no activation.  grid (ceil(Lout / GM), 512 / GN, B), 256 threads.
// RAGGED (``layer`` 1 .. 6 of items of lens[b] samples): Lin / Lout are the row strides of x / out and the grid's extent; the item's own output
// rows Lb follow from lens[b].  A tile wholly behind Lb returns before the K loop, so the cost follows the items' own lengths.  ``zero_tail``
// (the last layer): rows Lb .. Lout of the item are written as zeros, by that early return and by the partial tile's epilogue.
template <bool OUT32, bool RAGGED>
__global__ void __launch_bounds__(256) k_hfe_gemm(const _Float16* __restrict__ x, const _Float16* __restrict__ w, void* __restrict__ out, int Lin, int Lout,
                                                  int K, const int* __restrict__ lens, int layer, int zero_tail) {
    __shared__ _Float16 sW[GN][GK + GPAD], sX[GM][GK + GPAD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    const int wn = wave & 1, wm = wave >> 1;
    const int t0 = blockIdx.x * GM, n0 = blockIdx.y * GN, b = blockIdx.z;
    const _Float16* xb = x + (size_t)b * Lin * HC;
    const int Lb = RAGGED ? rows_after(lens[b], layer) : Lout;  // the item's own output rows (<= Lout)
    if (RAGGED && t0 >= Lb) {
        if (zero_tail) {  // 128 rows x 128 channels of fp16 zeros: 16 lanes per row
            const half8 z = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int r = tid >> 4; r < GM && t0 + r < Lout; r += 16)
                *(half8*)((_Float16*)out + ((size_t)b * Lout + t0 + r) * HC + n0 + (tid & 15) * 8) = z;
        }
        return;
    }
    // a thread moves chunks (row, kc) = ((tid >> 3) + 32 i, tid & 7) of both tiles: 8 halves each
    const int lr = tid >> 3, kc = (tid & 7) * 8;
    const _Float16* wp[4];
    const _Float16* xp[4];
    bool xv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = lr + 32 * i, t = t0 + r;
        wp[i] = w + (size_t)(n0 + r) * K + kc;
        xv[i] = t < Lb;
        xp[i] = xb + (size_t)(xv[i] ? t : 0) * (2 * HC) + kc;  // (stride 2: two input rows per frame)
    }
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 rw[4], rx[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rw[i] = *(const half8*)(wp[i] + k0);
            rx[i] = xv[i] ? *(const half8*)(xp[i] + k0) : zero;
        }
    };
    f32x4 acc[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += GK) {
        __syncthreads();  // the previous step's fragments have been read
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *(half8*)&sW[lr + 32 * i][kc] = rw[i];
            *(half8*)&sX[lr + 32 * i][kc] = rx[i];
        }
        __syncthreads();
        if (k0 + GK < K) fetch(k0 + GK);
#pragma unroll
        for (int kk = 0; kk < GK; kk += 32) {
            half8 wf[4], xf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *(const half8*)&sW[wn * 64 + j * 16 + l16][kk + g * 8];
#pragma unroll
            for (int i = 0; i < 4; ++i) xf[i] = *(const half8*)&sX[wm * 64 + i * 16 + l16][kk + g * 8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf[i], acc[j][i], 0, 0, 0);
        }
    }
    // lane: frame l16 of the frame subtile, output channels 4 g .. 4 g + 3 of the channel subtile
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int t = t0 + wm * 64 + i * 16 + l16;
        if (t >= Lb) {
            if (RAGGED && zero_tail && t < Lout) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    *(half4*)((_Float16*)out + ((size_t)b * Lout + t) * HC + n0 + wn * 64 + j * 16 + g * 4) = half4{0, 0, 0, 0};
            }
            continue;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const size_t o = ((size_t)b * Lout + t) * HC + n0 + wn * 64 + j * 16 + g * 4;
            const f32x4 v = acc[j][i];
            if (OUT32) {
                *(f32x4*)((float*)out + o) = v;
            } else {
                const half4 hv = {(_Float16)gelu_erf(v[0]), (_Float16)gelu_erf(v[1]), (_Float16)gelu_erf(v[2]), (_Float16)gelu_erf(v[3])};
                *(half4*)((_Float16*)out + o) = hv;
            }
        }
    }
}

}  // namespace hubert
}  // namespace rvcmi
