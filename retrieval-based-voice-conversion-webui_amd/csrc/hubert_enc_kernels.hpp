// Device kernels of HuBERT's post-norm transformer layer (csrc/hubert_enc.hip): x = LN(x + Attn(x)); x = LN(x + FFN(x)), head dim 64, exact GELU.
// Operands of every MFMA are fp16 (mfma_f32_16x16x32_f16), accumulation, softmax, residual adds and the LayerNorm statistics fp32.
//
//   k_he_gemm      [M][K] x [N][K]' + bias on a 64 x 128 tile, K in steps of 64 through LDS with the next step's global loads in flight (the
//                  loop of k_hfe_gemm).  EPI_QKV: N = 3 d, q is multiplied by head_dim^-0.5 AFTER its bias, and q / k / v leave as fp16
//                  [3][B][H][T][64].  EPI_GELU: exact GELU, fp16 [M][N].
//   k_he_attn      one (item, head, 64 queries) per block, a wave owns 16 queries.  Keys come in tiles of KT = 64: scores from fp16 q . k on
//                  MFMA, an online softmax in fp32 (running max and sum per query), probabilities rounded to fp16 for the P . V MFMA, the
//                  result divided by the fp32 sum of the UNROUNDED probabilities.  The score MFMA leaves a lane with keys 16 j + 4 g + r of
//                  its query; the P . V MFMA contracts over keys in any order as long as both operands agree, so the lane's probabilities
//                  are its B operand as they stand and V (transposed into LDS) is read in that same key order: P never goes through LDS.
//   k_he_gemm_ln   [M][K] x [d][K]' + bias + residual, then LayerNorm over the row, in ONE kernel: a block owns MT = 32 full rows, wave w the
//                  columns [w d / W, (w + 1) d / W) of W = 16, 8 or 4 waves.  No operand is shared between waves except the 32 activation
//                  rows, so the fragments are read straight from global memory (the weights once per block).  Mean, then the centred sum
//                  of squares, each by lane shuffles and a [32][W] LDS exchange summed in wave order.
//
// A GEMM output row depends on no other row of its tile and the K order is fixed; the attention block belongs to one item.  So an item's rows
// are bit-equal whatever else is in the batch.  No atomics: results are bit-identical from run to run.  Floating-point contraction is OFF in this
// file and every fused multiply-add is written out: left to the compiler, the unrolled copies of an epilogue (row subtile 0 and 1, say) may be
// contracted differently, and a row's LayerNorm statistics would then depend on where in its tile the row sits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace rvcmi {
namespace hubert_enc {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int HD = 64;                                 // head dim
constexpr int KT = 64;                                 // keys per tile of k_he_attn
constexpr int QT = 64;                                 // queries per block of k_he_attn
constexpr int MT = 32;                                 // rows per block of k_he_gemm_ln
constexpr int GM = 64, GN = 128, GK = 64, GPAD = 8;    // k_he_gemm: rows, columns, K per step, LDS row padding (halves)
constexpr int EPI_QKV = 0, EPI_GELU = 1;

__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.f + erff(v * 0.70710678118654752440f)); }

__device__ __forceinline__ half8 load8(const _Float16* p) { return *(const half8*)p; }
__device__ __forceinline__ half8 load8(const float* p) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
    return half8{(_Float16)a[0], (_Float16)a[1], (_Float16)a[2], (_Float16)a[3], (_Float16)b[0], (_Float16)b[1], (_Float16)b[2], (_Float16)b[3]};
}
__device__ __forceinline__ f32x4 load4f(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 load4f(const _Float16* p) {
    const half4 h = *(const half4*)p;
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
__device__ __forceinline__ void store4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void store4(_Float16* p, f32x4 v) { *(half4*)p = half4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]}; }

// x [M][K] (fp16, or fp32 rounded to fp16 on the way in), w [N][K] fp16 (torch's Linear layout), bias [N] fp32.  grid (ceil(M / GM), ceil(N / GN)).
// EPI_QKV: N = 3 H 64, rows are (item, frame) = (m / T, m % T); out fp16 [3][M / T][H][T][64], q scaled by qscale after the bias.
// EPI_GELU: out fp16 [M][N].  N is a multiple of 64.
template <typename XT, int EPI>
__global__ void __launch_bounds__(256) k_he_gemm(const XT* __restrict__ x, const _Float16* __restrict__ w, const float* __restrict__ bias,
                                                 _Float16* __restrict__ out, int M, int N, int K, int T, int H, float qscale) {
    __shared__ _Float16 sW[GN][GK + GPAD], sX[GM][GK + GPAD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    const int wn = wave & 1, wm = wave >> 1;
    const int m0 = blockIdx.x * GM, n0 = blockIdx.y * GN;
    // a thread moves chunks (row, kc) = ((tid >> 3) + 32 i, tid & 7): 8 halves each, 4 of the weight tile and 2 of the activation tile
    const int lr = tid >> 3, kc = (tid & 7) * 8;
    const _Float16* wp[4];
    const XT* xp[2];
    bool wv[4], xv[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = n0 + lr + 32 * i;
        wv[i] = n < N;
        wp[i] = w + (size_t)(wv[i] ? n : 0) * K + kc;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + lr + 32 * i;
        xv[i] = m < M;
        xp[i] = x + (size_t)(xv[i] ? m : 0) * K + kc;
    }
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 rw[4], rx[2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) rw[i] = wv[i] ? load8(wp[i] + k0) : zero;
#pragma unroll
        for (int i = 0; i < 2; ++i) rx[i] = xv[i] ? load8(xp[i] + k0) : zero;
    };
    f32x4 acc[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += GK) {
        __syncthreads();  // the previous step's fragments have been read
#pragma unroll
        for (int i = 0; i < 4; ++i) *(half8*)&sW[lr + 32 * i][kc] = rw[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *(half8*)&sX[lr + 32 * i][kc] = rx[i];
        __syncthreads();
        if (k0 + GK < K) fetch(k0 + GK);
#pragma unroll
        for (int kk = 0; kk < GK; kk += 32) {
            half8 wf[4], xf[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *(const half8*)&sW[wn * 64 + j * 16 + l16][kk + g * 8];
#pragma unroll
            for (int i = 0; i < 2; ++i) xf[i] = *(const half8*)&sX[wm * 32 + i * 16 + l16][kk + g * 8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf[i], acc[j][i], 0, 0, 0);
        }
    }
    // lane: row l16 of the row subtile, columns 4 g .. 4 g + 3 of the column subtile
    const int d = EPI == EPI_QKV ? N / 3 : N, nb = EPI == EPI_QKV ? M / T : 0;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 32 + i * 16 + l16;
        if (m >= M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + g * 4;
            if (n >= N) continue;
            const f32x4 bv = *(const f32x4*)(bias + n);
            f32x4 v = acc[j][i] + bv;
            if (EPI == EPI_QKV) {
                const int which = n / d, c = n - which * d, hh = c >> 6, dd = c & 63, b = m / T, t = m - b * T;
                if (which == 0) v *= qscale;
                store4(out + ((((size_t)which * nb + b) * H + hh) * T + t) * HD + dd, v);
            } else {
                store4(out + (size_t)m * N + n, f32x4{gelu_erf(v[0]), gelu_erf(v[1]), gelu_erf(v[2]), gelu_erf(v[3])});
            }
        }
    }
}

// q / k / v fp16 [B][H][T][64] (q already scaled), mask uint8 [B][T] or NULL (1: the key is padding), out fp16 [B][T][H 64].
// grid (ceil(T / QT), H, B), 256 threads.  A query row whose every key is masked leaves as zeros.
__global__ void __launch_bounds__(256) k_he_attn(const _Float16* __restrict__ q, const _Float16* __restrict__ k, const _Float16* __restrict__ v,
                                                 const uint8_t* __restrict__ mask, _Float16* __restrict__ out, int T, int H) {
    __shared__ _Float16 sK[KT][HD + GPAD], sVt[HD][KT + GPAD];
    __shared__ uint8_t sM[KT];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    const int h = blockIdx.y, b = blockIdx.z;
    const size_t base = ((size_t)b * H + h) * (size_t)T * HD;
    const int qrow = blockIdx.x * QT + wave * 16 + l16;
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    half8 qf[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) qf[s] = qrow < T ? *(const half8*)(q + base + (size_t)qrow * HD + s * 32 + g * 8) : zero;
    const float NEG = -__builtin_huge_valf();
    float m_run = NEG, l_run = 0.f;  // l_run: this lane's share of the row sum (its 16 keys of every tile)
    f32x4 o[4];
#pragma unroll
    for (int jd = 0; jd < 4; ++jd) o[jd] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kt0 = 0; kt0 < T; kt0 += KT) {
        __syncthreads();  // the previous tile has been read
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = tid + 256 * i, row = c >> 3, col = (c & 7) * 8, key = kt0 + row;
            const bool ok = key < T;
            const half8 kv = ok ? *(const half8*)(k + base + (size_t)key * HD + col) : zero;
            const half8 vv = ok ? *(const half8*)(v + base + (size_t)key * HD + col) : zero;
            *(half8*)&sK[row][col] = kv;
#pragma unroll
            for (int e = 0; e < 8; ++e) sVt[col + e][row] = vv[e];
        }
        if (tid < KT) {
            const int key = kt0 + tid;
            sM[tid] = (key >= T || (mask && mask[(size_t)b * T + key])) ? 1 : 0;
        }
        __syncthreads();
        f32x4 s[4];
        float mx = NEG;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const half8 kf = *(const half8*)&sK[j * 16 + l16][st * 32 + g * 8];
                s[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[st], s[j], 0, 0, 0);
            }
            // s[j][r]: key kt0 + 16 j + 4 g + r against query l16
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (sM[j * 16 + g * 4 + r]) s[j][r] = NEG;
                mx = fmaxf(mx, s[j][r]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_ref = m_new == NEG ? 0.f : m_new;  // (no key yet: every exponential below is exp(-inf) = 0, without a branch)
        const float alpha = expf(m_run - m_ref);         // (0 on the first tile with a key)
        m_run = m_new;
        float ps = 0.f;
        half8 pf[2];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = expf(s[j][r] - m_ref);
                ps += p;
                pf[j >> 1][(j & 1) * 4 + r] = (_Float16)p;
            }
        l_run = l_run * alpha + ps;
#pragma unroll
        for (int jd = 0; jd < 4; ++jd) {
            o[jd] *= alpha;
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                // the MFMA's k slots 8 g .. 8 g + 7 of step st: keys 32 st + 4 g + e and 32 st + 16 + 4 g + e, e < 4, in both operands
                const half4 v0 = *(const half4*)&sVt[jd * 16 + l16][st * 32 + g * 4];
                const half4 v1 = *(const half4*)&sVt[jd * 16 + l16][st * 32 + 16 + g * 4];
                const half8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
                o[jd] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[st], o[jd], 0, 0, 0);
            }
        }
    }
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    if (qrow >= T) return;
    const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
    // o[jd][r]: dim 16 jd + 4 g + r of query l16
    _Float16* op = out + ((size_t)b * T + qrow) * ((size_t)H * HD) + (size_t)h * HD + g * 4;
#pragma unroll
    for (int jd = 0; jd < 4; ++jd) store4(op + jd * 16, o[jd] * inv);
}

// x [M][K] fp16, w [d][K] fp16, bias / gamma / beta [d] fp32, res [M][d] (RT), out [M][d] (OT) = LayerNorm(x w' + bias + res); ALSO16: the
// same rounded to fp16 into out16 (the next GEMM's operand).  grid (ceil(M / MT)), 64 WAVES threads; wave w owns the d / WAVES columns from
// w d / WAVES on, d / WAVES = 16 nj, nj <= NJ (the host picks 16 waves when d is a multiple of 256, 8 for a multiple of 128, else 4: the weights
// stream through few blocks, so a block hides their latency with as many waves as the columns allow).  K is a multiple of 64 and goes in steps
// of 64 (32 on 16 waves), the next step's fragments in flight while the current one is multiplied.
template <int WAVES, int NJ, typename RT, typename OT, bool ALSO16>
__global__ void __launch_bounds__(WAVES * 64) k_he_gemm_ln(const _Float16* __restrict__ x, const _Float16* __restrict__ w, const float* __restrict__ bias,
                                                           const RT* __restrict__ res, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float eps, OT* __restrict__ out, _Float16* __restrict__ out16, int M, int d, int K) {
    __shared__ float red1[MT][WAVES], red2[MT][WAVES];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, g = lane >> 4;
    const int cw = d / WAVES, nj = cw >> 4, c0 = wave * cw, m0 = blockIdx.x * MT;
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    const _Float16* xp[2];
    bool xv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + i * 16 + l16;
        xv[i] = m < M;
        xp[i] = x + (size_t)(xv[i] ? m : 0) * K + g * 8;
    }
    const _Float16* wp = w + (size_t)(c0 + l16) * K + g * 8;
    f32x4 acc[NJ][2];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    // [.][32-wide part of a step]: steps of 64, of 32 on 16 waves (128 registers a lane there)
    constexpr int KS = WAVES == 16 ? 1 : 2, STEP = 32 * KS;
    half8 xa[2][KS], xb[2][KS], wa[NJ][KS], wb[NJ][KS];
    auto fetch = [&](half8(&xf)[2][KS], half8(&wf)[NJ][KS], int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < KS; ++s) xf[i][s] = xv[i] ? *(const half8*)(xp[i] + k0 + 32 * s) : zero;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (j < nj) {
#pragma unroll
                for (int s = 0; s < KS; ++s) wf[j][s] = *(const half8*)(wp + (size_t)j * 16 * K + k0 + 32 * s);
            }
    };
    auto mac = [&](const half8(&xf)[2][KS], const half8(&wf)[NJ][KS]) {
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                if (j < nj) {
                    acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j][s], xf[0][s], acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j][s], xf[1][s], acc[j][1], 0, 0, 0);
                }
    };
    fetch(xa, wa, 0);
    for (int k0 = 0; k0 < K; k0 += 2 * STEP) {
        const bool more = k0 + STEP < K;
        if (more) fetch(xb, wb, k0 + STEP);
        mac(xa, wa);
        if (more) {
            if (k0 + 2 * STEP < K) fetch(xa, wa, k0 + 2 * STEP);
            mac(xb, wb);
        }
    }
    // lane: row l16 of row subtile i, columns c0 + 16 j + 4 g + r.  + bias + residual, then the row's sum
    float sum[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j < nj) {
            const int c = c0 + j * 16 + g * 4;
            const f32x4 bv = *(const f32x4*)(bias + c);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = m0 + i * 16 + l16;
                const f32x4 rv = xv[i] ? load4f(res + (size_t)m * d + c) : f32x4{0.f, 0.f, 0.f, 0.f};
                acc[j][i] = (acc[j][i] + bv) + rv;
                sum[i] += (acc[j][i][0] + acc[j][i][1]) + (acc[j][i][2] + acc[j][i][3]);
            }
        }
    }
    float mean[2], rstd[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        sum[i] += __shfl_xor(sum[i], 16, 64);
        sum[i] += __shfl_xor(sum[i], 32, 64);
        if (g == 0) red1[i * 16 + l16][wave] = sum[i];
    }
    __syncthreads();
    const float invd = 1.f / (float)d;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float* r = red1[i * 16 + l16];
        float t = r[0];
#pragma unroll
        for (int v = 1; v < WAVES; ++v) t += r[v];  // in wave order
        mean[i] = t * invd;
        sum[i] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j < nj) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc[j][i] -= mean[i];
                const f32x4 a = acc[j][i];
                sum[i] = fmaf(a[3], a[3], fmaf(a[2], a[2], fmaf(a[1], a[1], fmaf(a[0], a[0], sum[i]))));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        sum[i] += __shfl_xor(sum[i], 16, 64);
        sum[i] += __shfl_xor(sum[i], 32, 64);
        if (g == 0) red2[i * 16 + l16][wave] = sum[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float* r = red2[i * 16 + l16];
        float t = r[0];
#pragma unroll
        for (int v = 1; v < WAVES; ++v) t += r[v];
        rstd[i] = 1.f / sqrtf(t * invd + eps);  // biased variance, as LayerNorm takes it
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (j < nj) {
            const int c = c0 + j * 16 + g * 4;
            const f32x4 gv = *(const f32x4*)(gamma + c), sv = *(const f32x4*)(beta + c);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int m = m0 + i * 16 + l16;
                if (!xv[i]) continue;
                const f32x4 n = acc[j][i] * rstd[i];
                const f32x4 y = {fmaf(n[0], gv[0], sv[0]), fmaf(n[1], gv[1], sv[1]), fmaf(n[2], gv[2], sv[2]), fmaf(n[3], gv[3], sv[3])};
                store4(out + (size_t)m * d + c, y);
                if (ALSO16) store4(out16 + (size_t)m * d + c, y);
            }
        }
    }
}

}  // namespace hubert_enc
}  // namespace rvcmi
