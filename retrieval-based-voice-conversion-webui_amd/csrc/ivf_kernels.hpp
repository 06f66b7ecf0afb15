// Kernels of the IVF-Flat search and of the index build: the coarse quantiser (k_coarse*), the query-major in-list scan with its
// per-wave top-k (k_scan, k_scan_v, TopK), the list-sorted query order (k_qsort_*), the blend (k_blend) and the k-means helpers
// (k_list_mean, k_assigned_dist, k_gather_rows).  Included once, by ivf.hip -- the only translation unit that instantiates IVF
// kernels (they have internal linkage: a second unit would duplicate them in the code object) -- in front of ivf_lm_kernels.hpp and
// ivf_add_kernels.hpp, which build on the coarse kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "glue_kernels.hpp"
#include "ivf_format.hpp"  // align_up

namespace rvcmi {

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------

constexpr int QT = 4;  // queries per coarse block

// Coarse quantiser, nprobe == 1: for QT queries (LDS, broadcast reads) every lane owns one centroid
// at a time and accumulates QT fp64 distances for it -- no cross-lane reduction in the hot loop.
// Each lane keeps its running best; one wave-level (dist, id) argmin per query at the end.
__global__ void __launch_bounds__(256) k_coarse1(const float* __restrict__ q, const float4* __restrict__ cent_t,
                                                 int64_t nq, int64_t nlist, int d, int64_t* __restrict__ assign) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* qs = (float*)smem_raw;                               // [QT][d]
    double* bd = (double*)(smem_raw + align_up((size_t)QT * d * 4, 16));  // [4 waves][QT]
    int64_t* bi = (int64_t*)(bd + 4 * QT);
    const int64_t q0 = (int64_t)blockIdx.x * QT;
    const int nqb = (int)min((int64_t)QT, nq - q0);
    for (int i = threadIdx.x; i < QT * d; i += 256) {
        int qi = i / d;
        qs[i] = qi < nqb ? q[(q0 + qi) * d + (i - qi * d)] : 0.f;
    }
    __syncthreads();
    double best[QT];
    int64_t besti[QT];
#pragma unroll
    for (int k = 0; k < QT; ++k) { best[k] = INFINITY; besti[k] = INT64_MAX; }
    const int d4 = d >> 2;
    for (int64_t c = threadIdx.x; c < nlist; c += 256) {
        const float4* row = cent_t + c;  // element e of centroid c lives at cent_t[e*nlist + c]
        double acc[QT];
#pragma unroll
        for (int k = 0; k < QT; ++k) acc[k] = 0.0;
#pragma unroll 8
        for (int e = 0; e < d4; ++e) {
            const float4 v = row[(size_t)e * nlist];
#pragma unroll
            for (int k = 0; k < QT; ++k) {
                const float4 qq = *(const float4*)(qs + k * d + e * 4);
                double t0 = (double)qq.x - (double)v.x, t1 = (double)qq.y - (double)v.y;
                double t2 = (double)qq.z - (double)v.z, t3 = (double)qq.w - (double)v.w;
                acc[k] = fma(t0, t0, acc[k]);
                acc[k] = fma(t1, t1, acc[k]);
                acc[k] = fma(t2, t2, acc[k]);
                acc[k] = fma(t3, t3, acc[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < QT; ++k)
            if (acc[k] < best[k]) { best[k] = acc[k]; besti[k] = c; }  // c ascending per lane: ties keep the lower id
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < QT; ++k) {
        double bdv = best[k];
        int64_t biv = besti[k];
        for (int off = 32; off >= 1; off >>= 1) {
            double od = __shfl_xor(bdv, off, 64);
            int64_t oi = __shfl_xor(biv, off, 64);
            if (od < bdv || (od == bdv && oi < biv)) { bdv = od; biv = oi; }
        }
        if (lane == 0) { bd[wave * QT + k] = bdv; bi[wave * QT + k] = biv; }
    }
    __syncthreads();
    if (threadIdx.x < nqb) {
        const int k = threadIdx.x;
        double bdv = bd[k];
        int64_t biv = bi[k];
        for (int w = 1; w < 4; ++w) {
            double od = bd[w * QT + k];
            int64_t oi = bi[w * QT + k];
            if (od < bdv || (od == bdv && oi < biv)) { bdv = od; biv = oi; }
        }
        assign[q0 + k] = biv;
    }
}

// ---- nprobe == 1 fast path: fp32 prefilter on the exact-fp32 MFMA, fp64 verification of the near-ties -------------
//
// k_coarse_gemm: S[q][c] = fl32(|c|^2) - 2*dot32(q, c) with v_mfma_f32_32x32x2_f32 (an fmaf chain, so the classic
// dot-product error bound holds: |err| <= d*u*|q||c|, u = 2^-24).  Block = 64 queries x 128 centroids, K chunks of 32
// staged in LDS (row stride 33 floats: conflict-free ds_read_b32 for both operands).
constexpr int CG_K = 32, CG_S = 33;
using f32x16 = __attribute__((ext_vector_type(16))) float;
// MQ query tiles of 32 per block, NWC waves each owning 32 centroids.  (2, 4): 64 x 128 tiles for big nlist;
// (1, 1): one wave per 32 x 32 tile, so that small problems (nlist 256: 8 x 19 blocks) are not latency-bound.
template <int MQ, int NWC>
__global__ void __launch_bounds__(64 * NWC) k_coarse_gemm(const float* __restrict__ q, const float* __restrict__ cent,
                                                          const float* __restrict__ cn, int64_t nq, int64_t nlist, int d,
                                                          float* __restrict__ S) {
    constexpr int NT = 64 * NWC, QR = 32 * MQ, CR = 32 * NWC;
    __shared__ float Qs[QR * CG_S];
    __shared__ float Cs[CR * CG_S];
    const int64_t q0 = (int64_t)blockIdx.y * QR, c0 = (int64_t)blockIdx.x * CR;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    f32x16 acc[MQ];
#pragma unroll
    for (int m = 0; m < MQ; ++m)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[m][e] = 0.f;
    constexpr int SLOTS = (QR + CR) * (CG_K / 4);  // float4 slots per K chunk
    static_assert(SLOTS % NT == 0, "staging slots must divide evenly");
    constexpr int PER = SLOTS / NT;
    float4 pre[PER];
    auto fetch = [&](int k0) {  // next chunk -> registers (clamped rows: unconditional loads)
#pragma unroll
        for (int it = 0; it < PER; ++it) {
            const int idx = threadIdx.x + it * NT;
            const int row = idx >> 3, c4 = idx & 7;
            const int kk = min(k0 + c4 * 4, d - 4);
            const float* src = row < QR ? q + min(q0 + row, nq - 1) * d : cent + min(c0 + (row - QR), nlist - 1) * d;
            const float4 v = *(const float4*)(src + kk);  // unconditional: no branch per load
            const bool ok = k0 + c4 * 4 < d;
            pre[it] = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < d; k0 += CG_K) {
#pragma unroll
        for (int it = 0; it < PER; ++it) {
            const int idx = threadIdx.x + it * NT;
            const int row = idx >> 3, c4 = idx & 7;
            float* dst = (row < QR ? Qs + row * CG_S : Cs + (row - QR) * CG_S) + c4 * 4;
            dst[0] = pre[it].x; dst[1] = pre[it].y; dst[2] = pre[it].z; dst[3] = pre[it].w;
        }
        __syncthreads();
        if (k0 + CG_K < d) fetch(k0 + CG_K);  // in flight while this chunk is multiplied
        const float* qa = Qs + (lane & 31) * CG_S + (lane >> 5);
        const float* cb = Cs + (wave * 32 + (lane & 31)) * CG_S + (lane >> 5);
#pragma unroll
        for (int ks = 0; ks < CG_K / 2; ++ks) {
            const float bv = cb[2 * ks];
#pragma unroll
            for (int m = 0; m < MQ; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[m * 32 * CG_S + 2 * ks], bv, acc[m], 0, 0, 0);
        }
        __syncthreads();
    }
    const int64_t c = c0 + wave * 32 + (lane & 31);
    if (c < nlist) {
        const float cnc = cn[c];
#pragma unroll
        for (int m = 0; m < MQ; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t qr = q0 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (qr < nq) S[qr * nlist + c] = cnc - 2.f * acc[m][r];
            }
    }
}

// One wave's share of a 32 x 32 score tile whose K dimension is split over the block's 4 waves (wave w: chunks w, w + 4, ...
// of CG_K floats).  `src[s]` = the row this lane stages in slot s (rows 0..31 of the A side, 32..63 of the B side; lane + 64 s
// = 8 row + float4 column).  DEPTH chunks are requested ahead: a wave walks d / 128 chunks (6 at d = 768), each a dependent
// memory round trip when fetched one ahead (13 us for a 152-tile launch); with DEPTH = 4 the walk is two round trips.
// NCH = chunks per wave (compile time: the ring is indexed statically); acc += A * B^T over this wave's chunks.
template <int NCH, int DEPTH>
__device__ __forceinline__ void ks_wave_tile(f32x16& acc, const float* const (&src)[8], float* st, int wave, int lane) {
    constexpr int D = DEPTH < NCH ? DEPTH : NCH;
    float4 pre[D][8];
    const int kstep = 4 * CG_K;
    const int kw = wave * CG_K;
    const int coff = (lane & 7) * 4;
#pragma unroll
    for (int c = 0; c < D; ++c)
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) pre[c][s2] = *(const float4*)(src[s2] + kw + c * kstep + coff);
    const float* qa = st + (lane & 31) * CG_S + (lane >> 5);
    const float* cb = st + (32 + (lane & 31)) * CG_S + (lane >> 5);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
            const int idx = lane + s2 * 64;
            float* dst = st + (idx >> 3) * CG_S + (idx & 7) * 4;
            const float4 v = pre[c % D][s2];
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
        if (c + D < NCH) {
#pragma unroll
            for (int s2 = 0; s2 < 8; ++s2) pre[c % D][s2] = *(const float4*)(src[s2] + kw + (c + D) * kstep + coff);
        }
#pragma unroll
        for (int ks = 0; ks < CG_K / 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[2 * ks], cb[2 * ks], acc, 0, 0, 0);
    }
}

// Small problems (nlist 256 x 599 queries = 152 tiles): one 32 x 32 tile per block, the K dimension split over 4 waves
// (wave w takes chunks w, w+4, ...), each with its own staging area and a register prefetch of its next chunk; the four
// partial accumulators are added in a fixed order through LDS.  The single-wave version walked 24 chunks serially and was
// bound by 24 load latencies (34 us); a tree of partial sums stays inside the error bound k_coarse_pick assumes.
__global__ void __launch_bounds__(256) k_coarse_gemm_ks(const float* __restrict__ q, const float* __restrict__ cent,
                                                        const float* __restrict__ cn, int64_t nq, int64_t nlist, int d,
                                                        float* __restrict__ S) {
    __shared__ float St[4][64 * CG_S];   // per wave: 32 query rows then 32 centroid rows
    __shared__ float Red[3][64 * 16];
    const int64_t q0 = (int64_t)blockIdx.y * 32, c0 = (int64_t)blockIdx.x * 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* st = St[wave];
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    float4 pre[8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = lane + it * 64;
            const int row = idx >> 3, c4 = idx & 7;
            const int kk = min(k0 + c4 * 4, d - 4);
            const float* src = row < 32 ? q + min(q0 + row, nq - 1) * d : cent + min(c0 + (row - 32), nlist - 1) * d;
            const float4 v = *(const float4*)(src + kk);
            const bool ok = k0 + c4 * 4 < d;
            pre[it] = make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f);
        }
    };
    const int kstep = 4 * CG_K;
    if (d == 768 || d == 256) {  // the shipped feature widths: deep prefetch ring (ks_wave_tile)
        const float* src[8];
#pragma unroll
        for (int s2 = 0; s2 < 8; ++s2) {
            const int row = (lane + s2 * 64) >> 3;
            src[s2] = row < 32 ? q + min(q0 + row, nq - 1) * d : cent + min(c0 + (row - 32), nlist - 1) * d;
        }
        if (d == 768) ks_wave_tile<6, 4>(acc, src, st, wave, lane);
        else ks_wave_tile<2, 2>(acc, src, st, wave, lane);
    } else {
    if (wave * CG_K < d) fetch(wave * CG_K);
    for (int k0 = wave * CG_K; k0 < d; k0 += kstep) {
#pragma unroll
        for (int it = 0; it < 8; ++it) {
            const int idx = lane + it * 64;
            const int row = idx >> 3, c4 = idx & 7;
            float* dst = st + row * CG_S + c4 * 4;
            dst[0] = pre[it].x; dst[1] = pre[it].y; dst[2] = pre[it].z; dst[3] = pre[it].w;
        }
        if (k0 + kstep < d) fetch(k0 + kstep);  // in flight while this chunk is multiplied (wave-private LDS: no barrier)
        const float* qa = st + (lane & 31) * CG_S + (lane >> 5);
        const float* cb = st + (32 + (lane & 31)) * CG_S + (lane >> 5);
#pragma unroll
        for (int ks = 0; ks < CG_K / 2; ++ks) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[2 * ks], cb[2 * ks], acc, 0, 0, 0);
    }
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) Red[wave - 1][e * 64 + lane] = acc[e];
    }
    __syncthreads();
    if (wave == 0) {
        const int64_t c = c0 + (lane & 31);
        if (c < nlist) {
            const float cnc = cn[c];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float dot = ((acc[r] + Red[0][r * 64 + lane]) + Red[1][r * 64 + lane]) + Red[2][r * 64 + lane];
                const int64_t qr = q0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (qr < nq) S[qr * nlist + c] = cnc - 2.f * dot;
            }
        }
    }
}

// k_coarse_pick: one wave per query.  m = min_c S[q][c]; every centroid with S <= m + margin is a candidate
// (margin = 2 * rigorous rounding bound, so the exact winner is always among them -- usually alone); candidates are
// re-evaluated cooperatively in fp64 as sum((q-c)^2) and the exact (distance, id) minimum wins.
__global__ void __launch_bounds__(256) k_coarse_pick(const float* __restrict__ q, const float* __restrict__ cent,
                                                     const float* __restrict__ S, int64_t nq, int64_t nlist, int d, double cmax,
                                                     int64_t* __restrict__ assign) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t qi = (int64_t)blockIdx.x * 4 + wave;
    if (qi >= nq) return;
    const float* row = S + qi * nlist;
    const float* qp = q + qi * d;
    // the query slice of this lane (float4 chunks lane, lane + 64, ...; up to 4 of them = d <= 1024 stay in registers) and the
    // score row are requested together: one memory round trip
    const int d4 = d >> 2;
    float4 xq[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xq[j] = lane + 64 * j < d4 ? ((const float4*)qp)[lane + 64 * j] : make_float4(0.f, 0.f, 0.f, 0.f);
    float m = INFINITY;
    for (int64_t c = lane; c < nlist; c += 64) m = fminf(m, row[c]);
    double qn2 = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        qn2 = fma((double)xq[j].x, (double)xq[j].x, qn2); qn2 = fma((double)xq[j].y, (double)xq[j].y, qn2);
        qn2 = fma((double)xq[j].z, (double)xq[j].z, qn2); qn2 = fma((double)xq[j].w, (double)xq[j].w, qn2);
    }
    for (int e = 256 * 4 + lane; e < d; e += 64) qn2 = fma((double)qp[e], (double)qp[e], qn2);  // (d > 1024 only)
    for (int off = 32; off >= 1; off >>= 1) {
        qn2 += __shfl_xor(qn2, off, 64);
        m = fminf(m, __shfl_xor(m, off, 64));
    }
    // |S_hat - S| <= (2d+4) u (|q| cmax + cmax^2), u = 2^-24; two such errors separate a false winner from the true one
    const double E = (2.0 * d + 4.0) * 5.9604644775390625e-08 * (sqrt(qn2) * cmax + cmax * cmax);
    const float thr = (float)((double)m + 2.0 * E + 1e-30) ;
    const float thr_up = __uint_as_float(__float_as_uint(fabsf(thr)) + 2u);  // round the threshold outwards
    const float lim = thr >= 0.f ? thr_up : -__uint_as_float(__float_as_uint(fabsf(thr)) - 2u);
    double best = INFINITY;
    int64_t besti = INT64_MAX;
    for (int64_t c0 = 0; c0 < nlist; c0 += 64) {
        const int64_t c = c0 + lane;
        const bool cand = c < nlist && row[c] <= lim;
        unsigned long long mask = __ballot(cand);
        while (mask) {
            // two candidates per trip (usually there are one or two in all): both centroids' loads are in flight together
            const int b0 = __builtin_ctzll(mask);
            mask &= mask - 1;
            const bool two = mask != 0;
            const int b1 = two ? __builtin_ctzll(mask) : b0;
            if (two) mask &= mask - 1;
            const float* cp0 = cent + (c0 + b0) * d;
            const float* cp1 = cent + (c0 + b1) * d;
            float4 y0[4], y1[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e4 = min(lane + 64 * j, d4 - 1);
                y0[j] = ((const float4*)cp0)[e4];
                y1[j] = ((const float4*)cp1)[e4];
            }
            double a0 = 0.0, a1 = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (lane + 64 * j < d4) {
                    const double x0 = (double)xq[j].x, x1 = (double)xq[j].y, x2 = (double)xq[j].z, x3 = (double)xq[j].w;
                    double t;
                    t = x0 - (double)y0[j].x; a0 = fma(t, t, a0); t = x1 - (double)y0[j].y; a0 = fma(t, t, a0);
                    t = x2 - (double)y0[j].z; a0 = fma(t, t, a0); t = x3 - (double)y0[j].w; a0 = fma(t, t, a0);
                    t = x0 - (double)y1[j].x; a1 = fma(t, t, a1); t = x1 - (double)y1[j].y; a1 = fma(t, t, a1);
                    t = x2 - (double)y1[j].z; a1 = fma(t, t, a1); t = x3 - (double)y1[j].w; a1 = fma(t, t, a1);
                }
            }
            for (int e = 256 * 4 + lane; e < d; e += 64) {  // (d > 1024 only)
                const double t0 = (double)qp[e] - (double)cp0[e], t1 = (double)qp[e] - (double)cp1[e];
                a0 = fma(t0, t0, a0);
                a1 = fma(t1, t1, a1);
            }
            for (int off = 32; off >= 1; off >>= 1) {
                a0 += __shfl_xor(a0, off, 64);
                a1 += __shfl_xor(a1, off, 64);
            }
            if (a0 < best || (a0 == best && c0 + b0 < besti)) { best = a0; besti = c0 + b0; }
            if (two && (a1 < best || (a1 == best && c0 + b1 < besti))) { best = a1; besti = c0 + b1; }
        }
    }
    if (lane == 0) assign[qi] = besti;
}

// General nprobe: full fp64 distance rows into scratch, then one wave per query extracts the nprobe
// smallest (dist, id) by repeated argmin.  Legacy indices only (tools/cmd/train-index.py used nprobe=9).
__global__ void __launch_bounds__(256) k_coarse_dist(const float* __restrict__ q, const float* __restrict__ cent,
                                                     int64_t nq, int64_t nlist, int d, double* __restrict__ dist) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq * nlist) return;
    const int64_t qi = i / nlist, c = i - qi * nlist;
    const float* a = q + qi * d;
    const float* b = cent + c * d;
    double acc = 0.0;
    for (int e = 0; e < d; ++e) {
        double t = (double)a[e] - (double)b[e];
        acc = fma(t, t, acc);
    }
    dist[i] = acc;
}
__global__ void __launch_bounds__(64) k_coarse_select(double* __restrict__ dist, int64_t nlist, int nprobe,
                                                      int64_t* __restrict__ assign) {
    const int64_t qi = blockIdx.x;
    double* row = dist + qi * nlist;
    const int lane = threadIdx.x;
    for (int p = 0; p < nprobe; ++p) {
        double bdv = INFINITY;
        int64_t biv = INT64_MAX;
        for (int64_t c = lane; c < nlist; c += 64) {
            double v = row[c];
            if (v < bdv) { bdv = v; biv = c; }
        }
        for (int off = 32; off >= 1; off >>= 1) {
            double od = __shfl_xor(bdv, off, 64);
            int64_t oi = __shfl_xor(biv, off, 64);
            if (od < bdv || (od == bdv && oi < biv)) { bdv = od; biv = oi; }
        }
        if (lane == 0) {
            assign[qi * nprobe + p] = biv == INT64_MAX ? -1 : biv;
            if (biv != INT64_MAX) row[biv] = INFINITY;
        }
        __syncthreads();
    }
}

constexpr int KMAX = 8;

struct TopK {
    double d[KMAX];
    int64_t id[KMAX];
    int64_t pos[KMAX];
};
__device__ __forceinline__ bool before(double da, int64_t ia, double db, int64_t ib) { return da < db || (da == db && ia < ib); }
__device__ __forceinline__ void topk_insert(TopK& t, double dv, int64_t idv, int64_t posv) {
    // The list always carries KMAX sorted slots (static register indices); callers emit the first k.
    if (!before(dv, idv, t.d[KMAX - 1], t.id[KMAX - 1])) return;
    t.d[KMAX - 1] = dv;
    t.id[KMAX - 1] = idv;
    t.pos[KMAX - 1] = posv;
#pragma unroll
    for (int s = KMAX - 1; s >= 1; --s) {
        if (before(t.d[s], t.id[s], t.d[s - 1], t.id[s - 1])) {
            const double td = t.d[s]; t.d[s] = t.d[s - 1]; t.d[s - 1] = td;
            const int64_t ti = t.id[s]; t.id[s] = t.id[s - 1]; t.id[s - 1] = ti;
            const int64_t tp = t.pos[s]; t.pos[s] = t.pos[s - 1]; t.pos[s - 1] = tp;
        }
    }
}

// List scan: one 256-thread block per query = 16 groups of 16 lanes.  Group g takes rows g, g+16, ... of the
// probed list(s); inside a group lane s reads float4 chunks s, s+16, ... of the row (16 lanes x 16 B = 256
// contiguous bytes per load, 4 loads in flight per lane) and the 16 partial fp64 sums are combined with four
// xor-shuffles (wavefront-level reduction).  Every lane of a group carries the group's sorted top-8 in
// registers; thread 0 merges the 16 group lists.  ~40 rows per list (web.py:544) => 2-3 rows per group, so the
// whole list is in flight at once instead of being walked serially.
constexpr int SCAN_GROUPS = 16;
__global__ void __launch_bounds__(256) k_scan(const float* __restrict__ q, const int64_t* __restrict__ assign, int nprobe,
                                              const int64_t* __restrict__ list_off, const int64_t* __restrict__ ids,
                                              const float* __restrict__ vecs, int64_t nq, int d, int k,
                                              float* __restrict__ D, int64_t* __restrict__ I, int64_t* __restrict__ P,
                                              int* __restrict__ any_short, int dbg) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int64_t qi = blockIdx.x;
    float* qs = (float*)smem_raw;
    TopK* merge = (TopK*)(smem_raw + align_up((size_t)d * 4, 16));
    for (int e = threadIdx.x; e < d; e += 256) qs[e] = q[qi * d + e];
    __syncthreads();
    TopK t;
#pragma unroll
    for (int s = 0; s < KMAX; ++s) { t.d[s] = INFINITY; t.id[s] = INT64_MAX; t.pos[s] = -1; }
    const int grp = threadIdx.x >> 4, sub = threadIdx.x & 15;
    const int d4 = d >> 2;
    for (int p = 0; p < nprobe; ++p) {
        const int64_t l = assign[qi * nprobe + p];
        if (l < 0) continue;
        const int64_t beg = list_off[l], end = list_off[l + 1];
        for (int64_t r = beg + grp; r < end; r += SCAN_GROUPS) {
            const float4* row = (const float4*)(vecs + r * d);
            double acc = 0.0;
            for (int c0 = sub; c0 < d4; c0 += 64) {
                float4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + 16 * u;
                    v[u] = (c < d4 && !(dbg & 2)) ? row[c] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = c0 + 16 * u;
                    if (c < d4 && !(dbg & 1)) {
                        const float4 qq = *(const float4*)(qs + c * 4);
                        double t0 = (double)qq.x - (double)v[u].x, t1 = (double)qq.y - (double)v[u].y;
                        double t2 = (double)qq.z - (double)v[u].z, t3 = (double)qq.w - (double)v[u].w;
                        acc = fma(t0, t0, acc);
                        acc = fma(t1, t1, acc);
                        acc = fma(t2, t2, acc);
                        acc = fma(t3, t3, acc);
                    }
                }
            }
            for (int off = 8; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
            if (dbg & 1) acc = (double)(r & 1023);
            if (!(dbg & 4)) topk_insert(t, acc, ids[r], r);
            else if (acc < t.d[0]) { t.d[0] = acc; t.id[0] = r; t.pos[0] = r; }
        }
    }
    if (sub == 0) merge[grp] = t;
    __syncthreads();
    // 16 sorted lists x 8 = 128 candidates; thread i ranks candidate i against all others (broadcast LDS reads)
    // under the strict order (distance, id, slot) and, if it lands in the first k, writes that output slot.
    if (threadIdx.x < SCAN_GROUPS * KMAX && !(dbg & 8)) {
        const int me = threadIdx.x;
        const int mg = me / KMAX, ms = me % KMAX;
        const double md = merge[mg].d[ms];
        const int64_t mid = merge[mg].id[ms];
        int rank = 0;
        for (int o = 0; o < SCAN_GROUPS * KMAX; ++o) {
            const double od = merge[o / KMAX].d[o % KMAX];
            const int64_t oid = merge[o / KMAX].id[o % KMAX];
            const bool ob = od < md || (od == md && (oid < mid || (oid == mid && o < me)));
            rank += ob ? 1 : 0;
        }
        if (rank < k) {
            if (mid == INT64_MAX) {  // fewer than k candidates: faiss pads with -1 / FLT_MAX
                D[qi * k + rank] = FLT_MAX;
                I[qi * k + rank] = -1;
                P[qi * k + rank] = -1;
                atomicOr(any_short, 1);
            } else {
                D[qi * k + rank] = (float)md;
                I[qi * k + rank] = mid;
                P[qi * k + rank] = merge[mg].pos[ms];
            }
        }
    }
}

// ---- list-sorted query order (nprobe == 1) ------------------------------------------------------------------------------
// The scan is one block per query.  On the benchmark index 599 queries probe 26 lists (16.5 MB of list rows) and walk 568 MB
// of them; with queries in arrival order every XCD's 4 MB L2 sees all 26 lists, misses, and the launch runs at the ~7.5 TB/s the
// Infinity Cache delivers (76 us).  Sorting the queries by probed list (counting sort: histogram, one-block exclusive scan,
// scatter -- the order INSIDE a list is whatever the atomics give, results do not depend on it) and handing every XCD one
// contiguous range of the sorted order (hardware puts block b on XCD b % 8) leaves each L2 with an eighth of the lists.
// MEASURED (r3l): scan 77.1 -> 74.4 us on the benchmark index, 52.5 -> 52.2 us per clip at B = 16, for 17 us (3.7 us per clip at
// B = 16) of sorting launches: the scan is bound by its longest blocks (the size-biased lists: 416 rows = 26 dependent iterations),
// which the sorted order also packs onto the same XCD, not by where the rows come from.  Opt-in (IVF_SORT=1), off by default.
__global__ void __launch_bounds__(256) k_qsort_hist(const int64_t* __restrict__ assign, int64_t nq, int64_t nlist, int* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const int64_t l = assign[i];
    atomicAdd(&cnt[(l < 0 || l >= nlist) ? nlist : l], 1);  // bucket nlist: queries without a list
}
__global__ void __launch_bounds__(1024) k_qsort_scan(int* __restrict__ cnt, int64_t n) {  // in place: counts -> exclusive offsets
    __shared__ int part[1024];
    const int64_t per = (n + 1023) / 1024;
    const int64_t b = (int64_t)threadIdx.x * per, e = b + per < n ? b + per : n;
    int s = 0;
    for (int64_t i = b; i < e; ++i) s += cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = threadIdx.x >= off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int64_t i = b; i < e; ++i) {
        const int c = cnt[i];
        cnt[i] = run;
        run += c;
    }
}
__global__ void __launch_bounds__(256) k_qsort_scatter(const int64_t* __restrict__ assign, int64_t nq, int64_t nlist, int* __restrict__ off,
                                                       int* __restrict__ perm) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const int64_t l = assign[i];
    perm[atomicAdd(&off[(l < 0 || l >= nlist) ? nlist : l], 1)] = (int)i;
}
// logical index of block b when every XCD (b % 8) takes one contiguous range of [0, nb)
__device__ __forceinline__ int64_t xcd_contiguous(int64_t b, int64_t nb) {
    const int64_t q = nb >> 3, r = nb & 7, xcd = b & 7, slot = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
}

// Specialised scan for d = 64*V (V = 12 for the 768-d v2 index, 4 for the 256-d v1 index): the query chunk of each
// lane lives in registers, every load of TWO rows is in flight before anything is consumed (one memory round trip per
// pair of rows instead of three per row), row indices are clamped so no load sits behind a branch.
// Specialised scan: d = LPR * 4 * VL, LPR lanes per row (16 or 32), G = 256 / LPR row groups, RU rows in flight per group.
// d = 768 uses 32 lanes per row: with 16 (48 floats of query + 96 of rows + fp64 temporaries per lane) the kernel needed
// 345 registers, ran one block per CU and turned the clip's 599 query blocks into three serial rounds of HBM-latency-bound
// work; at 32 lanes per row every block of the launch is resident at once.
template <int VL, int LPR, int RU>
// q and bfeats are NOT __restrict__: the fused blend runs in place (rvcmi_ivf_search_blend passes the same buffer for both).
// (3 blocks per CU: a clip's 599 query blocks must all be resident, see the register note above)
__global__ void __launch_bounds__(256, 3) k_scan_v(const float* q, const int64_t* __restrict__ assign, int nprobe,
                                                   const int64_t* __restrict__ list_off, const int64_t* __restrict__ ids,
                                                   const float* __restrict__ vecs, int64_t nq, int k, float* __restrict__ D,
                                                   int64_t* __restrict__ I, int64_t* __restrict__ P, int* __restrict__ any_short,
                                                   float* bfeats, float rate, float omr, int64_t pos_last, unsigned long long* ts = nullptr,
                                                   const int* __restrict__ perm = nullptr) {
    constexpr int d = LPR * 4 * VL;
    // dev only: wall-clock stamps of block 0's phases (RVCMI_IVF_STAMPS=1)
    auto stamp = [&](int i) {
        if (ts && blockIdx.x == 0 && threadIdx.x == 0) ts[i] = wall_clock64();
    };
    stamp(0);
    __shared__ float bd[KMAX];      // fused blend (bfeats != nullptr): the query's k results, by rank
    __shared__ long long bp[KMAX];
    constexpr int G = 256 / LPR;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    TopK* merge = (TopK*)smem_raw;
    const int64_t qi = perm ? (int64_t)perm[xcd_contiguous(blockIdx.x, gridDim.x)] : (int64_t)blockIdx.x;  // list-sorted order, one range per XCD
    const int grp = threadIdx.x / LPR, sub = threadIdx.x % LPR;
    // the query chunk of this lane, converted to fp64 ONCE (it used to be re-converted for every row: one of the four fp64-rate
    // instructions per element)
    double qd[VL][4];
#pragma unroll
    for (int i = 0; i < VL; ++i) {
        const float4 t4 = *(const float4*)(q + qi * d + (sub + LPR * i) * 4);
        qd[i][0] = (double)t4.x;
        qd[i][1] = (double)t4.y;
        qd[i][2] = (double)t4.z;
        qd[i][3] = (double)t4.w;
    }
    // the group's running top-8 lives in LDS and is maintained by the group's first lane: keeping it in registers (48 per
    // lane, all lanes) plus the unrolled compare-swap network cost ~100 VGPRs; a list has only 2-3 rows per group
    TopK& t = merge[grp];
    if (sub == 0) {
#pragma unroll
        for (int s = 0; s < KMAX; ++s) { t.d[s] = INFINITY; t.id[s] = INT64_MAX; t.pos[s] = -1; }
    }
    for (int p = 0; p < nprobe; ++p) {
        const int64_t l = assign[qi * nprobe + p];
        if (ts && threadIdx.x == 0 && blockIdx.x == 0) { asm volatile("" ::"v"((int)l)); ts[1] = wall_clock64(); }
        if (l < 0) continue;
        const int64_t beg = list_off[l], end = list_off[l + 1];
        if (ts && threadIdx.x == 0 && blockIdx.x == 0) { asm volatile("" ::"v"((int)beg), "v"((int)end)); ts[2] = wall_clock64(); }
        if (end <= beg) continue;
        // Row loop, software-pipelined: the loads of the NEXT 16 rows are in flight while the current ones are reduced (one
        // iteration used to be a full load -> fp64 -> shuffle -> LDS-insertion round trip, 3.5 us; lists are size-biased, the
        // longest one sets the kernel time).  Addresses are clamped to the list's last row, so every load is unconditional.
        auto load_rows = [&](float4(&v)[RU][VL], int64_t(&idv)[RU], int64_t r0) {
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int64_t rr = r0 + u * G;
                const int64_t rc = rr < end ? rr : end - 1;
                const float4* row = (const float4*)(vecs + rc * d);
#pragma unroll
                for (int i = 0; i < VL; ++i) v[u][i] = row[sub + LPR * i];
                idv[u] = ids[rc];
            }
        };
        auto proc_rows = [&](const float4(&v)[RU][VL], const int64_t(&idv)[RU], int64_t r0) {
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                const int64_t rr = r0 + u * G;
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < VL; ++i) {
                    const double t0 = qd[i][0] - (double)v[u][i].x, t1 = qd[i][1] - (double)v[u][i].y;
                    const double t2 = qd[i][2] - (double)v[u][i].z, t3 = qd[i][3] - (double)v[u][i].w;
                    acc = fma(t0, t0, acc);
                    acc = fma(t1, t1, acc);
                    acc = fma(t2, t2, acc);
                    acc = fma(t3, t3, acc);
                }
                for (int off = LPR / 2; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
                if (sub == 0 && rr < end && before(acc, idv[u], t.d[KMAX - 1], t.id[KMAX - 1])) {
                    int s = KMAX - 1;  // insertion into the sorted LDS list
                    while (s > 0 && before(acc, idv[u], t.d[s - 1], t.id[s - 1])) {
                        t.d[s] = t.d[s - 1];
                        t.id[s] = t.id[s - 1];
                        t.pos[s] = t.pos[s - 1];
                        --s;
                    }
                    t.d[s] = acc;
                    t.id[s] = idv[u];
                    t.pos[s] = rr;
                }
            }
        };
        float4 va[RU][VL], vb[RU][VL];
        int64_t ia[RU], ib[RU];
        int64_t r0 = beg + grp;
        stamp(3);
        load_rows(va, ia, r0);
        while (r0 < end) {
            load_rows(vb, ib, r0 + G * RU);
            proc_rows(va, ia, r0);
            r0 += G * RU;
            if (!(r0 < end)) break;
            load_rows(va, ia, r0 + G * RU);
            proc_rows(vb, ib, r0);
            r0 += G * RU;
        }
    }
    stamp(6);
    __syncthreads();
    stamp(7);
    if (threadIdx.x < G * KMAX) {
        const int me = threadIdx.x;
        const int mg = me / KMAX, ms = me % KMAX;
        const double md = merge[mg].d[ms];
        const int64_t mid = merge[mg].id[ms];
        int rank = 0;
#pragma unroll 8
        for (int o = 0; o < G * KMAX; ++o) {
            const double od = merge[o / KMAX].d[o % KMAX];
            const int64_t oid = merge[o / KMAX].id[o % KMAX];
            rank += (od < md || (od == md && (oid < mid || (oid == mid && o < me)))) ? 1 : 0;
        }
        if (rank < k) {
            if (mid == INT64_MAX) {
                D[qi * k + rank] = FLT_MAX;
                I[qi * k + rank] = -1;
                P[qi * k + rank] = -1;
                bd[rank] = FLT_MAX;
                bp[rank] = -1;
                atomicOr(any_short, 1);
            } else {
                D[qi * k + rank] = (float)md;
                I[qi * k + rank] = mid;
                P[qi * k + rank] = merge[mg].pos[ms];
                bd[rank] = (float)md;
                bp[rank] = merge[mg].pos[ms];
            }
        }
    }
    if (bfeats) {
        // pipeline.py:129-138 for this query's row, exactly as k_blend evaluates it (numpy's operation order); the rows were
        // just read by the scan, so the gather hits L2.  Only used without the realtime guard (which is a per-call decision).
#pragma clang fp contract(off)
        __syncthreads();
        float w[KMAX];
        for (int s = 0; s < k; ++s) {
            const float inv = div_rn(1.0f, bd[s]);
            w[s] = mul_rn(inv, inv);
        }
        float sum;
        if (k == 8) {
            sum = add_rn(add_rn(add_rn(w[0], w[1]), add_rn(w[2], w[3])),
                            add_rn(add_rn(w[4], w[5]), add_rn(w[6], w[7])));
        } else {
            sum = w[0];
            for (int s = 1; s < k; ++s) sum = add_rn(sum, w[s]);
        }
        for (int s = 0; s < k; ++s) w[s] = div_rn(w[s], sum);
        long long pp[KMAX];  // gather positions in registers; all KMAX row loads of an element are issued before the sums
#pragma unroll
        for (int s = 0; s < KMAX; ++s) {
            const long long p = s < k ? bp[s] : 0;
            pp[s] = p < 0 ? pos_last : p;
        }
        for (int e = threadIdx.x; e < d; e += 256) {
            float gv[KMAX];
#pragma unroll
            for (int s = 0; s < KMAX; ++s) gv[s] = vecs[pp[s] * d + e];
            const float f = bfeats[qi * d + e];
            float acc = 0.f;
#pragma unroll
            for (int s = 0; s < KMAX; ++s) {
                if (s < k) {
                    const float prod = mul_rn(gv[s], w[s]);
                    acc = s == 0 ? prod : add_rn(acc, prod);
                }
            }
            bfeats[qi * d + e] = add_rn(mul_rn(acc, rate), mul_rn(omr, f));
        }
    }
    stamp(8);
}

// pipeline.py:129-138 with numpy's fp32 operation order:
//   weight = np.square(1/score); weight /= weight.sum(axis=1, keepdims=True)      (pairwise sum of 8)
//   npy = np.sum(big_npy[ix] * weight[..., None], axis=1)                          (sequential over k)
//   feats = npy*index_rate + (1-index_rate)*feats
// One block per query, threads over d.  id -1 gathers big_npy[-1] exactly like numpy does.
__global__ void __launch_bounds__(256) k_blend(float* __restrict__ feats, const float* __restrict__ D,
                                               const int64_t* __restrict__ P, const float* __restrict__ vecs, int d, int k,
                                               int64_t pos_last, float rate, float omr, const int* __restrict__ any_short,
                                               int skip_if_short) {
#pragma clang fp contract(off)
    if (skip_if_short && *any_short) return;
    const int64_t qi = blockIdx.x;
    float w[KMAX];
    for (int s = 0; s < k; ++s) {
        const float inv = div_rn(1.0f, D[qi * k + s]);
        w[s] = mul_rn(inv, inv);
    }
    float sum;
    if (k == 8) {
        sum = add_rn(add_rn(add_rn(w[0], w[1]), add_rn(w[2], w[3])),
                        add_rn(add_rn(w[4], w[5]), add_rn(w[6], w[7])));
    } else {
        sum = w[0];
        for (int s = 1; s < k; ++s) sum = add_rn(sum, w[s]);
    }
    for (int s = 0; s < k; ++s) w[s] = div_rn(w[s], sum);
    int64_t pp[KMAX];  // all KMAX gathers of an element are issued before the sums (a serial load -> use chain per neighbour was 8 L2 round trips)
#pragma unroll
    for (int s = 0; s < KMAX; ++s) {
        const int64_t p = s < k ? P[qi * k + s] : 0;
        pp[s] = p < 0 ? pos_last : p;
    }
    for (int e = threadIdx.x; e < d; e += 256) {
        float gv[KMAX];
#pragma unroll
        for (int s = 0; s < KMAX; ++s) gv[s] = vecs[pp[s] * d + e];
        const float f = feats[qi * d + e];
        float acc = 0.f;
#pragma unroll
        for (int s = 0; s < KMAX; ++s) {
            if (s < k) {
                const float prod = mul_rn(gv[s], w[s]);
                acc = s == 0 ? prod : add_rn(acc, prod);
            }
        }
        feats[qi * d + e] = add_rn(mul_rn(acc, rate), mul_rn(omr, f));
    }
}

// ---- index build (web.py:544-563: index.train = k-means for the nlist centroids, index.add = nearest-centroid lists) ----
// Lloyd update: centroid l <- mean of its members, members in ascending id order, fp64 accumulation (deterministic).
// One block per list, threads over the dimension.
__global__ void __launch_bounds__(256) k_list_mean(const float* __restrict__ x, const int64_t* __restrict__ order,
                                                   const int64_t* __restrict__ off, int d, float* __restrict__ cent) {
    const int64_t l = blockIdx.x;
    const int64_t beg = off[l], end = off[l + 1];
    if (end == beg) return;  // empty list: the host re-seeds it
    for (int e = threadIdx.x; e < d; e += 256) {
        double acc = 0.0;
        for (int64_t i = beg; i < end; ++i) acc += (double)x[order[i] * d + e];
        cent[l * d + e] = (float)(acc / (double)(end - beg));
    }
}
// squared distance (fp64) of every point to its assigned centroid: the k-means objective, one wave per point
__global__ void __launch_bounds__(256) k_assigned_dist(const float* __restrict__ x, const float* __restrict__ cent,
                                                       const int64_t* __restrict__ assign, int64_t n, int d, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n) return;
    const float* xp = x + i * d;
    const float* cp = cent + assign[i] * d;
    double acc = 0.0;
    for (int e = lane; e < d; e += 64) {
        const double t = (double)xp[e] - (double)cp[e];
        acc += t * t;
    }
    for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) out[i] = acc;
}
// vecs[p] = x[order[p]]: the list-major copy of the vectors
__global__ void __launch_bounds__(256) k_gather_rows(const float* __restrict__ x, const int64_t* __restrict__ order, int64_t n, int d,
                                                     float* __restrict__ out) {
    const int64_t p = blockIdx.x;
    const float4* src = (const float4*)(x + order[p] * d);
    float4* dst = (float4*)(out + p * d);
    for (int e = threadIdx.x; e < d / 4; e += 256) dst[e] = src[e];
}

}  // namespace rvcmi
