// Where a long input is cut (infer/modules/vc/pipeline.py:219-236): the quietest sample, |x| summed over one window, within
// +-t_query of every multiple of t_center.  The reference runs `window` numpy passes over the whole file in float64:
//
//   audio_pad = np.pad(audio, (window // 2, window // 2), mode="reflect")
//   audio_sum = zeros;  for i in range(window): audio_sum += abs(audio_pad[i : i - window])
//   cut(t)    = t - t_query + first argmin of audio_sum[t - t_query : t + t_query]
//
// so audio_sum[j] = (((0 + |p[j]|) + |p[j + 1]|) + ... + |p[j + window - 1]|), a fixed order of IEEE fp64 adds.  The kernels follow
// it literally -- no tree, no sliding update, no prefix-sum difference: each of those is mathematically equal and differs in the
// last bits, and a cut that moves by one sample changes every segment's length -- and only at the positions a search window looks at.
// The reflection is index arithmetic; there is no padded copy.  Nothing here multiplies, so there is nothing to contract.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rvcmi {

constexpr int CUT_THREADS = 256;
constexpr int CUT_PER_THREAD = 4;                          // independent positions per thread: four add chains in flight
constexpr int CUT_TILE = CUT_THREADS * CUT_PER_THREAD;     // positions per block
constexpr int RVCMI_CUT_MAX_WINDOW = 1024;                 // LDS staging: CUT_TILE + window - 1 doubles (16 KB at the limit)
constexpr int64_t CUT_NONE = INT64_MAX;                    // "no candidate yet": every real position is lower

struct CutBest {
    double v;
    int64_t pos;
};

// smaller value wins; on equal values the lower position wins.  A comparison with NaN is false: a NaN is never taken.
__device__ __forceinline__ void cut_take(double& bv, int64_t& bp, double v, int64_t p) {
    if (v < bv || (v == bv && p < bp)) {
        bv = v;
        bp = p;
    }
}

// |audio_pad[k]| for k in [0, n + 2 half): np.pad(..., mode="reflect") as index arithmetic (the entry point requires n > window)
__device__ __forceinline__ double cut_abs_padded(const double* __restrict__ a, int64_t n, int half, int64_t k) {
    int64_t i = k - half;
    if (i < 0) i = -i;
    else if (i >= n) i = 2 * n - 2 - i;
    return __builtin_fabs(a[i]);
}

__device__ __forceinline__ void cut_block_reduce(double& bv, int64_t& bp, CutBest* red) {
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_down(bv, o, 64);
        const int64_t op = __shfl_down((long long)bp, o, 64);
        cut_take(bv, bp, ov, op);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[wave].v = bv;
        red[wave].pos = bp;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < CUT_THREADS / 64; ++w) cut_take(bv, bp, red[w].v, red[w].pos);
}

// grid (tiles of a search window, cuts).  Block (x, c) owns positions [lo + x CUT_TILE, ... + CUT_TILE) of the window
// [lo, hi) = [t - t_query, min(t + t_query, n)), t = (c + 1) t_center.  Thread i sums positions i, i + 256, i + 512, i + 768 of the
// tile: at step k the 64 lanes of a wave read 64 consecutive doubles of LDS (no bank conflict at any read width the compiler picks).
static __global__ void __launch_bounds__(CUT_THREADS) k_cut_sums(const double* __restrict__ audio, int64_t n, int window, int64_t t_center,
                                                                 int64_t t_query, int tiles, CutBest* __restrict__ best,
                                                                 double* __restrict__ sums) {
    __shared__ double s_abs[CUT_TILE + RVCMI_CUT_MAX_WINDOW - 1];
    __shared__ CutBest s_red[CUT_THREADS / 64];
    const int64_t t = ((int64_t)blockIdx.y + 1) * t_center;
    const int64_t lo = t - t_query;
    const int64_t hi = t + t_query < n ? t + t_query : n;
    const int64_t base = lo + (int64_t)blockIdx.x * CUT_TILE;  // first position of this tile
    const int half = window / 2;
    const int64_t left = hi - base;                            // positions of this tile inside the window (may be <= 0)
    const int npos = left < CUT_TILE ? (left > 0 ? (int)left : 0) : CUT_TILE;
    const int nstage = npos > 0 ? npos + window - 1 : 0;      // padded indices base .. base + nstage - 1 < n + window
    for (int l = threadIdx.x; l < nstage; l += CUT_THREADS) s_abs[l] = cut_abs_padded(audio, n, half, base + l);
    __syncthreads();
    double acc[CUT_PER_THREAD];
    int idx[CUT_PER_THREAD];
#pragma unroll
    for (int u = 0; u < CUT_PER_THREAD; ++u) {
        const int p = threadIdx.x + u * CUT_THREADS;
        acc[u] = 0.0;
        idx[u] = p < npos ? p : 0;  // a thread past the end of the window re-adds position 0 (staged, never stored) instead of branching
    }
    if (npos > 0) {
        for (int k = 0; k < window; ++k) {
#pragma unroll
            for (int u = 0; u < CUT_PER_THREAD; ++u) acc[u] = acc[u] + s_abs[idx[u] + k];
        }
    }
    double bv = __builtin_inf();
    int64_t bp = CUT_NONE;
#pragma unroll
    for (int u = 0; u < CUT_PER_THREAD; ++u) {
        const int p = threadIdx.x + u * CUT_THREADS;
        if (p < npos) {
            cut_take(bv, bp, acc[u], base + p);
            if (sums) sums[(int64_t)blockIdx.y * 2 * t_query + (base + p - lo)] = acc[u];
        }
    }
    cut_block_reduce(bv, bp, s_red);
    if (threadIdx.x == 0) {
        best[(int64_t)blockIdx.y * tiles + blockIdx.x].v = bv;
        best[(int64_t)blockIdx.y * tiles + blockIdx.x].pos = bp;
    }
}

// one block per cut: the tiles' pairs under the same rule.  A window that holds nothing but NaN has no candidate and yields its
// first position (the reference raises IndexError there; an enqueue-only call cannot raise on data).
static __global__ void __launch_bounds__(CUT_THREADS) k_cut_pick(const CutBest* __restrict__ best, int tiles, int64_t t_center, int64_t t_query,
                                                                 int64_t* __restrict__ cuts) {
    __shared__ CutBest s_red[CUT_THREADS / 64];
    double bv = __builtin_inf();
    int64_t bp = CUT_NONE;
    for (int x = threadIdx.x; x < tiles; x += CUT_THREADS) {
        const CutBest b = best[(int64_t)blockIdx.x * tiles + x];
        cut_take(bv, bp, b.v, b.pos);
    }
    cut_block_reduce(bv, bp, s_red);
    if (threadIdx.x == 0) cuts[blockIdx.x] = bp != CUT_NONE ? bp : ((int64_t)blockIdx.x + 1) * t_center - t_query;
}

}  // namespace rvcmi
