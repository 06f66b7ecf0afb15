// Device code of the NSF-HiFi-GAN generator for gfx950 (CDNA4): conv_post (k_post, k_post_dma) and the debug-tap helpers.
//
// Reference semantics reproduced here (file:line in the reference):
//   stage mean, post, tanh rvc/layers/nsf.py:186-189
#pragma once
#include <hip/hip_runtime.h>

#include "exact_fp.hpp"
#include "mfma_conv.hpp"

namespace rvcmi {

// out[b][t] = tanh(sum_{j,ci} lrelu(x[t-3+j][ci], 0.01) * Wp[j][ci]),  x = ((xa + xb) + xc) / div   (nsf.py:186-189)
// HBM-bound: the last stage is read exactly once with coalesced float4 loads into an LDS tile whose
// row stride C+4 floats keeps every row 16-byte aligned and the per-thread row walk (ds_read_b128, consecutive
// lanes = consecutive rows, 20- or 36-word stride) conflict-free: 56 LDS reads per output instead of 224 scalar ones.
constexpr int POST_TT = 256;  // = blockDim: one output sample per thread (a 128-row tile measured no faster)
// Loops over time tiles (any grid.x).  Measured at B = 1 (2246 tiles, 1536 resident blocks): one tile per block 40-41 us,
// grid = resident blocks 41 us, two tiles for every block 46 us -- the launch is not limited by its last half-empty round.
static __global__ void __launch_bounds__(256) k_post(const float* __restrict__ xa, const float* __restrict__ xb,
                                              const float* __restrict__ xc, const float* __restrict__ Wp /*[7][C]*/,
                                              float* __restrict__ out, int Lmax, int C, float div, int in_half,
                                              const int* __restrict__ lens, int lmul, int dbg = 0 /* timing ablation: 2 = staging only */) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* w = (float*)smem_raw;          // [7][C]
    float* tile = w + 7 * C;              // [POST_TT + 6][C + 4]
    const int b = blockIdx.y;
    const int S = C + 4;
    for (int i = threadIdx.x; i < 7 * C; i += 256) w[i] = Wp[i];
    const int C4 = C >> 2;
    const int L = item_rows(lens, b, lmul, Lmax);  // rows of this item (strides: Lmax); rows [L, Lmax) of the output are zeroed
    const size_t boff = (size_t)b * Lmax * C;
    const int ntiles = (Lmax + POST_TT - 1) / POST_TT;
    for (int ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
        const int t0 = ti * POST_TT;
        if (t0 >= L) {  // block-uniform: a tile behind the item's end
            if (t0 + (int)threadIdx.x < Lmax) out[(size_t)b * Lmax + t0 + threadIdx.x] = 0.f;
            continue;
        }
        // batched, unconditional (clamped) loads: the former per-chunk `if (in range) { load; if (xb) load; if (xc) load }` loop
        // was ~8 serial HBM round trips per thread
        constexpr int SB = 5;
        const int total = (POST_TT + 6) * C4;
        if (in_half) {  // fp16 streams (pack4_h): 8 channels per 16-byte load
            const int C8 = C >> 3;
            const int total8 = (POST_TT + 6) * C8;
            const _Float16 *ha = (const _Float16*)xa, *hb = (const _Float16*)xb, *hc = (const _Float16*)xc;
            for (int base = threadIdx.x; base < total8; base += SB * 256) {
                uint4 va[SB], vb[SB], vc[SB];
                size_t off[SB];
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int idx = min(base + u * 256, total8 - 1);
                    const int r = idx / C8, c8 = idx - r * C8;
                    const int tc = min(max(t0 - 3 + r, 0), L - 1);
                    off[u] = boff + (size_t)tc * C + c8 * 8;
                    va[u] = *(const uint4*)(ha + off[u]);
                }
                if (xb) {
#pragma unroll
                    for (int u = 0; u < SB; ++u) vb[u] = *(const uint4*)(hb + off[u]);
                }
                if (xc) {
#pragma unroll
                    for (int u = 0; u < SB; ++u) vc[u] = *(const uint4*)(hc + off[u]);
                }
#pragma unroll
                for (int u = 0; u < SB; ++u) {
                    const int idx = base + u * 256;
                    if (idx < total8) {
                        const int r = idx / C8, c8 = idx - r * C8;
                        const int t = t0 - 3 + r;
                        float v[8], w2[8];
                        unpack8_h(va[u], v);
                        if (xb) {
                            unpack8_h(vb[u], w2);
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] += w2[e];
                        }
                        if (xc) {
                            unpack8_h(vc[u], w2);
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] += w2[e];
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            float x = v[e];
                            if (div == 3.f) x = div3_exact(x);
                            else if (div != 1.f) x = x / div;
                            x = lrelu(x, 0.01f);
                            v[e] = (t < 0 || t >= L) ? 0.f : x;
                        }
                        *(float4*)(tile + r * S + c8 * 8) = make_float4(v[0], v[1], v[2], v[3]);
                        *(float4*)(tile + r * S + c8 * 8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
                    }
                }
            }
        } else
        for (int base = threadIdx.x; base < total; base += SB * 256) {
            float4 va[SB], vb[SB], vc[SB];
            size_t off[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int idx = min(base + u * 256, total - 1);
                const int r = idx / C4, c4 = idx - r * C4;
                const int tc = min(max(t0 - 3 + r, 0), L - 1);
                off[u] = boff + (size_t)tc * C + c4 * 4;
                va[u] = *(const float4*)(xa + off[u]);
            }
            if (xb) {
#pragma unroll
                for (int u = 0; u < SB; ++u) vb[u] = *(const float4*)(xb + off[u]);
            }
            if (xc) {
#pragma unroll
                for (int u = 0; u < SB; ++u) vc[u] = *(const float4*)(xc + off[u]);
            }
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int idx = base + u * 256;
                if (idx < total) {
                    const int r = idx / C4, c4 = idx - r * C4;
                    const int t = t0 - 3 + r;
                    float4 v = va[u];
                    if (xb) { v.x += vb[u].x; v.y += vb[u].y; v.z += vb[u].z; v.w += vb[u].w; }
                    if (xc) { v.x += vc[u].x; v.y += vc[u].y; v.z += vc[u].z; v.w += vc[u].w; }
                    if (div == 3.f) { v.x = div3_exact(v.x); v.y = div3_exact(v.y); v.z = div3_exact(v.z); v.w = div3_exact(v.w); }
                    else if (div != 1.f) { v.x = v.x / div; v.y = v.y / div; v.z = v.z / div; v.w = v.w / div; }
                    v.x = lrelu(v.x, 0.01f); v.y = lrelu(v.y, 0.01f); v.z = lrelu(v.z, 0.01f); v.w = lrelu(v.w, 0.01f);
                    if (t < 0 || t >= L) v = make_float4(0.f, 0.f, 0.f, 0.f);
                    *(float4*)(tile + r * S + c4 * 4) = v;
                }
            }
        }
        __syncthreads();
        const int t = t0 + threadIdx.x;
        if (dbg & 2) {  // (timing ablation, wrong results: what the staging alone costs)
            if (threadIdx.x == 0) out[(size_t)b * Lmax + t0] = tile[0];
            __syncthreads();
            continue;
        }
        if (t < L) {
            float acc = 0.f;
            for (int j = 0; j < 7; ++j) {
                const float4* row = (const float4*)(tile + (threadIdx.x + j) * S);
                const float4* wj = (const float4*)(w + j * C);
                for (int c = 0; c < C4; ++c) {  // same accumulation order as the scalar loop
                    const float4 xv = row[c], wv = wj[c];
                    acc = fmaf(xv.x, wv.x, acc);
                    acc = fmaf(xv.y, wv.y, acc);
                    acc = fmaf(xv.z, wv.z, acc);
                    acc = fmaf(xv.w, wv.w, acc);
                }
            }
            out[(size_t)b * Lmax + t] = tanhf(acc);
        } else if (t < Lmax) {
            out[(size_t)b * Lmax + t] = 0.f;
        }
        __syncthreads();  // the tile is restaged by the next iteration
    }
}

// ---- k_post with register-free staging (round 6) ------------------------------------------------------------------------------
// Same arithmetic as k_post for the shipped case (three fp16 streams, div = 3); what changes is HOW the bytes arrive.  k_post's block is a
// chain load (15 x 16 B per thread held in registers) -> convert -> barrier -> conv -> barrier, and every value held across the load costs
// registers.  Here a PERSISTENT block walks its tiles and the raw fp16 rows of tile i + 1 travel global -> LDS by LDS-DMA
// (`global_load_lds_dwordx4`: no VGPR round trip, lane-linear 1 KB pieces; a tile's rows are contiguous in a [L][C] stream) while tile i
// is converted (one LDS -> LDS pass: (a + b) + c, div3_exact, lrelu 0.01, fp32) and convolved.  Ordering: the pieces a wave issued are
// retired by ITS `s_waitcnt vmcnt(0)`, then a barrier publishes all waves' pieces (the documented RAW rule for LDS-DMA); `raw` is free for
// the next tile after the barrier that ends the convert pass.
// One 1 KB LDS-DMA piece: lane l's 16 bytes at `g` land at LDS byte address `lds_off` + 16 l (`lds_off` wave-uniform, goes through M0).
// Issued through INLINE ASM on purpose: with `__builtin_amdgcn_global_load_lds` hipcc treats every later LDS read as a possible reader of
// the piece and puts `s_waitcnt vmcnt(0)` in front of it (checked in the ISA of the first version of k_post_dma: the wait sat between the
// prefetch of tile i + 1 and the conv of tile i, so the "prefetch" never overlapped anything and the kernel's phases simply added up).
// The compiler does not see these operations: THE CALLER waits for them with explicit `s_waitcnt vmcnt(N)` (loads retire in order, so hidden
// older operations only make the compiler's own counted waits stricter) and must drain them before the kernel ends.
__device__ __forceinline__ void glds16(const void* g, unsigned lds_off) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(g), "s"(lds_off)
                 : "memory");
}
constexpr int POSTD_TT = 128;  // output rows per tile = threads per block (two waves); three blocks per CU
// Ablations (round 6, B = 1, option POST_DBG): whole kernel 36 us; DMA alone 23 us (113 MB at 4.9 TB/s: three blocks per CU x one 26 KB
// tile in flight each against ~4 us of loaded latency); everything but the DMA ~15 us (LDS-bound: 112 ds_read_b128 per output).  A variant with TWO
// tiles in flight (counted vmcnt, two 75 KB blocks per CU) was built, bit-identical, and measured 46 us: four waves per CU hide even less of the LDS phase.  Removed.
template <int C>
static __global__ void __launch_bounds__(POSTD_TT) k_post_dma(const _Float16* __restrict__ xa, const _Float16* __restrict__ xb,
                                                             const _Float16* __restrict__ xc, const float* __restrict__ Wp /*[7][C]*/,
                                                             float* __restrict__ out, int Lmax, const int* __restrict__ lens, int lmul,
                                                             int dbg /* timing ablations only (wrong results): 1 no DMA, 2 no convert / conv */) {
    constexpr int TT = POSTD_TT, NW = TT / 64, S = C + 4, C8 = C / 8, ROWB = C * 2;
    constexpr int TILEB = (TT + 6) * ROWB;                 // bytes of one stream's rows of a tile
    constexpr int NP = (TILEB + 1023) / 1024, RAWB = NP * 1024;  // 1 KB DMA pieces per stream
    constexpr int PPW0 = (3 * NP + NW - 1) / NW;           // pieces per tile issued by a wave (at most)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* w = (float*)smem_raw;                           // [7][C]
    float* tile = w + 7 * C;                               // [TT + 6][C + 4] fp32
    char* raw = (char*)(tile + (TT + 6) * S);              // [3][RAWB] fp16 rows as they lie in HBM
    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < 7 * C; i += TT) w[i] = Wp[i];
    const int L = item_rows(lens, b, lmul, Lmax);
    const size_t boff = (size_t)b * Lmax * C;
    const int nvalid = (L + TT - 1) / TT, nall = (Lmax + TT - 1) / TT;
    const char* src[3] = {(const char*)(xa + boff), (const char*)(xb + boff), (const char*)(xc + boff)};
    const unsigned raw_off = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(const __attribute__((address_space(3))) char*)raw);

    auto issue = [&](int ti) {  // the (TT + 6) rows [t0 - 3, t0 + TT + 3) of the three streams; rows outside [0, L) are clamped here, zeroed in convert
        if (dbg & 1) return;
        const int t0 = ti * TT;
#pragma unroll
        for (int p0 = 0; p0 < PPW0; ++p0) {
            const int p = p0 * NW + wave;  // wave-uniform
            if (p < 3 * NP) {
                const int st = p / NP, pp = p - st * NP;
                const int o = pp * 1024 + lane * 16;
                const int r = o / ROWB, col = o - r * ROWB;
                const int tc = min(max(t0 - 3 + r, 0), L - 1);
                glds16(src[st] + (size_t)tc * ROWB + col, raw_off + (unsigned)(st * RAWB + pp * 1024));
            }
        }
    };

    int ti = blockIdx.x;
    if (ti < nvalid) issue(ti);
    for (; ti < nvalid; ti += gridDim.x) {
        const int t0 = ti * TT;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the pieces THIS wave issued have landed ...
        lds_barrier();                                   // ... and so have everybody's; the previous tile's conv is done with `tile`
        if (dbg & 2) {
            lds_barrier();
            if (ti + (int)gridDim.x < nvalid) issue(ti + gridDim.x);
            if (tid == 0) out[(size_t)b * Lmax + t0] = *(const float*)raw;
            continue;
        }
        for (int idx = tid; idx < (TT + 6) * C8; idx += TT) {
            const int r = idx / C8, c8 = idx - r * C8;
            const int t = t0 - 3 + r;
            float v[8], u[8];
            unpack8_h(*(const uint4*)(raw + r * ROWB + c8 * 16), v);
            unpack8_h(*(const uint4*)(raw + RAWB + r * ROWB + c8 * 16), u);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] += u[e];
            unpack8_h(*(const uint4*)(raw + 2 * RAWB + r * ROWB + c8 * 16), u);
            const bool in = t >= 0 && t < L;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = in ? lrelu(div3_exact(v[e] + u[e]), 0.01f) : 0.f;
            *(float4*)(tile + r * S + c8 * 8) = make_float4(v[0], v[1], v[2], v[3]);
            *(float4*)(tile + r * S + c8 * 8 + 4) = make_float4(v[4], v[5], v[6], v[7]);
        }
        lds_barrier();  // the tile is complete and `raw` is free
        if (ti + (int)gridDim.x < nvalid) issue(ti + gridDim.x);  // flies during the conv below
        const int t = t0 + tid;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const float4* row = (const float4*)(tile + (tid + j) * S);
            const float4* wj = (const float4*)(w + j * C);
#pragma unroll
            for (int c = 0; c < C / 4; ++c) {  // same accumulation order as k_post / the scalar loop
                const float4 xv = row[c], wv = wj[c];
                acc = fmaf(xv.x, wv.x, acc);
                acc = fmaf(xv.y, wv.y, acc);
                acc = fmaf(xv.z, wv.z, acc);
                acc = fmaf(xv.w, wv.w, acc);
            }
        }
        if (t < L) out[(size_t)b * Lmax + t] = tanhf(acc);
        else if (t < Lmax) out[(size_t)b * Lmax + t] = 0.f;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (nothing is in flight here by construction; the compiler cannot know)
    for (ti = blockIdx.x; ti < nall; ti += gridDim.x)  // (ragged batch) tiles behind the item's end
        if (ti >= nvalid && ti * TT + tid < Lmax) out[(size_t)b * Lmax + ti * TT + tid] = 0.f;
}
template <int C>
static constexpr size_t post_dma_smem() {
    return (size_t)(7 * C + (POSTD_TT + 6) * (C + 4)) * 4 + (size_t)3 * (((POSTD_TT + 6) * C * 2 + 1023) / 1024) * 1024;
}

// ... of fp16 streams (Y_F16)
static __global__ void __launch_bounds__(256) k_sum3h(const _Float16* __restrict__ a, const _Float16* __restrict__ b,
                                               const _Float16* __restrict__ c, float* __restrict__ y, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = ((float)a[i] + (b ? (float)b[i] : 0.f)) + (c ? (float)c[i] : 0.f);
}
static __global__ void __launch_bounds__(256) k_h2f(const _Float16* __restrict__ a, float* __restrict__ y, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = (float)a[i];
}
// y = (a + b) + c   (debug tap of the stage sum only)
static __global__ void __launch_bounds__(256) k_sum3(const float* __restrict__ a, const float* __restrict__ b,
                                              const float* __restrict__ c, float* __restrict__ y, size_t n) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = (a[i] + (b ? b[i] : 0.f)) + (c ? c[i] : 0.f);
}

// channels-last fp32 [B][L][C] -> channel-first [B][C][L] (debug taps only)
static __global__ void __launch_bounds__(256) k_cl_to_cf(const float* __restrict__ in, float* __restrict__ out, int L, int C) {
    const int b = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)L * C) return;
    const int c = (int)(i / L);
    const int t = (int)(i - (size_t)c * L);
    out[(size_t)b * L * C + i] = in[((size_t)b * L + t) * C + c];
}

}  // namespace rvcmi
