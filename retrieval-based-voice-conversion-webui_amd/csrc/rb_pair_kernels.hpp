// Device code of the NSF-HiFi-GAN generator for gfx950 (CDNA4): one (conv1, conv2) pair of ResBlock1 per launch (k_rb_pair).
//
// Reference semantics reproduced here (file:line in the reference):
//   ResBlock1              rvc/layers/residuals.py:68-85
#pragma once
#include <hip/hip_runtime.h>

#include "mfma_conv.hpp"

namespace rvcmi {

// ------------------------------------------------------------------------------------------------
// Fused ResBlock1 pair (residuals.py:73-82):   x <- conv2(lrelu(conv1_dil(lrelu(x)) + b1)) + b2 + x
// ------------------------------------------------------------------------------------------------
//
// One launch covers pair level m of ALL resblocks of a stage (grid.y = resblock j; they read the same
// or sibling fp32 streams and are independent).  Per block, for one utterance and one time tile:
//   1. stage lrelu(x) as OpT into an LDS tile X of 128 + (k-1)*dil rows           (HBM read #1)
//   2. conv1 (dilated) on MFMA -> 128 rows of h; barrier
//   3. h -> lrelu -> OpT written back INTO THE SAME LDS region (X is dead; rows outside [0,L) are
//      written as zeros because conv2 zero-pads ITS input)                        barrier
//   4. conv2 (dil 1) on MFMA over the h tile -> 128-(k-1) valid output rows
//   5. epilogue: + b2 + residual x (fp32, HBM read #2) -> fp32 store              (HBM write)
// The intermediate never leaves the CU, and the only barriers are around step 3.  A block is
// C/64 waves (each wave owns a 64-channel output slice and streams its own weights), so 2-8 blocks
// share a CU and one block's staging/epilogue overlaps another block's MFMA work.

struct RbJob {
    const float* src;   // x  [B][L][C] fp32
    float* dst;         // x' [B][L][C] fp32
    const void* w1;     // packed conv1 weights
    const void* w2;
    const float* b1;
    const float* b2;
    long ct1, ct2;      // packed elements per 32-channel output tile
    int k_p;            // padded tap count (same for conv1 and conv2)
    int k;              // real kernel size
    int dil;            // conv1 dilation
    int tt2;            // valid outputs per tile = 128 - (k-1)
    int ntiles;
};
struct RbPairArgs {
    RbJob job[4];
    int L;
    const int* lens;  // ragged batch (item_rows)
    int lmul;
    long bstride;
    int dbg;  // timing ablations only (RVCMI_DBG): 2 skip conv1, 4 skip conv2, 16 skip store, 32 phase stamps
    unsigned long long* ts;
};

constexpr int RB_ROWS = 128;  // default conv1 output rows per tile = 4 MFMA column tiles per wave (template NJ overrides)

// Waves are laid out NW (output-channel slices of 32*MI) x NWT (time slabs of 32*NJ_ rows); OCC = waves per SIMD the
// register budget is capped for.
// (Round 5, measured and removed: the lean K loop kconv + LDS-only barriers of k_rb_stream for the C = 256 instantiation -- 253 registers, no
//  spills, parity-green -- ran 0.295 -> 0.320 ms per clip, ABAB x 3 on one lease: with two co-resident blocks at pair level 0 the group
//  structure of conv_run was never the limit, and kconv's 8-deep ring holds twice the weight registers.  DESIGN.md 4f.)
template <typename OpT, int C, int MI, int NW, int KG, int NJ_ = RB_ROWS / 32, int NWT = 1, int OCC = 2>
static __global__ void __launch_bounds__(64 * NW * NWT, OCC) k_rb_pair(RbPairArgs a) {
    constexpr int ROWS = 32 * NJ_ * NWT;  // conv1 output rows per tile
    using TL = Tile<C>;
    using frag = typename Op<OpT>::frag;
    constexpr int STRIDE = TL::STRIDE;
    constexpr int C8 = C / 8;
    constexpr int NT = 64 * NW * NWT;
    constexpr int NJ = NJ_;
    constexpr int NB = 2;
    constexpr int CP = 32 * MI * NW;  // padded channel count
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int bjob = blockIdx.y, btile = blockIdx.x;
    const RbJob& J = a.job[bjob];
    if (btile >= J.ntiles) return;
    const int b = blockIdx.z;
    const int Lb = item_rows(a.lens, b, a.lmul, a.L);  // (a local: writing to the by-value argument struct sends it to scratch)
    if (btile * J.tt2 >= Lb) return;  // (ragged batch) a tile behind the item's end: block-uniform, before any barrier
    const int p2 = (J.k - 1) / 2;
    const int p1 = J.dil * (J.k - 1) / 2;
    const int t0 = btile * J.tt2;          // first output time of this tile
    const int h0 = t0 - p2;                     // global time of h row 0
    const int x0 = h0 - p1;                     // global time of X row 0
    const int xrows = ROWS + (J.k_p - 1) * J.dil;
    const float* src = J.src + (size_t)b * a.bstride;
    float* bias_l = (float*)(smem + (size_t)xrows * STRIDE);  // [2][CP]: b1 then b2
    unsigned long long* tsl = (unsigned long long*)(bias_l + 2 * CP);  // dev-only phase stamps (dbg & 32)
    int tsn = 0;
    auto stamp = [&]() {
#ifdef RVCMI_DEV_STAMPS
        if ((a.dbg & 32) && (threadIdx.x & 63) == 0 && tsn < 8) tsl[(threadIdx.x >> 6) * 8 + tsn] = __builtin_readcyclecounter();
#endif
        ++tsn;
    };
    stamp();  // 0

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int ct0 = (wave % NW) * MI;             // first 32-channel output tile of this wave
    const int slab = (wave / NW) * 32 * NJ_;      // first row of this wave's time slab
    const int half4 = 4 * (lane >> 5);

    // conv1's first weight groups are requested before anything else: their latency hides behind the staging
    frag A[NB][KG][MI];
    conv_prefetch<OpT, C, MI, KG, NB>(A, (const OpT*)J.w1 + (size_t)ct0 * J.ct1 + lane * 8, J.ct1, J.k_p);

    // ---- 1. stage lrelu(x) -> OpT tile.  SB independent 32-byte loads in flight per thread (the accumulators are
    //         not live yet); clamped addresses keep every load unconditional (no exec-masked block per load).
    constexpr int SB = 12;  // 188-row tiles are 23.5 chunks per thread: two batches of 12 (three of 8 cost one more HBM round trip)
    const int total = xrows * C8;
    for (int base = threadIdx.x; base < total; base += SB * NT) {
        float4 lo[SB], hi[SB];
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int idx = min(base + u * NT, total - 1);  // past the tile: re-request its last chunk (an L1 hit), not the neighbour's rows
            const int r = idx / C8;
            const int c8 = idx - r * C8;
            const int gr = x0 + r;
            const int grc = min(max(gr, 0), Lb - 1);
            const float4* p = (const float4*)(src + (size_t)grc * C + c8 * 8);
            lo[u] = p[0];
            hi[u] = p[1];
            if (gr < 0 || gr >= Lb) {
                lo[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                hi[u] = lo[u];
            }
        }
#pragma unroll
        for (int u = 0; u < SB; ++u) {
            const int idx = base + u * NT;
            if (idx >= total) continue;
            const int r = idx / C8;
            const int c8 = idx - r * C8;
            const float f[8] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z, hi[u].w};
            frag v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (OpT)lrelu_op<OpT>(f[e]);
            *(frag*)(smem + (size_t)r * STRIDE + c8 * 16) = v;
        }
    }
    for (int i = threadIdx.x; i < 2 * CP; i += NT) {
        const int c = i % CP;
        bias_l[i] = c < C ? (i < CP ? J.b1[c] : J.b2[c]) : 0.f;
    }
    stamp();  // 1: staged
    __syncthreads();
    stamp();  // 2

    const char* lds_lane = smem + (size_t)(slab + (lane & 31)) * STRIDE + (lane >> 5) * 16;
    f32x16 acc[MI][NJ];
    auto init_bias = [&](const float* bl) {  // accumulators start from the bias: no add in the epilogues
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 bv = *(const f32x4*)(bl + (ct0 + mi) * 32 + 8 * g + half4);
#pragma unroll
                for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[mi][jt][4 * g + e] = bv[e];
            }
    };

    // ---- 2. conv1 -----------------------------------------------------------------------------------
    init_bias(bias_l);
    if (!(a.dbg & 2))
        conv_run<OpT, C, MI, NJ, KG, NB>(acc, A, lds_lane, (const OpT*)J.w1 + (size_t)ct0 * J.ct1 + lane * 8, J.ct1, J.k_p, 0, J.dil);
    conv_prefetch<OpT, C, MI, KG, NB>(A, (const OpT*)J.w2 + (size_t)ct0 * J.ct2 + lane * 8, J.ct2, J.k_p);  // across the barriers
    stamp();  // 3: conv1 done
    __syncthreads();  // every wave has finished reading X

    // ---- 3. h = lrelu(conv1 + b1) -> OpT, in place over X (zero outside the utterance: conv2 pads ITS input) ----
    {
        const bool interior = h0 >= 0 && h0 + ROWS <= Lb;  // block-uniform: no masking needed
        unsigned rowmask[NJ];
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) {
            const int th = h0 + slab + jt * 32 + (lane & 31);
            rowmask[jt] = (th >= 0 && th < Lb) ? 0xffffffffu : 0u;
        }
        char* hw = smem + (size_t)(slab + (lane & 31)) * STRIDE + (ct0 * 32 + half4) * 2;
        if (interior) publish_operand<OpT, C, MI, NJ, STRIDE, false>(hw, acc, rowmask, ct0 * 32);
        else publish_operand<OpT, C, MI, NJ, STRIDE, true>(hw, acc, rowmask, ct0 * 32);
    }
    stamp();  // 4: h published
    __syncthreads();
    stamp();  // 5

    // ---- 4. conv2 (accumulators start from b2) -----------------------------------------------------------
    init_bias(bias_l + CP);
    if (!(a.dbg & 4))
        conv_run<OpT, C, MI, NJ, KG, NB>(acc, A, lds_lane, (const OpT*)J.w2 + (size_t)ct0 * J.ct2 + lane * 8, J.ct2, J.k_p, 0, 1);

    stamp();  // 6: conv2 done
    // ---- 5. epilogue: x' = (conv2 + b2) + x --------------------------------------------------------------
    float* dst = J.dst + (size_t)b * a.bstride;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
        const int o = slab + jt * 32 + (lane & 31);
        const int t = t0 + o;
        const bool valid = o < J.tt2 && t < Lb;
        const int tc = min(t, Lb - 1);
        f32x4 r[MI][4];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if ((ct0 + mi) * 0 + mi * 32 + 8 * g < CP)  // always true; keeps the loads unconditional
                    r[mi][g] = (C % 32 == 0 || (ct0 + mi) * 32 + 8 * g + half4 < C)
                                   ? *(const f32x4*)(src + (size_t)tc * C + min((ct0 + mi) * 32 + 8 * g + half4, C - 4))
                                   : f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid && !(a.dbg & 16)) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = (ct0 + mi) * 32 + 8 * g + half4;
                    if ((C % 32 != 0) && co >= C) continue;
                    f32x4 v = {acc[mi][jt][4 * g + 0], acc[mi][jt][4 * g + 1], acc[mi][jt][4 * g + 2], acc[mi][jt][4 * g + 3]};
                    v += r[mi][g];
                    *(f32x4*)(dst + (size_t)t * C + co) = v;
                }
        }
    }
    stamp();  // 7: stores issued
#ifdef RVCMI_DEV_STAMPS
    if ((a.dbg & 32) && (threadIdx.x & 63) < 8) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.ts[(blk * NW * NWT + (threadIdx.x >> 6)) * 8 + (threadIdx.x & 63)] = tsl[(threadIdx.x >> 6) * 8 + (threadIdx.x & 63)];
    }
#endif
}

}  // namespace rvcmi
