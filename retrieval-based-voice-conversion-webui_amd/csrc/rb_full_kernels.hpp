// Device code of the NSF-HiFi-GAN generator for gfx950 (CDNA4): the fully fused ResBlock1 for C <= 64 (k_rb_full).
//
// Reference semantics reproduced here (file:line in the reference):
//   ResBlock1              rvc/layers/residuals.py:68-85
#pragma once
#include <hip/hip_runtime.h>

#include "mfma_conv.hpp"

namespace rvcmi {

// ------------------------------------------------------------------------------------------------
// Fully fused ResBlock1 (residuals.py:68-85) for C <= 64: all (conv1, conv2) pairs in ONE kernel
// ------------------------------------------------------------------------------------------------
//
// The fp32 residual stream x never leaves the register file: each of the block's 4 waves owns a slab
// of R/4 time rows x ALL channels as MFMA accumulators (conv2 accumulates straight onto x, which IS the
// residual add).  LDS holds only the two activated OpT operand tiles (X = lrelu(x), H = lrelu(conv1)),
// through which the waves exchange their halo rows.  The tile is computed "overlap-save": the block
// loads R rows, every pair runs on all R rows, edge garbage creeps inwards by (p1+p2) rows per pair and
// only the central R - 2*HL rows are stored (HL = sum of the pair halos).  Per resblock: one HBM read of
// x, one HBM write -- instead of one of each per PAIR -- and 2 barriers per pair.
struct RbFullJob {
    const float* src;
    float* dst;
    const void* w1[3];
    const void* w2[3];
    const float* b1[3];
    const float* b2[3];
    long ct1, ct2;
    int k, k_p;
    int dil[3];
    int nd;
    int HL;       // total one-sided halo of the resblock
    int tvalid;   // R - 2*HL
    int ntiles;
};
struct RbFullArgs {
    RbFullJob job[3];
    int L;
    const int* lens;  // ragged batch (item_rows)
    int lmul;
    long bstride;
    int dbg;
    int yh;  // 1: dst streams are fp16 (pack4_h), same element layout
    int xh;  // 1: src (X0, the start of the fp32 residual stream) is fp16 (option X0_F16)
    unsigned long long* ts;  // dbg & 32: per-wave s_memtime stamps [block][wave][16]
    int pad_tap;  // 1: C <= 32 also multiplies the zero taps that round k up to a whole k-group (option RBF_PAD_TAP)
};

constexpr int RBF_G = 32;   // zero guard rows around X (>= max dilated half-width + one padded tap)
constexpr int RBF_G2 = 8;   // zero guard rows around H

template <typename OpT, int C, int MI, int NJ, int KG, int NB, int OCC = 1, int NWV = 4>
static __global__ void __launch_bounds__(64 * NWV, OCC) k_rb_full(RbFullArgs a) {
    constexpr int NT = 64 * NWV;  // NWV waves, each owning a slab of 32*NJ rows
    using TL = Tile<C>;
    constexpr int STRIDE = TL::STRIDE;
    constexpr int SLAB = 32 * NJ;
    constexpr int R = NWV * SLAB;
    constexpr int XROWS = R + 2 * RBF_G;
    constexpr int HROWS = R + 2 * RBF_G2;
    constexpr int CP = 32 * MI;  // padded channel count (C == 16 runs as one 32-channel tile)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* X = smem;
    char* H = smem + (size_t)XROWS * STRIDE;
    float* bias_l = (float*)(smem + (size_t)(XROWS + HROWS) * STRIDE);          // [nd][2][CP]
    unsigned long long* tsl = (unsigned long long*)(bias_l + 3 * 2 * CP);         // dev-only phase stamps

    const RbFullJob& J = a.job[blockIdx.y];
    if ((int)blockIdx.x >= J.ntiles) return;
    const int b = blockIdx.z;
    const int Lb = item_rows(a.lens, b, a.lmul, a.L);  // (a local: see k_rb_pair)
    const int tg0 = blockIdx.x * J.tvalid - J.HL;  // global time of tile row 0
    if (tg0 + J.HL >= Lb) return;  // (ragged batch) no valid row of this tile lies inside the item: block-uniform, before any barrier
    const float* src = J.src + (size_t)b * a.bstride;
    float* dst = J.dst + (size_t)b * a.bstride;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slab = wave * SLAB;
    const int half4 = 4 * (lane >> 5);

    int tsn = 0;
    auto stamp = [&]() {  // dev-only (-DRVCMI_DEV_STAMPS): kept in LDS and flushed once at the end (a global store
#ifdef RVCMI_DEV_STAMPS   // per stamp would sit in front of the next barrier's vmcnt(0))
        if ((a.dbg & 32) && lane == 0 && tsn < 16) tsl[wave * 16 + tsn] = __builtin_readcyclecounter();
#endif
        ++tsn;
    };
    stamp();  // 0

    // Rows of this lane's NJ column tiles that lie outside the utterance must read as zero in every operand tile
    // (each conv zero-pads ITS input).  Interior tiles (the vast majority) skip the masking altogether.
    const bool interior = tg0 >= 0 && tg0 + R <= Lb;  // block-uniform
    unsigned rowmask[NJ];
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
        const int tg = tg0 + slab + jt * 32 + (lane & 31);
        rowmask[jt] = (tg >= 0 && tg < Lb) ? 0xffffffffu : 0u;
    }

    // ---- load x into the accumulator layout ---------------------------------------------------------------
    // A D-layout global access touches 32 rows x 32 bytes per instruction and costs ~54 cycles of the CU's address path
    // (measured); with one block per CU nothing overlaps it.  TIO: the tile is read as whole rows
    // (1 KB contiguous per instruction) into the not-yet-used operand regions of LDS and picked up from there in D layout
    // (row stride C*4 + 16 bytes: 16 consecutive rows hit 16 different 16-byte bank groups); the store goes the same way back.
    constexpr bool TIO = C % 32 == 0;
    constexpr int TS = C * 4 + 16;
    constexpr int C4 = C / 4;
    static_assert(!TIO || (size_t)R * TS <= (size_t)(XROWS + HROWS) * STRIDE, "transposition tile must fit the X | H regions");
    static_assert(!TIO || (R * C4) % NT == 0, "whole batches of row chunks");
    f32x16 xacc[MI][NJ];
    if (a.xh) {  // fp16 X0: half the bytes through HBM and through the LDS transposition
        const _Float16* srch = (const _Float16*)J.src + (size_t)b * a.bstride;
        if constexpr (TIO) {
            constexpr int C8 = C / 8, TSH = C * 2 + 16;
            static_assert((R * C8) % NT == 0, "whole batches of fp16 row chunks");
            constexpr int PERH = R * C8 / NT;
            uint4 v[PERH];
#pragma unroll
            for (int u = 0; u < PERH; ++u) {
                const int idx = (int)threadIdx.x + u * NT;
                const int row = idx / C8, c8 = idx - row * C8;
                const int tg = tg0 + row;
                const int tgc = min(max(tg, 0), Lb - 1);
                v[u] = *(const uint4*)(srch + (size_t)tgc * C + c8 * 8);
                if (tg < 0 || tg >= Lb) v[u] = make_uint4(0u, 0u, 0u, 0u);  // rows outside the utterance read as zero
            }
#pragma unroll
            for (int u = 0; u < PERH; ++u) {
                const int idx = (int)threadIdx.x + u * NT;
                const int row = idx / C8, c8 = idx - row * C8;
                *(uint4*)(smem + (size_t)row * TSH + c8 * 16) = v[u];
            }
            __syncthreads();
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        using h4 = __attribute__((ext_vector_type(4))) _Float16;
                        const h4 q = *(const h4*)(smem + (size_t)(slab + jt * 32 + (lane & 31)) * TSH + (mi * 32 + 8 * g + half4) * 2);
#pragma unroll
                        for (int e = 0; e < 4; ++e) xacc[mi][jt][4 * g + e] = (float)q[e];
                    }
            __syncthreads();  // the guard zeroing and the first publish below overwrite the tile
        } else {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int jt = 0; jt < NJ; ++jt) {
                    const int tg = tg0 + slab + jt * 32 + (lane & 31);
                    const int tgc = min(max(tg, 0), Lb - 1);
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        if (mi * 32 + 8 * g < C) {
                            using h4 = __attribute__((ext_vector_type(4))) _Float16;
                            const h4 q = *(const h4*)(srch + (size_t)tgc * C + mi * 32 + 8 * g + half4);
#pragma unroll
                            for (int e = 0; e < 4; ++e) xacc[mi][jt][4 * g + e] = mask_bits((float)q[e], rowmask[jt]);
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) xacc[mi][jt][4 * g + e] = 0.f;
                        }
                    }
                }
        }
    } else if constexpr (TIO) {
        constexpr int PER = R * C4 / NT;
        float4 v[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = (int)threadIdx.x + u * NT;
            const int row = idx / C4, c4 = idx - row * C4;
            const int tg = tg0 + row;
            const int tgc = min(max(tg, 0), Lb - 1);
            v[u] = *(const float4*)(src + (size_t)tgc * C + c4 * 4);
            if (tg < 0 || tg >= Lb) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);  // rows outside the utterance read as zero
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int idx = (int)threadIdx.x + u * NT;
            const int row = idx / C4, c4 = idx - row * C4;
            *(float4*)(smem + (size_t)row * TS + c4 * 16) = v[u];
        }
        __syncthreads();
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 q = *(const f32x4*)(smem + (size_t)(slab + jt * 32 + (lane & 31)) * TS + (mi * 32 + 8 * g + half4) * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) xacc[mi][jt][4 * g + e] = q[e];
                }
        __syncthreads();  // the guard zeroing and the first publish below overwrite the tile
    } else
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) {
            const int tg = tg0 + slab + jt * 32 + (lane & 31);
            const int tgc = min(max(tg, 0), Lb - 1);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (mi * 32 + 8 * g < C) {  // folds to a constant once the loops are unrolled
                    const f32x4 v = *(const f32x4*)(src + (size_t)tgc * C + mi * 32 + 8 * g + half4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) xacc[mi][jt][4 * g + e] = mask_bits(v[e], rowmask[jt]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) xacc[mi][jt][4 * g + e] = 0.f;
                }
            }
        }
    // (the x loads above are in flight while this runs) zero the guard rows once -- nobody writes them afterwards --
    // and stage every bias vector of the resblock in LDS
    {
        constexpr int W = STRIDE / 16;  // 16-byte words per row
        const uint4 z = make_uint4(0, 0, 0, 0);
        for (int i = threadIdx.x; i < 2 * RBF_G * W; i += NT) {
            const int r = i / W, c = i - r * W;
            const int row = r < RBF_G ? r : RBF_G + R + (r - RBF_G);
            *(uint4*)(X + (size_t)row * STRIDE + c * 16) = z;
        }
        for (int i = threadIdx.x; i < 2 * RBF_G2 * W; i += NT) {
            const int r = i / W, c = i - r * W;
            const int row = r < RBF_G2 ? r : RBF_G2 + R + (r - RBF_G2);
            *(uint4*)(H + (size_t)row * STRIDE + c * 16) = z;
        }
        for (int i = threadIdx.x; i < J.nd * 2 * CP; i += NT) {
            const int m = i / (2 * CP), w = (i / CP) & 1, c = i % CP;
            const float* bp = w ? J.b2[m] : J.b1[m];
            bias_l[i] = c < C ? bp[c] : 0.f;
        }
    }

    stamp();  // 1: x loaded
    typename Op<OpT>::frag A[NB][KG][MI];  // weight register ring, requested one phase ahead of its use
    conv_prefetch<OpT, C, MI, KG, NB>(A, (const OpT*)J.w1[0] + lane * 8, J.ct1, J.k_p);
    char* xw = X + (size_t)(RBF_G + slab + (lane & 31)) * STRIDE + half4 * 2;   // this lane's publish base in X
    char* hw = H + (size_t)(RBF_G2 + slab + (lane & 31)) * STRIDE + half4 * 2;  // ... and in H
    publish_operand<OpT, C, MI, NJ, STRIDE, false>(xw, xacc, rowmask);          // masked already
    stamp();  // 2
    __syncthreads();
    stamp();  // 3

    const char* xl = X + (size_t)(slab + (lane & 31)) * STRIDE + (lane >> 5) * 16;
    const char* hl = H + (size_t)(slab + (lane & 31)) * STRIDE + (lane >> 5) * 16;
    const int p2 = (J.k - 1) / 2;
    // C <= 32: a k-group is 2 (C = 32) or 4 (C = 16) taps and k = 11 / 7 / 3 is packed as 12 / 8 / 4; the K loops stop behind the real taps
    constexpr bool REAL = TL::CC < KG;
    const int nks = (REAL && !a.pad_tap ? J.k : J.k_p) * TL::CC;

    for (int m = 0; m < J.nd; ++m) {
        const int p1 = J.dil[m] * (J.k - 1) / 2;
        // ---- conv1 (dilated) -> h; the accumulators start from b1 ----------------------------------------
        f32x16 hacc[MI][NJ];
        {
            const float* bl = bias_l + (m * 2 + 0) * CP + half4;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bv = *(const f32x4*)(bl + mi * 32 + 8 * g);
#pragma unroll
                    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                        for (int e = 0; e < 4; ++e) hacc[mi][jt][4 * g + e] = bv[e];
                }
        }
        conv_run<OpT, C, MI, NJ, KG, NB, REAL>(hacc, A, xl, (const OpT*)J.w1[m] + lane * 8, J.ct1, J.k_p, RBF_G - p1, J.dil[m], nks);
        conv_prefetch<OpT, C, MI, KG, NB>(A, (const OpT*)J.w2[m] + lane * 8, J.ct2, J.k_p);  // in flight across the publish + barrier
        if (m == 0) stamp();  // 4: conv1 done
        if (interior) publish_operand<OpT, C, MI, NJ, STRIDE, false>(hw, hacc, rowmask);
        else publish_operand<OpT, C, MI, NJ, STRIDE, true>(hw, hacc, rowmask);
        if (m == 0) stamp();  // 5
        __syncthreads();  // h complete; every wave is also done reading X
        if (m == 0) stamp();  // 6
        // ---- conv2 accumulates onto x: x <- (x + b2) + conv2(h) ------------------------------------------
        {
            const float* bl = bias_l + (m * 2 + 1) * CP + half4;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 bv = *(const f32x4*)(bl + mi * 32 + 8 * g);
#pragma unroll
                    for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                        for (int e = 0; e < 4; ++e) xacc[mi][jt][4 * g + e] += bv[e];
                }
        }
        conv_run<OpT, C, MI, NJ, KG, NB, REAL>(xacc, A, hl, (const OpT*)J.w2[m] + lane * 8, J.ct2, J.k_p, RBF_G2 - p2, 1, nks);
        if (m + 1 < J.nd) conv_prefetch<OpT, C, MI, KG, NB>(A, (const OpT*)J.w1[m + 1] + lane * 8, J.ct1, J.k_p);
        if (m == 0) stamp();  // 7: conv2 done
        if (m + 1 < J.nd) {  // publish lrelu(x') for the next pair
            if (interior) publish_operand<OpT, C, MI, NJ, STRIDE, false>(xw, xacc, rowmask);
            else publish_operand<OpT, C, MI, NJ, STRIDE, true>(xw, xacc, rowmask);
            if (m == 0) stamp();  // 8
            __syncthreads();
            if (m == 0) stamp();  // 9
        }
    }
    stamp();  // 10: all pairs done

    // ---- store the valid centre of the tile ---------------------------------------------------------------
    if (a.yh) {  // fp16 output stream: half the LDS round trip and half the store instructions
        _Float16* dsth = (_Float16*)J.dst + (size_t)b * a.bstride;
        if constexpr (TIO) {
            constexpr int TSH = C * 2 + 16;
            constexpr int C8 = C / 8;
            __syncthreads();  // every wave is done with the operand tiles
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        *(uint2*)(smem + (size_t)(slab + jt * 32 + (lane & 31)) * TSH + (mi * 32 + 8 * g + half4) * 2) =
                            pack4_h(xacc[mi][jt][4 * g + 0], xacc[mi][jt][4 * g + 1], xacc[mi][jt][4 * g + 2], xacc[mi][jt][4 * g + 3]);
            __syncthreads();
            if (!(a.dbg & 16)) {
                const int nrow = min(R - 2 * J.HL, Lb - (tg0 + J.HL));
                const int tot = nrow * C8;
                for (int i = threadIdx.x; i < tot; i += NT) {
                    const int r = i / C8, c8 = i - r * C8;
                    const int row = J.HL + r;
                    *(uint4*)(dsth + (size_t)(tg0 + row) * C + c8 * 8) = *(const uint4*)(smem + (size_t)row * TSH + c8 * 16);
                }
            }
        } else if (!(a.dbg & 16)) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int jt = 0; jt < NJ; ++jt) {
                    const int row = slab + jt * 32 + (lane & 31);
                    const int tg = tg0 + row;
                    if (row >= J.HL && row < R - J.HL && tg < Lb) {
#pragma unroll
                        for (int g = 0; g < 4; ++g)
                            if (mi * 32 + 8 * g < C)
                                *(uint2*)(dsth + (size_t)tg * C + mi * 32 + 8 * g + half4) =
                                    pack4_h(xacc[mi][jt][4 * g + 0], xacc[mi][jt][4 * g + 1], xacc[mi][jt][4 * g + 2], xacc[mi][jt][4 * g + 3]);
                    }
                }
        }
    } else if constexpr (TIO) {
        __syncthreads();  // every wave is done with the operand tiles
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 q = {xacc[mi][jt][4 * g + 0], xacc[mi][jt][4 * g + 1], xacc[mi][jt][4 * g + 2], xacc[mi][jt][4 * g + 3]};
                    *(f32x4*)(smem + (size_t)(slab + jt * 32 + (lane & 31)) * TS + (mi * 32 + 8 * g + half4) * 4) = q;
                }
        __syncthreads();
        if (!(a.dbg & 16)) {
            const int nrow = min(R - 2 * J.HL, Lb - (tg0 + J.HL));  // valid rows of this tile that lie inside the utterance
            const int tot = nrow * C4;
            for (int i = threadIdx.x; i < tot; i += NT) {
                const int r = i / C4, c4 = i - r * C4;
                const int row = J.HL + r;
                *(float4*)(dst + (size_t)(tg0 + row) * C + c4 * 4) = *(const float4*)(smem + (size_t)row * TS + c4 * 16);
            }
        }
    } else if (!(a.dbg & 16)) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt) {
                const int row = slab + jt * 32 + (lane & 31);
                const int tg = tg0 + row;
                if (row >= J.HL && row < R - J.HL && tg < Lb) {
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        if (mi * 32 + 8 * g < C) {  // folds to a constant once the loops are unrolled
                            const f32x4 v = {xacc[mi][jt][4 * g + 0], xacc[mi][jt][4 * g + 1], xacc[mi][jt][4 * g + 2], xacc[mi][jt][4 * g + 3]};
                            *(f32x4*)(dst + (size_t)tg * C + mi * 32 + 8 * g + half4) = v;
                        }
                    }
                }
            }
    }
    stamp();  // 11: stores issued
#ifdef RVCMI_DEV_STAMPS
    if ((a.dbg & 32) && lane < 16) {
        const size_t blk = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        a.ts[(blk * NWV + wave) * 16 + lane] = lane < tsn ? tsl[wave * 16 + lane] : 0ull;
    }
#endif
}

}  // namespace rvcmi
