// Device code of the NSF-HiFi-GAN generator for gfx950 (CDNA4): the polyphase upsampler with the noise conv (k_ups).
//
// Reference semantics reproduced here (file:line in the reference):
//   ups / noise_convs      rvc/layers/nsf.py:169-174
//   stage mean             rvc/layers/nsf.py:186
#pragma once
#include <hip/hip_runtime.h>

#include "exact_fp.hpp"
#include "mfma_conv.hpp"

namespace rvcmi {

// ------------------------------------------------------------------------------------------------
// Polyphase transposed convolution + noise conv (nsf.py:171-174):
//   X0[q*u + r] = b + sum_j lrelu(x)[q + off_r - j] * Wt[:, :, cm_r + j*u]  +  noise_conv(har)[q*u + r]
// ------------------------------------------------------------------------------------------------
//
// x = ((in_a + in_b) + in_c) / div is the mean of the previous stage's resblocks (nsf.py:186).  The
// activated input tile is staged ONCE per block and shared by every phase r and output-channel group
// ("virtual tile") the block's waves walk through; the epilogue adds the bias and the strided 1->C
// noise convolution (VALU, k = 2*s taps of the har excitation) so X0 is written exactly once.
struct UpsArgs {
    const float* in_a;
    const float* in_b;
    const float* in_c;
    int in_half;  // 1: in_a / in_b / in_c are fp16 streams (pack4_h) with the same [B][Lin][cin] element layout
    int in_raw;   // 1 (round 6, stage 0): in_a is ALREADY the activated operand tile source -- conv_pre wrote to_op(lrelu(conv + bias + cond, 0.1)),
                  //    exactly what this staging would compute from its fp32 output (div = 1, one input) -- rows are copied, 16 bytes per chunk
    float div;
    int Lin, cin;
    long in_bstride;
    const void* w;
    long ct_stride;
    long ph_w_off[16];
    int ph_in_off[16];
    int ntaps_p, u, cout;
    int lo;          // lowest input-row offset any (phase, tap) touches relative to q
    int tile_rows;
    const float* bias;
    float* out;
    int out_half;  // 1: X0 is written as fp16 (pack4_h; option X0_F16, stages whose ResBlocks run on k_rb_full), same element layout
    int out_tr;    // 1: the block owns WHOLE output rows (every phase, every channel: gridDim.y == 1) and stores them row-wise through an LDS
                   //    tile at byte offset out_tr_off of the dynamic LDS: each D-layout store touched 8 (fp16) / 16 (fp32) bytes of 32 rows --
                   //    16 partial writes per 128-byte line, 1.6 TB/s -- the row-wise stores write whole lines
    int out_tr_off;
    int out_tw_off;  // > 0 (round 6; NJ == 1, fp16 X0, the block does NOT own whole rows -- stage 1 of v2/48k): byte offset of four wave-private
                     //    transposition tiles [32][MI * 64 + 16 B]: a wave's virtual tile (32 rows x MI * 32 channels) is written there in D layout
                     //    and stored from there as 16 bytes per lane, eight lanes = one whole 128-byte line of a row
    long out_bstride;
    const float* addend;  // optional [B][Lin*u][cout] fp32 added in the epilogue (noise conv done by the MFMA conv)
    const float* har;  // [B][Lh] or nullptr (no-f0 generator / addend in use)
    int Lh;
    int Lh_stride;     // elements between the items of har (= the longest item's Lh)
    const int* lens;   // ragged batch (item_rows): Lin = lens[b] * lmul, Lh = lens[b] * lhmul
    int lmul, lhmul;
    const float* Wn;   // [nk][cout]
    const float* bn;
    int nk, ns, npad;
    const void* wnz;   // nz_k1: noise weights packed as ONE MFMA k-step [co_tile][lane][8] (taps >= nk are zero)
    int nz_k1;         // 1: the <=16-tap noise conv runs as one extra k-step fed from an fp16 copy of the har span in LDS
    int nvt, cog, vpw;
    int dbg;  // timing ablations only: 1 skip staging loads, 2 skip MFMA, 4 skip noise conv, 16 skip store
    int bias_off;      // > 0: byte offset of a [2][cout] fp32 LDS copy of bias / bn, staged with the tile (round 5: the epilogue's bias
                       // vectors were a dependent global round trip behind the K loop of every virtual tile)
};

constexpr int UPS_BLOCKS = 2;  // blocks per CU the register budget is capped for: one block stages / stores while the other multiplies
template <typename OpT, int CIN, int MI, int WV, int NJ = 4>
static __global__ void __launch_bounds__(256, UPS_BLOCKS) k_ups(UpsArgs a) {
    using TL = Tile<CIN>;
    using frag = typename Op<OpT>::frag;
    constexpr int STRIDE = TL::STRIDE;
    constexpr int C8 = CIN / 8;
    constexpr int WT = 4 / WV;
    constexpr int TQ = 32 * NJ * WT;
    constexpr int SB = 5;  // chunk loads (x 3 inputs) in flight per thread: 1280 chunks per pass cover the 1056 / 1048 of the two HBM-bound stages in ONE pass (8 cost the C_in = 64 instantiation its fourth resident block: 134 registers)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.z;
    const int q0 = blockIdx.x * TQ;
    const int Linb = item_rows(a.lens, b, a.lmul, a.Lin), Lhb = item_rows(a.lens, b, a.lhmul, a.Lh);  // (locals: see k_rb_pair)
    if (q0 >= Linb) return;  // (ragged batch) a tile behind the item's end: block-uniform, before the barrier
    const int g0 = q0 + a.lo;
    const size_t boff = (size_t)b * a.in_bstride;

    // nz_k1: the excitation samples this block's output rows can touch -- requested FIRST (two per thread cover the usual spans),
    // together with this wave's bias vectors: with the tile's own loads they are ONE memory round trip instead of three dependent
    // ones (a block is ~4 round trips long; measured 20 us per 64-row tile at 3 blocks per CU)
    const int us = a.u * a.ns;
    const long hbase = (long)q0 * us - a.npad;
    const int hspan = TQ * us + 16;
    float hpre[2] = {0.f, 0.f};
    if (a.nz_k1) {
        const float* hp = a.har + (size_t)b * a.Lh_stride;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long idx = hbase + (int)threadIdx.x + 256 * j;
            const long idc = min(max(idx, 0L), (long)Lhb - 1);
            const float v = hp[idc];
            hpre[j] = (idx >= 0 && idx < Lhb && (int)threadIdx.x + 256 * j < hspan) ? v : 0.f;
        }
    }
    float* bias_l = (float*)(smem + a.bias_off);
    if (a.bias_off) {
        for (int i = threadIdx.x; i < 2 * a.cout; i += 256) bias_l[i] = i < a.cout ? a.bias[i] : (a.bn ? a.bn[i - a.cout] : 0.f);
    }
    const int total = a.tile_rows * C8;
    // Round 6: EVERY load of a batch is issued before the first one is used.  The loop used to read `load a; if (in_b) load b; if (in_c) load c`
    // per chunk; hipcc compiled each conditional load into its own block with `s_waitcnt vmcnt(0)` behind it -- 24 DEPENDENT memory round trips
    // per thread and tile, one 4 KB wave-load in flight per wave (found in the ISA after the timing ablations showed the staging alone at
    // 46 of ups_c128's 60 us = 2.4 TB/s, against 23 us for the same bytes through k_post_dma).  Now the pointers of absent streams alias in_a
    // (unconditional loads) and only the register adds are conditional.
    auto convert_store = [&](int idx, float (&f)[8], bool ok) {
        const int r = idx / C8;
        const int c8 = idx - r * C8;
        if (!ok) {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = 0.f;
        }
        frag v;
        if (a.div == 3.f) {  // the three ResBlocks of every shipped config: the short exact quotient, one v_mul + one v_med3 lrelu
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (OpT)lrelu_op<OpT>(div3_exact(f[e]));
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float x = f[e];
                if (a.div != 1.f) x = x / a.div;
                v[e] = to_op<OpT>(lrelu(x, 0.1f));
            }
        }
        *(frag*)(smem + (size_t)r * STRIDE + c8 * 16) = v;
    };
    if (a.in_raw) {
        const OpT* pa = (const OpT*)a.in_a;
        constexpr int SR = 8;
        for (int base = threadIdx.x; base < total; base += SR * 256) {
            uint4 rr[SR];
#pragma unroll
            for (int u = 0; u < SR; ++u) {
                const int idx = min(base + u * 256, total - 1);
                const int r = idx / C8;
                const int c8 = idx - r * C8;
                const int grc = min(max(g0 + r, 0), Linb - 1);
                rr[u] = *(const uint4*)(pa + boff + (size_t)grc * CIN + c8 * 8);
            }
#pragma unroll
            for (int u = 0; u < SR; ++u) {
                const int idx = base + u * 256;
                if (idx >= total) continue;
                const int r = idx / C8;
                const int c8 = idx - r * C8;
                const int gr = g0 + r;
                *(uint4*)(smem + (size_t)r * STRIDE + c8 * 16) = (gr >= 0 && gr < Linb) ? rr[u] : uint4{0u, 0u, 0u, 0u};
            }
        }
    } else if (a.in_half) {  // fp16 streams: one 16-byte load per input and chunk
        const _Float16* pa = (const _Float16*)a.in_a;
        const _Float16* pb = a.in_b ? (const _Float16*)a.in_b : pa;
        const _Float16* pc = a.in_c ? (const _Float16*)a.in_c : pa;
        for (int base = threadIdx.x; base < total; base += SB * 256) {
            uint4 ra[SB], rb[SB], rc[SB];
            size_t off[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int idx = min(base + u * 256, total - 1);  // past the tile: re-request its last chunk (an L1 hit), not the neighbour's rows
                const int r = idx / C8;
                const int c8 = idx - r * C8;
                const int grc = min(max(g0 + r, 0), Linb - 1);  // clamped address: unconditional loads
                off[u] = boff + (size_t)grc * CIN + c8 * 8;
                ra[u] = *(const uint4*)(pa + off[u]);
            }
#pragma unroll
            for (int u = 0; u < SB; ++u) rb[u] = *(const uint4*)(pb + off[u]);
#pragma unroll
            for (int u = 0; u < SB; ++u) rc[u] = *(const uint4*)(pc + off[u]);
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int idx = base + u * 256;
                if (idx >= total) continue;
                float f[8], t[8];
                unpack8_h(ra[u], f);
                if (a.in_b) {
                    unpack8_h(rb[u], t);
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] += t[e];
                }
                if (a.in_c) {
                    unpack8_h(rc[u], t);
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] += t[e];
                }
                const int gr = g0 + idx / C8;
                convert_store(idx, f, gr >= 0 && gr < Linb);
            }
        }
    } else {  // fp32 streams (stage 0 reads conv_pre's output, stage 1 the fp32 streams of k_rb_pair<256>): two 16-byte loads per input and chunk
        constexpr int SF = 4;
        const float* pb = a.in_b ? a.in_b : a.in_a;
        const float* pc = a.in_c ? a.in_c : a.in_a;
        for (int base = threadIdx.x; base < total; base += SF * 256) {
            float4 la[SF], ha[SF], lb[SF], hb[SF], lc[SF], hc[SF];
            size_t off[SF];
#pragma unroll
            for (int u = 0; u < SF; ++u) {
                const int idx = min(base + u * 256, total - 1);
                const int r = idx / C8;
                const int c8 = idx - r * C8;
                const int grc = min(max(g0 + r, 0), Linb - 1);
                off[u] = boff + (size_t)grc * CIN + c8 * 8;
                la[u] = *(const float4*)(a.in_a + off[u]);
                ha[u] = *(const float4*)(a.in_a + off[u] + 4);
            }
#pragma unroll
            for (int u = 0; u < SF; ++u) {
                lb[u] = *(const float4*)(pb + off[u]);
                hb[u] = *(const float4*)(pb + off[u] + 4);
            }
#pragma unroll
            for (int u = 0; u < SF; ++u) {
                lc[u] = *(const float4*)(pc + off[u]);
                hc[u] = *(const float4*)(pc + off[u] + 4);
            }
#pragma unroll
            for (int u = 0; u < SF; ++u) {
                const int idx = base + u * 256;
                if (idx >= total) continue;
                float f[8] = {la[u].x, la[u].y, la[u].z, la[u].w, ha[u].x, ha[u].y, ha[u].z, ha[u].w};
                if (a.in_b) {
                    f[0] += lb[u].x; f[1] += lb[u].y; f[2] += lb[u].z; f[3] += lb[u].w; f[4] += hb[u].x; f[5] += hb[u].y; f[6] += hb[u].z; f[7] += hb[u].w;
                }
                if (a.in_c) {
                    f[0] += lc[u].x; f[1] += lc[u].y; f[2] += lc[u].z; f[3] += lc[u].w; f[4] += hc[u].x; f[5] += hc[u].y; f[6] += hc[u].z; f[7] += hc[u].w;
                }
                const int gr = g0 + idx / C8;
                convert_store(idx, f, gr >= 0 && gr < Linb);
            }
        }
    }
    // nz_k1: fp16 copy of the excitation samples every output row of this block can touch (zero outside the signal)
    OpT* har16 = (OpT*)(smem + (size_t)a.tile_rows * STRIDE);
    if (a.nz_k1) {
        const float* hp = a.har + (size_t)b * a.Lh_stride;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if ((int)threadIdx.x + 256 * j < hspan) har16[threadIdx.x + 256 * j] = to_op<OpT>(hpre[j]);
        for (int i = threadIdx.x + 512; i < hspan; i += 256) {  // (spans beyond 512 samples: large noise strides)
            const long idx = hbase + i;
            har16[i] = (idx >= 0 && idx < Lhb) ? to_op<OpT>(hp[idx]) : (OpT)0.f;
        }
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int wv = wave % WV, wt = wave / WV;
    const int tw0 = wt * NJ * 32;
    const char* lds_lane = smem + (size_t)(tw0 + (lane & 31)) * STRIDE + (lane >> 5) * 16;
    const float* har = (a.har && !a.nz_k1) ? a.har + (size_t)b * a.Lh_stride : nullptr;  // VALU noise path only
    float* out = a.out + (size_t)b * a.out_bstride;

    for (int i = 0; i < a.vpw; ++i) {
        const int vt = ((int)blockIdx.y * WV + wv) * a.vpw + i;
        if (vt >= a.nvt) break;
        const int r = vt / a.cog;
        const int ct0 = (vt - r * a.cog) * MI;
        f32x16 acc[MI][NJ];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[mi][jt][e] = 0.f;
        const OpT* wlane = (const OpT*)a.w + a.ph_w_off[r] + (size_t)ct0 * a.ct_stride + lane * 8;
        // (requesting the epilogue's bias vectors here, before the K loop, costs 78 registers = one resident block per CU:
        //  ups_c128 65 -> 78 us on one lease, ABAB.  Occupancy, not the number of dependent round trips, is what this kernel lives on.)
// (a 4-group weight ring for the one-tile waves: 148 -> 200 VGPRs, 3 -> 2 blocks per CU; C_in 256 unchanged, 128 slower)
        // (round 5, measured: requesting the first virtual tile's weights BEFORE the staging -- conv_prefetch hoisted, conv_run here -- costs
        //  154 -> 214 registers at C_in = 128 / 256, i.e. 3 -> 2 resident blocks, like every other value held across the staging)
        if (!(a.dbg & 2)) conv_core<OpT, CIN, MI, NJ>(acc, lds_lane, wlane, a.ct_stride, a.ntaps_p, a.ph_in_off[r] - a.lo, -1);
        if (a.nz_k1) {  // + noise_convs[i](har): one k-step, B = the row's 16-sample window (nsf.py:173-174)
            frag An[MI], Bn[NJ];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) An[mi] = *(const frag*)((const OpT*)a.wnz + (size_t)(ct0 + mi) * 512 + lane * 8);
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt) {
                const int ql = tw0 + jt * 32 + (lane & 31);
                const unsigned* wp = (const unsigned*)(har16 + ql * us + r * a.ns + 8 * (lane >> 5));  // 4-byte aligned (ns even)
                union { unsigned u[4]; frag f; } cv;
#pragma unroll
                for (int e = 0; e < 4; ++e) cv.u[e] = wp[e];
                Bn[jt] = cv.f;
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int jt = 0; jt < NJ; ++jt) acc[mi][jt] = Op<OpT>::mfma(An[mi], Bn[jt], acc[mi][jt]);
        }

        const float* addend = a.addend ? a.addend + (size_t)b * a.out_bstride : nullptr;
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) {
            const int q = q0 + tw0 + jt * 32 + (lane & 31);
            const bool valid = q < Linb;
            const int t = min(q, Linb - 1) * a.u + r;  // clamped: loads below stay unconditional
            // noise conv for this output row: nv[mi][g] (4 channels each) += har[t*s - pad + j] * Wn[j][co]
            f32x4 nv[MI][4];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = min((ct0 + mi) * 32 + 8 * g + 4 * (lane >> 5), a.cout - 4);
                    nv[mi][g] = addend ? *(const f32x4*)(addend + (size_t)t * a.cout + co) : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            if (har && !(a.dbg & 4)) {
                const int hb = t * a.ns - a.npad;
                for (int j = 0; j < a.nk; ++j) {
                    const int hi = hb + j;
                    const float hv = (hi >= 0 && hi < Lhb) ? har[hi] : 0.f;
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int co = min((ct0 + mi) * 32 + 8 * g + 4 * (lane >> 5), a.cout - 4);
                            const f32x4 wv4 = *(const f32x4*)(a.Wn + (size_t)j * a.cout + co);
                            nv[mi][g] += wv4 * hv;
                        }
                }
            }
            if (valid && !(a.dbg & 16)) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int co = (ct0 + mi) * 32 + 8 * g + 4 * (lane >> 5);
                        if (co >= a.cout) continue;
                        f32x4 v = {acc[mi][jt][4 * g + 0], acc[mi][jt][4 * g + 1], acc[mi][jt][4 * g + 2], acc[mi][jt][4 * g + 3]};
                        const float* bsrc = a.bias_off ? bias_l : a.bias;
                        const float* bnsrc = a.bias_off ? bias_l + a.cout : a.bn;
                        v += *(const f32x4*)(bsrc + co);
                        if (har) v += nv[mi][g] + *(const f32x4*)(bnsrc + co);  // x + (noise_conv + its bias), nsf.py:173-174
                        else if (addend) v += nv[mi][g];                       // the addend already carries the noise bias
                        else if (a.nz_k1) v += *(const f32x4*)(bnsrc + co);
                        if (a.out_tr) {  // row (q - q0) * u + r of the block's output tile; row pitch = cout elements + 16 bytes
                            const int orow = (tw0 + jt * 32 + (lane & 31)) * a.u + r;
                            char* ot = smem + a.out_tr_off;
                            if (a.out_half) *(uint2*)(ot + (size_t)orow * (a.cout * 2 + 16) + co * 2) = pack4_h(v[0], v[1], v[2], v[3]);
                            else *(f32x4*)(ot + (size_t)orow * (a.cout * 4 + 16) + co * 4) = v;
                        } else if (NJ == 1 && a.out_tw_off) {
                            *(uint2*)(smem + a.out_tw_off + (wave * 32 + (lane & 31)) * (MI * 64 + 16) + (mi * 32 + 8 * g + 4 * (lane >> 5)) * 2) =
                                pack4_h(v[0], v[1], v[2], v[3]);
                        } else if (a.out_half) *(uint2*)((_Float16*)a.out + (size_t)b * a.out_bstride + (size_t)t * a.cout + co) = pack4_h(v[0], v[1], v[2], v[3]);
                        else *(f32x4*)(out + (size_t)t * a.cout + co) = v;
                    }
            }
        }
        if (NJ == 1 && a.out_tw_off && !(a.dbg & 16)) {
            // (wave-private: a wave's LDS operations execute in order, no barrier; each D-layout global store touched 8 bytes of 32 different rows)
            constexpr int TWP = MI * 64 + 16, CPR = MI * 4;
            const char* sc = smem + a.out_tw_off + wave * 32 * TWP;
            for (int i2 = lane; i2 < 32 * CPR; i2 += 64) {
                const int row = i2 / CPR, c = i2 - row * CPR;
                const int q = q0 + tw0 + row;
                if (q < Linb)
                    *(uint4*)((char*)((_Float16*)a.out + (size_t)b * a.out_bstride + ((size_t)q * a.u + r) * a.cout + ct0 * 32) + c * 16) =
                        *(const uint4*)(sc + row * TWP + c * 16);
            }
        }
    }
    if (a.out_tr) {  // (block-uniform) whole rows out of the LDS tile: 16 bytes per lane, consecutive lanes = consecutive chunks of a row
        __syncthreads();
        const int esz = a.out_half ? 2 : 4;
        const int pitch = a.cout * esz + 16, cpr = a.cout * esz / 16;  // bytes per tile row, 16-byte chunks per row
        const int nrows = min(TQ, Linb - q0) * a.u;                    // rows of this tile inside the item
        const char* ot = smem + a.out_tr_off;
        char* og = (char*)a.out + ((size_t)b * a.out_bstride + (size_t)q0 * a.u * a.cout) * esz;
        for (int i = threadIdx.x; i < nrows * cpr; i += 256) {
            const int row = i / cpr, c = i - row * cpr;
            *(uint4*)(og + ((size_t)row * cpr + c) * 16) = *(const uint4*)(ot + (size_t)row * pitch + c * 16);
        }
    }
}

}  // namespace rvcmi
