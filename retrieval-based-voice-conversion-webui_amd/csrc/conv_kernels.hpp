// Device code of the NSF-HiFi-GAN generator for gfx950 (CDNA4): the single-conv kernels -- the exact-fp32 VALU path, the
// generic MFMA conv (stage tile -> conv_core -> epilogue) and its K-split form.  Layout and GEMM view: mfma_conv.hpp.
//
// Reference semantics reproduced here (file:line in the reference):
//   conv_pre + cond        rvc/layers/nsf.py:164-166
//   ups / noise_convs      rvc/layers/nsf.py:169-174
#pragma once
#include <hip/hip_runtime.h>

#include "exact_fp.hpp"
#include "mfma_conv.hpp"

namespace rvcmi {

// ------------------------------------------------------------------------------------------------
// Exact-fp32 VALU kernels (RVCMI_OPERAND_F32): correctness-first reference-grade path on the GPU.
// ------------------------------------------------------------------------------------------------

enum InMode : int {
    IN_F32_ACT = 0,   // fp32 channels-last, apply v = lrelu(v / div, slope) on load
    IN_OP_RAW = 1,    // already-activated operand copy (OpT in MFMA mode, fp32 in F32 mode)
    IN_F32_CF = 2,    // fp32 channel-first [B][C][L] raw (conv_pre input, the reference layout)
    IN_HAR = 3        // the excitation viewed as frames: row t, channel c = har[t*hs - hpad + c] (c < hs), else 0
};
enum OutMode : int {
    OUT_ACT = 0,      // out = lrelu(acc + bias, slope_out) stored as operand type
    OUT_F32 = 1       // out (+)= acc + bias (+ res) (+ cb[b][co]) stored fp32
};

struct ConvArgs {
    // input
    const void* in;
    const float* in_b;  // optional 2nd / 3rd fp32 addends: v = ((in + in_b) + in_c) / div_in   (nsf.py:177-186)
    const float* in_c;
    long in_bstride;   // elements per batch item
    int Lin;           // valid input rows
    int cf_stride;     // IN_F32_CF: elements between channels (= the longest item's Lin)
    const int* lens;   // ragged batch (item_rows): Lin = lens[b] * lmul_in, Lq = lens[b] * lmul_q; nullptr = every item full length
    int lmul_in, lmul_q;
    int cin;
    int in_mode;
    int hs, hpad;      // IN_HAR: frame length (= noise-conv stride) and left padding; Lin counts SAMPLES of har
    float slope_in, div_in;
    // weights
    const void* w;     // F32: [taps][cin][cout] fp32.  MFMA: packed fragments (see pack_conv_weights)
    long w_ct_stride;  // MFMA: elements per 32-channel output tile
    const float* bias; // [cout] or nullptr
    int cout;
    // geometry: output position q, tap j reads input row  q + in_off + j*dstep
    int ntaps;         // real taps (F32) / padded taps (MFMA)
    int in_off, dstep;
    int roff;          // MFMA: LDS tile row of (q = q0, tap 0) ; tile starts at input row q0+in_off-roff
    int tile_rows;     // MFMA: rows staged in LDS
    int Lq;            // output positions
    // output
    int out_mode;
    void* out;
    long out_bstride;
    int out_C;         // channels per output row
    int out_mul, out_add;  // output row = q*out_mul + out_add  (polyphase transposed conv)
    float slope_out;
    const float* res;  // fp32 residual [B][Lq][out_C] or nullptr
    long res_bstride;
    int accumulate;    // out += ...
    const float* cb;   // per-(batch, channel) additive term [B][cout] or nullptr
    // polyphase (transposed conv): blockIdx.y selects the phase; per-phase geometry
    int nphase;
    int ph_in_off[16];
    int ph_ntaps[16];   // F32 only
    long ph_w_off[16];  // element offset into w
};

// One thread per (q, co); co fastest so that weight reads and stores coalesce.
static __global__ void __launch_bounds__(256) k_conv_f32(ConvArgs a) {
    const int b = blockIdx.z;
    const int Linb = item_rows(a.lens, b, a.lmul_in, a.Lin), Lqb = item_rows(a.lens, b, a.lmul_q, a.Lq);
    const int ph = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Lqb * a.cout) return;
    const int q = (int)(i / a.cout);
    const int co = (int)(i - (size_t)q * a.cout);
    const int in_off = a.nphase > 1 ? a.ph_in_off[ph] : a.in_off;
    const int ntaps = a.nphase > 1 ? a.ph_ntaps[ph] : a.ntaps;
    const float* W = (const float*)a.w + (a.nphase > 1 ? a.ph_w_off[ph] : 0);
    const float* in = (const float*)a.in + (size_t)b * a.in_bstride;
    float acc = a.bias ? a.bias[co] : 0.f;
    for (int j = 0; j < ntaps; ++j) {
        const int r = q + in_off + j * a.dstep;
        if (r < 0 || r >= Linb) continue;
        const float* wj = W + (size_t)j * a.cin * a.cout + co;
        if (a.in_mode == IN_F32_CF) {
            for (int ci = 0; ci < a.cin; ++ci) acc = fmaf(in[(size_t)ci * a.cf_stride + r], wj[(size_t)ci * a.cout], acc);
        } else if (a.in_mode == IN_F32_ACT) {
            const float* row = in + (size_t)r * a.cin;
            const float* rowb = a.in_b ? a.in_b + (size_t)b * a.in_bstride + (size_t)r * a.cin : nullptr;
            const float* rowc = a.in_c ? a.in_c + (size_t)b * a.in_bstride + (size_t)r * a.cin : nullptr;
            for (int ci = 0; ci < a.cin; ++ci) {
                float v = row[ci];
                if (rowb) v = v + rowb[ci];
                if (rowc) v = v + rowc[ci];
                if (a.div_in != 1.f) v = v / a.div_in;
                acc = fmaf(lrelu(v, a.slope_in), wj[(size_t)ci * a.cout], acc);
            }
        } else {
            const float* row = in + (size_t)r * a.cin;
            for (int ci = 0; ci < a.cin; ++ci) acc = fmaf(row[ci], wj[(size_t)ci * a.cout], acc);
        }
    }
    const size_t orow = (size_t)q * a.out_mul + (a.nphase > 1 ? ph : a.out_add);
    if (a.out_mode == OUT_ACT) {
        ((float*)a.out)[(size_t)b * a.out_bstride + orow * a.out_C + co] = lrelu(acc, a.slope_out);
    } else {
        if (a.cb) acc = acc + a.cb[(size_t)b * a.cout + co];
        if (a.res) acc = acc + a.res[(size_t)b * a.res_bstride + orow * a.out_C + co];
        float* o = (float*)a.out + (size_t)b * a.out_bstride + orow * a.out_C + co;
        *o = a.accumulate ? (*o + acc) : acc;
    }
}

// x[b][t][co] += bn[co] + sum_j har[b][t*s - pad + j] * Wn[j][co]      (nsf.py:173-174)
static __global__ void __launch_bounds__(256) k_noise_add(float* __restrict__ x, const float* __restrict__ har,
                                                   const float* __restrict__ Wn /*[k][C]*/, const float* __restrict__ bn,
                                                   int L, int C, int Lh, int k, int s, int pad, const int* __restrict__ lens, int lmul,
                                                   int lhmul) {
    const int b = blockIdx.z;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)item_rows(lens, b, lmul, L) * C) return;
    const int Lhb = item_rows(lens, b, lhmul, Lh);
    const int t = (int)(i / C);
    const int co = (int)(i - (size_t)t * C);
    const float* h = har + (size_t)b * Lh;
    float acc = bn[co];
    const int base = t * s - pad;
    for (int j = 0; j < k; ++j) {
        int r = base + j;
        if (r >= 0 && r < Lhb) acc = fmaf(h[r], Wn[(size_t)j * C + co], acc);
    }
    x[((size_t)b * L + t) * C + co] += acc;
}

// Stage `rows` input rows starting at global row g0 into the LDS tile (zero outside [0, Lin)).
template <typename OpT, int CIN>
__device__ __forceinline__ void stage_tile(char* smem, const ConvArgs& a, int b, int g0, int rows) {
    using frag = typename Op<OpT>::frag;
    constexpr int STRIDE = Tile<CIN>::STRIDE;
    constexpr int C8 = CIN / 8;
    const int tid = threadIdx.x;
    const int Linb = item_rows(a.lens, b, a.lmul_in, a.Lin);  // ragged batch: this item's input rows
    if (a.in_mode == IN_F32_CF) {
        // channel-first input (the caller's [B][C][T], nsf.py:164): consecutive lanes walk TIME so that every load
        // instruction is one contiguous run per channel; 8 channels x SBC chunks in flight per thread (the row-major
        // mapping below made this 8 uncoalesced serial loads per chunk: 49 us for conv_pre at T = 1198)
        constexpr int SBC = 4;
        const float* ip = (const float*)a.in + (size_t)b * a.in_bstride;
        const int total = rows * C8;
        for (int base = tid; base < total; base += SBC * 256) {
            float f[SBC][8];
#pragma unroll
            for (int u = 0; u < SBC; ++u) {
                const int idx = min(base + u * 256, total - 1);
                const int c8 = idx / rows, r = idx - c8 * rows;
                const int grc = min(max(g0 + r, 0), Linb - 1);
#pragma unroll
                for (int e = 0; e < 8; ++e) f[u][e] = ip[(size_t)(c8 * 8 + e) * a.cf_stride + grc];
            }
#pragma unroll
            for (int u = 0; u < SBC; ++u) {
                const int idx = base + u * 256;
                if (idx < total) {
                    const int c8 = idx / rows, r = idx - c8 * rows;
                    const int gr = g0 + r;
                    const bool ok = gr >= 0 && gr < Linb;
                    frag v;
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] = ok ? to_op<OpT>(f[u][e]) : (OpT)0.f;
                    *(frag*)(smem + (size_t)r * STRIDE + c8 * 16) = v;
                }
            }
        }
        return;
    }
    if (a.in_mode == IN_OP_RAW || (a.in_mode == IN_F32_ACT && !a.in_b && !a.in_c && a.div_in == 1.f)) {
        // plain row-major inputs (the conv-by-conv resblock path): SB chunks in flight per thread, clamped addresses so that every
        // load is unconditional (the one-chunk-at-a-time loop below is a load -> convert -> store round trip per chunk: 22 serial
        // L2 latencies for a 176-row tile at C = 256, the whole duration of a small launch)
        constexpr int SB = 8;
        const int total = rows * C8;
        const bool raw = a.in_mode == IN_OP_RAW;
        for (int base = tid; base < total; base += SB * 256) {
            frag vr[SB];
            float4 lo[SB], hi[SB];
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int idx = min(base + u * 256, total - 1);
                const int r = idx / C8, c8 = idx - r * C8;
                const int grc = min(max(g0 + r, 0), Linb - 1);
                if (raw) {
                    vr[u] = *(const frag*)((const OpT*)a.in + (size_t)b * a.in_bstride + (size_t)grc * CIN + c8 * 8);
                } else {
                    const float4* p = (const float4*)((const float*)a.in + (size_t)b * a.in_bstride + (size_t)grc * CIN + c8 * 8);
                    lo[u] = p[0];
                    hi[u] = p[1];
                }
            }
#pragma unroll
            for (int u = 0; u < SB; ++u) {
                const int idx = base + u * 256;
                if (idx < total) {
                    const int r = idx / C8, c8 = idx - r * C8;
                    const int gr = g0 + r;
                    const bool ok = gr >= 0 && gr < Linb;
                    frag v;
                    if (raw) {
                        v = vr[u];
                    } else {
                        const float f[8] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z, hi[u].w};
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = to_op<OpT>(lrelu(f[e], a.slope_in));
                    }
                    if (!ok) {
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = (OpT)0.f;
                    }
                    *(frag*)(smem + (size_t)r * STRIDE + c8 * 16) = v;
                }
            }
        }
        return;
    }
    for (int idx = tid; idx < rows * C8; idx += 256) {
        const int r = idx / C8;
        const int c8 = idx - r * C8;
        const int gr = g0 + r;
        frag v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (OpT)0.f;
        if (a.in_mode == IN_HAR) {
            // noise_convs[i] (nsf.py:103-115) is Conv1d(1, C, k=2s, stride s, pad s/2): over frames of s samples it is
            // a plain 2-tap conv with C_in = s, so it runs on the MFMA path.  s % 8 == 0 keeps every 8-sample
            // chunk entirely inside or outside the signal and 16-byte aligned.
            // (hs % 8 == 0, hpad = hs/2 and Lin % 4 == 0 make every 4-sample half either fully inside or fully
            // outside the signal; an 8-sample chunk may straddle its start/end, so validity is per half.)
            const long base = (long)gr * a.hs - a.hpad + c8 * 8;
            if (c8 * 8 < a.hs) {
                const float* hp = (const float*)a.in + (size_t)b * a.in_bstride;
                const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 lo = (base >= 0 && base + 4 <= Linb) ? *(const float4*)(hp + base) : z4;
                const float4 hi = (base + 4 >= 0 && base + 8 <= Linb) ? *(const float4*)(hp + base + 4) : z4;
                const float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = to_op<OpT>(f[e]);
            }
        } else if (gr >= 0 && gr < Linb) {
            if (a.in_mode == IN_OP_RAW) {
                v = *(const frag*)((const OpT*)a.in + (size_t)b * a.in_bstride + (size_t)gr * CIN + c8 * 8);
            } else if (a.in_mode == IN_F32_ACT) {
                const float4* p = (const float4*)((const float*)a.in + (size_t)b * a.in_bstride + (size_t)gr * CIN + c8 * 8);
                float4 lo = p[0], hi = p[1];
                float f[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
                if (a.in_b) {
                    const float4* pb = (const float4*)(a.in_b + (size_t)b * a.in_bstride + (size_t)gr * CIN + c8 * 8);
                    float4 l2 = pb[0], h2 = pb[1];
                    f[0] += l2.x; f[1] += l2.y; f[2] += l2.z; f[3] += l2.w; f[4] += h2.x; f[5] += h2.y; f[6] += h2.z; f[7] += h2.w;
                }
                if (a.in_c) {
                    const float4* pc = (const float4*)(a.in_c + (size_t)b * a.in_bstride + (size_t)gr * CIN + c8 * 8);
                    float4 l2 = pc[0], h2 = pc[1];
                    f[0] += l2.x; f[1] += l2.y; f[2] += l2.z; f[3] += l2.w; f[4] += h2.x; f[5] += h2.y; f[6] += h2.z; f[7] += h2.w;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float x = f[e];
                    if (a.div_in == 3.f) x = div3_exact(x);
                    else if (a.div_in != 1.f) x = x / a.div_in;
                    v[e] = to_op<OpT>(lrelu(x, a.slope_in));
                }
            } else {  // IN_F32_CF
                const float* p = (const float*)a.in + (size_t)b * a.in_bstride + (size_t)(c8 * 8) * a.cf_stride + gr;
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = to_op<OpT>(p[(size_t)e * a.cf_stride]);
            }
        }
        *(frag*)(smem + (size_t)r * STRIDE + c8 * 16) = v;
    }
}

// Generic single-conv kernel: stage tile -> conv_core -> epilogue.  Grid: x = time tile,
// y = (co block) * nphase + phase, z = batch.  Block = 4 waves laid out WCO (co) x WT (time).
template <typename OpT, int CIN, int MI, int NJ, int WCO, int NB = 2, bool PFW = false>
__device__ __forceinline__ void conv_mfma_body(const ConvArgs& a, int b, char* smem) {
    using TL = Tile<CIN>;
    constexpr int WT = 4 / WCO;
    constexpr int TT = WT * NJ * 32;
    const int ph = a.nphase > 1 ? (int)(blockIdx.y % a.nphase) : 0;
    const int cob = a.nphase > 1 ? (int)(blockIdx.y / a.nphase) : (int)blockIdx.y;
    const int q0 = blockIdx.x * TT;
    const int in_off = a.nphase > 1 ? a.ph_in_off[ph] : a.in_off;
    const OpT* wbase = (const OpT*)a.w + (a.nphase > 1 ? a.ph_w_off[ph] : 0);

    unsigned pf_acc = 0;
    if constexpr (PFW) {
        // Tiny launches (a realtime chunk) use every weight byte for a handful of row tiles only, so the weights are never
        // L2-resident: the K loop's 12 KB of loads in flight per wave then runs at the latency of the far memory side (measured:
        // 24 us per launch for a 6 us K loop).  Touch the block's whole weight slice up front -- every thread 16 bytes per 4 KB
        // round, all rounds in flight next to the tile staging -- so that the K loop finds it in the XCD's L2.
        const char* wb = (const char*)(wbase + (size_t)cob * WCO * MI * a.w_ct_stride);
        const size_t bytes = (size_t)WCO * MI * a.w_ct_stride * sizeof(OpT);
        const size_t rounds = bytes / 4096;
#pragma unroll 8
        for (size_t r = 0; r < rounds; ++r) {
            const uint4 v = *(const uint4*)(wb + r * 4096 + threadIdx.x * 16);
            pf_acc ^= v.x ^ v.y ^ v.z ^ v.w;
        }
    }
    stage_tile<OpT, CIN>(smem, a, b, q0 + in_off - a.roff, a.tile_rows);
    if constexpr (PFW) {
        if (pf_acc == 0x9e3779b9u && a.Lq < 0) *(unsigned*)smem = pf_acc;  // never true: keeps the prefetch loads alive
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int wco = wave % WCO;
    const int wt = wave / WCO;
    const int ct0 = (cob * WCO + wco) * MI;  // first 32-channel output tile of this wave
    const int tw0 = wt * NJ * 32;            // first time row of this wave inside the block tile

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][jt][r] = 0.f;

    const char* lds_lane = smem + (size_t)(tw0 + (lane & 31)) * TL::STRIDE + (lane >> 5) * 16;
    const OpT* wlane = wbase + (size_t)ct0 * a.w_ct_stride + lane * 8;
    conv_core<OpT, CIN, MI, NJ, KGROUP, NB>(acc, lds_lane, wlane, a.w_ct_stride, a.ntaps, a.roff, a.dstep);

    // ---- epilogue -------------------------------------------------------------------------
    const int out_add = a.nphase > 1 ? ph : a.out_add;
    // bias (+ the per-utterance cond vector) of this lane's channels: fetched ONCE, as one batch, before the store loops
    // (a conditional load inside them becomes a branch with its own wait: 64 serialised L2 round trips = ~30 us on conv_pre)
    f32x4 bvec[MI][4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int g = 0; g < 4; ++g) bvec[mi][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (a.bias) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int g = 0; g < 4; ++g) bvec[mi][g] = *(const f32x4*)(a.bias + min((ct0 + mi) * 32 + 4 * (lane >> 5) + 8 * g, a.cout - 4));
    }
    if (a.cb) {  // (also with OUT_ACT: conv_pre writes lrelu(conv + bias + cond) as operands, round 6)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                bvec[mi][g] += *(const f32x4*)(a.cb + (size_t)b * a.cout + min((ct0 + mi) * 32 + 4 * (lane >> 5) + 8 * g, a.cout - 4));
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int cobase = (ct0 + mi) * 32 + 4 * (lane >> 5);
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) {
            const int q = q0 + tw0 + jt * 32 + (lane & 31);
            if (q >= item_rows(a.lens, b, a.lmul_q, a.Lq)) continue;
            const size_t orow = (size_t)q * a.out_mul + out_add;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = cobase + 8 * g;
                if (co >= a.cout) continue;  // cout is a multiple of 4 whenever it is < the padded tile
                f32x4 v = {acc[mi][jt][4 * g + 0], acc[mi][jt][4 * g + 1], acc[mi][jt][4 * g + 2], acc[mi][jt][4 * g + 3]};
                v += bvec[mi][g];
                if (a.out_mode == OUT_ACT) {
                    using o4 = __attribute__((ext_vector_type(4))) OpT;
                    o4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = to_op<OpT>(lrelu(v[e], a.slope_out));
                    *(o4*)((OpT*)a.out + (size_t)b * a.out_bstride + orow * a.out_C + co) = o;
                } else {
                    if (a.res) v += *(const f32x4*)(a.res + (size_t)b * a.res_bstride + orow * a.out_C + co);
                    f32x4* o = (f32x4*)((float*)a.out + (size_t)b * a.out_bstride + orow * a.out_C + co);
                    if (a.accumulate) v += *o;
                    *o = v;
                }
            }
        }
    }
}

template <typename OpT, int CIN, int MI, int NJ, int WCO>
static __global__ void __launch_bounds__(256) k_conv_mfma(ConvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    conv_mfma_body<OpT, CIN, MI, NJ, WCO>(a, (int)blockIdx.z, smem);
}

// Up to three independent convs of one shape in ONE launch (grid.z = batch x jobs).  Used where a fused resblock launch would
// be a handful of blocks (the realtime chunk: 310 rows at C = 256 = 9 pair tiles, each streaming 2.9 MB of weights through one
// CU): conv1 / conv2 of all the stage's resblocks as separate, output-channel-split launches (k_conv_ks_jobs).
struct ConvJobs {
    ConvArgs job[3];
    int njobs;
};
// K-SPLIT form of the same conv (round 5).  In the conv-by-conv path of a realtime chunk (310 rows at C = 256, 3100 at C = 128) a wave's K
// loop is one MFMA per k-step behind a weight fragment from L2: 176 k-steps at k = 11 run at the LATENCY of that stream whatever the ring
// depth (19-22 us per launch for ~6 us of work), and three row tiles x eight channel tiles x three jobs are 72 blocks on 256 CUs.  Here the
// block's four waves split the TAPS of ONE 32-row x 32 MI-channel output tile (44 k-steps each at k = 11), the partial sums meet in LDS and
// wave 0 adds them in a fixed order ((w0 + w1) + w2) + w3 and runs the epilogue: a quarter of the dependent weight round trips per wave, no
// weight byte fetched twice, and row tiles x channel tiles x jobs = 240 blocks.  Grid: x = 32-row tile, y = channel tile, z = batch x jobs.
// NJ = row tiles per block.  Measured (realtime chunk, ABAB): C = 256, NJ = 1: six launches 134 -> 107 us; C = 128 (3100 rows): NJ = 1 114 -> 155 us
// (1164 blocks that each stage 82 rows for 32 outputs), NJ = 3 (396 blocks) 113 -> 107 us.
template <typename OpT, int CIN, int MI, int NJ>
__device__ __forceinline__ void conv_ks_body(const ConvArgs& a, int b, char* smem) {
    using TL = Tile<CIN>;
    constexpr int CC = TL::CC;
    constexpr int TT = 32 * NJ;  // rows per block
    static_assert(CC >= KGROUP, "K split by taps: a tap must be whole k-groups");
    const int cob = (int)blockIdx.y;
    const int q0 = blockIdx.x * TT;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ct0 = cob * MI;
    const OpT* wbase = (const OpT*)a.w;
    // this wave's taps [t0, t1) (k = 3: one tap each for three waves, the fourth adds zeros)
    const int per = (a.ntaps + 3) / 4;
    const int t0 = min(wave * per, a.ntaps), t1 = min(t0 + per, a.ntaps);
    unsigned pf_acc = 0;
    {   // touch this wave's weight slice up front (see conv_mfma_body PFW): the K loop then finds it in the XCD's L2
        const char* wb = (const char*)(wbase + (size_t)ct0 * a.w_ct_stride + (size_t)t0 * CC * 512);
        for (int r = 0; r < (t1 - t0) * CC; ++r)
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                const uint4 v = *(const uint4*)(wb + ((size_t)mi * a.w_ct_stride + (size_t)r * 512) * sizeof(OpT) + lane * 16);
                pf_acc ^= v.x ^ v.y ^ v.z ^ v.w;
            }
    }
    // epilogue operands of wave 0, requested before the staging (their round trip runs under it)
    const int cobase = ct0 * 32 + 4 * (lane >> 5);
    const int Lqb = item_rows(a.lens, b, a.lmul_q, a.Lq);
    f32x4 bvec[MI][4], rvec[MI][NJ][4];
    if (wave == 0) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = min(cobase + mi * 32 + 8 * g, a.cout - 4);
                bvec[mi][g] = a.bias ? *(const f32x4*)(a.bias + co) : f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.cb) bvec[mi][g] += *(const f32x4*)(a.cb + (size_t)b * a.cout + co);
#pragma unroll
                for (int jt = 0; jt < NJ; ++jt) {
                    const size_t orow = (size_t)min(q0 + jt * 32 + (lane & 31), Lqb - 1) * a.out_mul + a.out_add;
                    rvec[mi][jt][g] = (a.res && a.out_mode != OUT_ACT) ? *(const f32x4*)(a.res + (size_t)b * a.res_bstride + orow * a.out_C + co)
                                                                      : f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
    }
    stage_tile<OpT, CIN>(smem, a, b, q0 + a.in_off - a.roff, a.tile_rows);
    if (pf_acc == 0x9e3779b9u && a.Lq < 0) *(unsigned*)smem = pf_acc;  // never true: keeps the prefetch loads alive
    __syncthreads();

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][jt][r] = 0.f;
    const char* lds_lane = smem + (size_t)(lane & 31) * TL::STRIDE + (lane >> 5) * 16;
    if (t1 > t0)  // (wave-uniform)
        conv_core<OpT, CIN, MI, NJ, KGROUP, 4>(acc, lds_lane, wbase + (size_t)ct0 * a.w_ct_stride + (size_t)t0 * CC * 512 + lane * 8, a.w_ct_stride,
                                               t1 - t0, a.roff + t0 * a.dstep, a.dstep);
    // partial sums of waves 1..3 -> LDS behind the operand tile ([3][MI][NJ][16][64] floats)
    float* red = (float*)(smem + (size_t)a.tile_rows * TL::STRIDE);
    if (wave > 0) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
                for (int r = 0; r < 16; ++r) red[((((wave - 1) * MI + mi) * NJ + jt) * 16 + r) * 64 + lane] = acc[mi][jt][r];
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll
    for (int jt = 0; jt < NJ; ++jt) {
        const int q = q0 + jt * 32 + (lane & 31);
        if (q >= Lqb) continue;
        const size_t orow = (size_t)q * a.out_mul + a.out_add;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co = cobase + mi * 32 + 8 * g;
                if (co >= a.cout) continue;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = 4 * g + e;
                    v[e] = ((acc[mi][jt][r] + red[(((0 * MI + mi) * NJ + jt) * 16 + r) * 64 + lane]) + red[(((1 * MI + mi) * NJ + jt) * 16 + r) * 64 + lane]) +
                           red[(((2 * MI + mi) * NJ + jt) * 16 + r) * 64 + lane];
                }
                v += bvec[mi][g];
                if (a.out_mode == OUT_ACT) {
                    using o4 = __attribute__((ext_vector_type(4))) OpT;
                    o4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = to_op<OpT>(lrelu(v[e], a.slope_out));
                    *(o4*)((OpT*)a.out + (size_t)b * a.out_bstride + orow * a.out_C + co) = o;
                } else {
                    if (a.res) v += rvec[mi][jt][g];
                    f32x4* o = (f32x4*)((float*)a.out + (size_t)b * a.out_bstride + orow * a.out_C + co);
                    if (a.accumulate) v += *o;
                    *o = v;
                }
            }
    }
}
template <typename OpT, int CIN, int MI, int NJ>
static __global__ void __launch_bounds__(256) k_conv_ks_jobs(ConvJobs js) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int j = (int)blockIdx.z % js.njobs, b = (int)blockIdx.z / js.njobs;
    conv_ks_body<OpT, CIN, MI, NJ>(js.job[j], b, smem);
}

}  // namespace rvcmi
