// The MFMA convolution machinery shared by the generator, the streaming ResBlock and the front for gfx950 (CDNA4):
// operand types, the LDS tile geometry, the K loops (conv_run, kconv, kconv16) and the publish helpers.
//
// Internal activation layout is CHANNELS-LAST  [B][L][C]  (fp32 residual stream; the activated
// MFMA operand copies are OpT = bf16 / fp16).  With channels last, one MFMA B-fragment of a k-tap
// dilated convolution is "8 consecutive input channels of ONE time row": a single 16-byte LDS
// read, and moving to the next tap is a constant row offset -- no im2col is ever materialised.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace rvcmi {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

__device__ __forceinline__ float lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// Ragged batches (rvcmi_nsf_forward `lengths`): item b of a batch holds lens[b] <= T valid frames and is computed EXACTLY as a
// separate call of that length would compute it -- every layer zero-pads its input beyond the item's own last row (the padded
// batch of the reference lets the rows behind a short item leak into its tail through every receptive field).  Each kernel
// replaces its row count by the item's: rows(lens, b, mul, Lmax) = lens[b] * mul (mul = the stage's upsampling factor so far);
// buffer strides stay those of the longest item.
// (clamped on BOTH sides: a device-resident lengths tensor is not validated on the host -- no sync -- and lens[b] <= 0 would make the
//  clamped staging loads `min(max(row, 0), rows - 1)` read row -1 of the stream, out of bounds for item 0)
__device__ __forceinline__ int item_rows(const int* __restrict__ lens, int b, int mul, int Lmax) {
    return lens ? max(min(Lmax, lens[b] * mul), min(Lmax, mul)) : Lmax;
}

// ------------------------------------------------------------------------------------------------
// MFMA convolution (RVCMI_OPERAND_BF16 / _F16)
// ------------------------------------------------------------------------------------------------
//
// GEMM view of a k-tap conv: D[co][t] = sum_{tap,ci} W[co][tap,ci] * X[t + off(tap)][ci]
//   M = output channels, N = time, K = taps*C_in, instruction v_mfma_f32_32x32x16_{bf16,f16}.
//   A (weights)      lane l holds W[co = l&31][k = 8*(l>>5) .. +8]  -> pre-packed in that exact
//                    order on the host, streamed global->VGPR (each wave owns its own co slice,
//                    so LDS staging would buy nothing), double-buffered one k-group ahead.
//   B (activations)  lane l holds X[t = l&31][ci = 8*(l>>5) .. +8]  -> ONE ds_read_b128 from the
//                    channels-last LDS tile; rows padded by 16 B so the 16 lanes of a read group
//                    hit 16 distinct 16-byte bank slots.
//   D                lane l holds t = l&31, co = (r&3) + 8*(r>>2) + 4*(l>>5)  -> 4 consecutive
//                    channels per register quad = one float4 (or 8-byte OpT) store per quad.
// The activation tile is staged ONCE per block and reused by every tap and every output channel,
// so the K loop has no barrier at all.

template <typename OpT>
struct Op;
template <>
struct Op<__bf16> {
    using frag = bf16x8;
    static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 mfma16(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
template <>
struct Op<_Float16> {
    using frag = f16x8;
    static __device__ __forceinline__ f32x16 mfma(frag a, frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ f32x4 mfma16(frag a, frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};

constexpr int KGROUP = 4;  // k-steps (of 16) per software-pipeline group (also the weight-packing pad unit)

// float -> operand, round-to-nearest-even; fp16 saturates instead of overflowing to inf.
template <typename OpT>
__device__ __forceinline__ OpT to_op(float v) {
    return (OpT)v;
}
template <>
__device__ __forceinline__ _Float16 to_op<_Float16>(float v) {
    return (_Float16)__builtin_amdgcn_fmed3f(v, -65504.f, 65504.f);  // one v_med3_f32 instead of max + min
}

template <int CIN>
struct Tile {
    static constexpr int CC = CIN / 16;              // k-steps per tap
    static constexpr int STRIDE = CIN * 2 + 16;      // bytes per LDS row (16-B pad: conflict-free b128 reads)
    static constexpr int TAPS_PER_GROUP = (CC >= KGROUP) ? 1 : KGROUP / CC;
    static_assert(CIN % 16 == 0, "C_in must be a multiple of 16");
    static_assert((CC >= KGROUP) ? (CC % KGROUP == 0) : (KGROUP % CC == 0), "k-group must tile a tap");
};

// The K loop.  acc[mi][jt] += sum over (padded) taps and channel chunks.
//   lds_lane : smem + (wave_t0 + (lane&31)) * STRIDE + (lane>>5)*16
//   wlane    : packed weights of this wave's first co tile + lane*8
// The K loop is split in two so that a kernel can put a barrier / epilogue BETWEEN "weights requested" and
// "weights used":
//   conv_prefetch  issues the global loads of the first NB-1 weight groups (KGROUP k-steps each) into registers;
//   conv_run       multiplies group g while group g+NB-1 is in flight.  (An explicit one-k-step-ahead double buffer
//                  of the B fragments was tried and measured SLOWER -- 11.2k -> 13.3k cycles per k=7 conv at C=64 --
//                  than leaving the ds_read placement to the compiler.)
template <typename OpT, int MI, int KGROUP, int NB>
__device__ __forceinline__ void conv_load_group(typename Op<OpT>::frag (&Ab)[KGROUP][MI], const OpT* wlane, long ct_stride, int grp) {
    using frag = typename Op<OpT>::frag;
#pragma unroll
    for (int g = 0; g < KGROUP; ++g)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
            Ab[g][mi] = *(const frag*)(wlane + (size_t)mi * ct_stride + (size_t)(grp * KGROUP + g) * 512);
}

template <typename OpT, int CIN, int MI, int KGROUP, int NB>
__device__ __forceinline__ void conv_prefetch(typename Op<OpT>::frag (&A)[NB][KGROUP][MI], const OpT* wlane, long ct_stride,
                                              int ntaps_p) {
    const int NG = ntaps_p * Tile<CIN>::CC / KGROUP;
#pragma unroll
    for (int i = 0; i < NB - 1; ++i)
        if (i < NG) conv_load_group<OpT, MI, KGROUP, NB>(A[i], wlane, ct_stride, i);
}

// One wave per SIMD issues in order, so every non-MFMA instruction must sit in the 32-cycle shadow of an MFMA:
//   * B addresses are a running per-group base + compile-time immediates (no per-k-step scalar math),
//   * every load is unconditional (clamped indices instead of branches, so a whole k-group is one scheduling region),
//   * the ds_reads of the NEXT k-step and the global weight loads of group g+NB-1 are spread one per MFMA and the
//     order is pinned with sched_group_barrier (MFMA, DS_READ, MFMA, DS_READ, ..., MFMA, VMEM, ...).
// Measured in tools/ubench/kloop.hip (C=64, k=7): 58.5 -> see DESIGN.md cycles per MFMA.
// REAL (only where a k-group holds several taps, C_in < 16 * KGROUP): the packed tap count is rounded up to a whole k-group, so the
// last group ends in taps of zero weights.  `nks` = k-steps that carry real taps (taps * CC); the wave leaves the last group at the
// first tap boundary at or behind it (wave-uniform), skipping the MFMAs, the B reads and the ring requests of the dead slots.
// nks >= ntaps_p * CC runs the padded loop.
// JT0: first column tile that is computed (as in kconv, below): tiles 0 .. JT0-1 keep what acc held on entry.
template <typename OpT, int CIN, int MI, int NJ, int KGROUP, int NB, bool REAL = false, int JT0 = 0>
__device__ __forceinline__ void conv_run(f32x16 (&acc)[MI][NJ], typename Op<OpT>::frag (&A)[NB][KGROUP][MI],
                                         const char* lds_lane, const OpT* wlane, long ct_stride, int ntaps_p, int roff,
                                         int dstep, int nks = 0) {
    using frag = typename Op<OpT>::frag;
    using TL = Tile<CIN>;
    constexpr int CC = TL::CC;
    constexpr int STRIDE = TL::STRIDE;
    static_assert((CC >= KGROUP) ? (CC % KGROUP == 0) : (KGROUP % CC == 0), "k-group must tile a tap");
    static_assert(NB >= 2 && NB <= 4, "2..4 weight buffers");
    static_assert(KGROUP % 2 == 0, "the B ping-pong needs an even k-group");
    static_assert(JT0 >= 0 && JT0 < NJ, "at least one column tile runs");
    constexpr int NJA = NJ - JT0;  // column tiles that run
    constexpr int GPT = (CC >= KGROUP) ? CC / KGROUP : 1;  // k-groups per tap
    constexpr int TPG = (CC >= KGROUP) ? 1 : KGROUP / CC;  // taps per k-group
    const int NG = ntaps_p * CC / KGROUP;
    const int dS = dstep * STRIDE;

    // byte offset of k-step k of a group relative to the group base
    auto koff = [&](int k) { return (CC >= KGROUP) ? k * 32 : (k / CC) * dS + (k % CC) * 32; };

    const char* gb = lds_lane + roff * STRIDE;  // B base of the current group
    int gi = 0;                                 // group index inside the current tap (CC >= KGROUP only)
    const OpT* an = wlane + (size_t)min(NB - 1, NG - 1) * KGROUP * 512;  // weights of the group to request next
    int gn = min(NB - 1, NG - 1);

    frag Bf[2][NJ];
    // first k-step's B fragments, in ASCENDING tile order like every later k-step (the waitcnt pass merges the loop entry
    // with the back edge: a different order here makes it wait for lgkmcnt(0) at the head of every group)
#pragma unroll
    for (int jt = JT0; jt < NJ; ++jt) {
        Bf[0][jt] = *(const frag*)(gb + koff(0) + jt * 32 * STRIDE);
        __builtin_amdgcn_sched_barrier(0);
    }
    for (int grp = 0; grp < NG; grp += NB) {
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int g = grp + u;
            if (g < NG) {
                const char* gbn;
                if constexpr (CC >= KGROUP) gbn = (gi + 1 == GPT) ? gb - (GPT - 1) * KGROUP * 32 + dS : gb + KGROUP * 32;
                else gbn = gb + TPG * dS;
                // Slot i of a k-step = MFMA i, then (i < NJ) the ds_read of the NEXT k-step's B fragment of time tile i, then
                // (last MI slots) one weight load of group g+NB-1.  The order is pinned with sched_barrier: left to the
                // scheduler, the reads that cross a group boundary came out in DESCENDING tile order, so the first MFMA of
                // every group waited for the LAST read issued (s_waitcnt lgkmcnt(0): a full LDS round trip, ~120 cycles per
                // 24 MFMAs = the 37 instead of 32 cycles per MFMA measured in round 2).
#pragma unroll
                for (int k = 0; k < KGROUP; ++k) {
                    if constexpr (REAL && TPG > 1)
                        if (k > 0 && k % CC == 0 && g * KGROUP + k >= nks) goto done;  // only zero taps are left
                    const char* nbp = (k + 1 < KGROUP) ? gb + koff(k + 1) : gbn + koff(0);
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                        for (int jt = JT0; jt < NJ; ++jt) {
                            constexpr int NS = MI * NJA;
                            const int i = mi * NJA + jt - JT0;
                            acc[mi][jt] = Op<OpT>::mfma(A[u][k][mi], Bf[k & 1][jt], acc[mi][jt]);
                            if (i < NJA) Bf[(k + 1) & 1][JT0 + i] = *(const frag*)(nbp + (JT0 + i) * 32 * STRIDE);
                            if (i >= NS - MI)
                                A[(u + NB - 1) % NB][k][i - (NS - MI)] = *(const frag*)(an + (size_t)(i - (NS - MI)) * ct_stride + k * 512);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                }
                gb = gbn;
                if constexpr (CC >= KGROUP) gi = (gi + 1 == GPT) ? 0 : gi + 1;
                if (gn < NG - 1) {
                    ++gn;
                    an += KGROUP * 512;
                }
            }
        }
    }
done:;
}

// ---- the lean K loop (round 3) ---------------------------------------------------------------------------------------
// conv_run's ring of NB groups of KGROUP k-steps pays a scalar/vector bookkeeping tail per group (one MFMA gap of ~9 and a tail
// of ~14 instructions per 24 MFMAs): 37.0 cycles per MFMA for a lone wave against 34.0 for the same traffic without it
// (tools/ubench/kloop2.hip).  kconv keeps that structure out of the loop:
//   * weights are RAW BUFFER loads: SGPR resource + SGPR running offset + one lane offset VGPR + immediate -- no 64-bit per-lane
//     address arithmetic at all;
//   * the weight ring is 8 k-steps deep and refilled IN PLACE: A[kk] is re-requested for the k-step 8 later right after its last
//     MFMA (twice the look-ahead of NB = 2 x KGROUP = 4 in the same registers), so the loop has no group structure;
//   * B fragments come from the channels-last LDS tile through one base VGPR per 8 k-steps and immediate offsets.
// For C_in a multiple of 128 (8 k-steps = a whole or half tap).  lds_row: LDS byte address of this lane's row at tap 0 (+ 16 for
// the upper half-wave), rsrc / loff: this wave's first output-channel tile and lane * 16, ctb: bytes per output-channel tile.
using lds_cptr_t = const __attribute__((address_space(3))) char*;
__device__ __forceinline__ unsigned lds_address(const void* p) { return (unsigned)(size_t)(lds_cptr_t)p; }
using u32x4_t = __attribute__((ext_vector_type(4))) unsigned;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t weight_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7fffffff, 0x00020000);
}
template <typename OpT>
__device__ __forceinline__ typename Op<OpT>::frag weight_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(typename Op<OpT>::frag, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
template <typename OpT, int MI>
__device__ __forceinline__ void kconv_prefetch(typename Op<OpT>::frag (&A)[8][MI], __amdgpu_buffer_rsrc_t r, unsigned loff, unsigned ctb) {
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) A[kk][mi] = weight_load<OpT>(r, loff + kk * 1024, mi * ctb);
}
// JT0: first column tile that is computed.  Tiles 0 .. JT0-1 keep what acc held on entry: no MFMA, no B read (k_rb_stream's first step of
// a strip, whose leading tiles are pipeline fill).  The weight requests stay one per k-step, now behind (NJ - JT0) * MI MFMAs.
template <typename OpT, int CIN, int MI, int NJ, int STRIDE, int JT0 = 0>
__device__ __forceinline__ void kconv(f32x16 (&acc)[MI][NJ], typename Op<OpT>::frag (&A)[8][MI], unsigned lds_row, __amdgpu_buffer_rsrc_t r,
                                      unsigned loff, unsigned ctb, int ntaps, int dstep) {
    using frag = typename Op<OpT>::frag;
    constexpr int CC = CIN / 16, GPT = CC / 8;  // k-steps per tap, groups of 8 k-steps per tap
    static_assert(CIN % 128 == 0, "kconv: C_in must be a multiple of 128");
    static_assert(JT0 >= 0 && JT0 < NJ, "kconv: at least one column tile runs");
    constexpr int NJA = NJ - JT0;  // column tiles that run
    constexpr unsigned TS = 32u * STRIDE;
    auto ld = [](unsigned a) { return *(const __attribute__((address_space(3))) frag*)(size_t)a; };
    frag Bf[2][NJ];
#pragma unroll
    for (int jt = JT0; jt < NJ; ++jt) {
        Bf[0][jt] = ld(lds_row + jt * TS);
        __builtin_amdgcn_sched_barrier(0);
    }
    const unsigned dS = (unsigned)(dstep * STRIDE);
    const int ngroups = ntaps * GPT;
    const unsigned slast = (unsigned)(ngroups - 1) * 8192u;
    unsigned soff = ngroups > 1 ? 8192u : 0u;  // byte offset of the group being requested (clamped: the last one re-requests itself)
    int gi = 0;                                // group inside the tap
    for (int g = 0; g < ngroups; ++g) {
        const unsigned nrow = (gi + 1 == GPT) ? lds_row - (unsigned)((GPT - 1) * 256) + dS : lds_row + 256u;  // next group's first k-step
        // (opaque copies: loop strength reduction otherwise rebases every read on the POST-increment pointer with negative
        //  offsets, which do not fit the ds_read offset field -- one v_add per MFMA)
        unsigned b0 = lds_row, b1 = nrow;
        asm volatile("" : "+v"(b0), "+v"(b1));
#pragma unroll
        for (int kk = 0; kk < 8; ++kk) {
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int jt = JT0; jt < NJ; ++jt) {
                    constexpr int NS = MI * NJA;
                    const int i = mi * NJA + jt - JT0;
                    acc[mi][jt] = Op<OpT>::mfma(A[kk][mi], Bf[kk & 1][jt], acc[mi][jt]);
                    if (i < NJA) Bf[(kk + 1) & 1][JT0 + i] = ld((kk < 7 ? b0 + (unsigned)((kk + 1) * 32) : b1) + (JT0 + i) * TS);
                    if (i >= NS - MI) A[kk][i - (NS - MI)] = weight_load<OpT>(r, loff + kk * 1024, soff + (unsigned)(i - (NS - MI)) * ctb);
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
        lds_row = nrow;
        gi = (gi + 1 == GPT) ? 0 : gi + 1;
        soff = soff < slast ? soff + 8192u : soff;
    }
}

// ---- the lean K loop on v_mfma_f32_16x16x32 (k_rb_stream, option RS_MFMA) ------------------------------------------------------
// The same sum over the same LDS tile and the same packed weights [co_tile][k_step][lane][8] in steps of 32 k; the chip holds a
// higher clock on this shape (tools/ubench/kloop2.hip `shape`).  A wave's 32 channels x 32 NJ rows are 2 channel
// halves x 2 NJ column tiles of 16 rows; per 32 k a tile's B fragment is ONE ds_read_b128 and feeds both halves' MFMAs.
//   B  lane l = (q, n) = (l / 16, l % 16) reads row mfma16_row(n) of the tile and the 8 channels of 16-byte chunk
//      mfma16_chunk(q) of the 32: which 8 channels sit in which K-block of the instruction is free as long as A agrees, and
//      the tile's rows may stand in any column order that the D lanes then follow.  Chunks {0, 2, 1, 3} and even rows on columns
//      0-3, 12-15, odd rows on 4-11 give every ds_read_b128 lane group ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, + 32) 16
//      distinct 16-byte slots with rows of 17 slots; the natural order puts two lanes of each group on one slot
//      (tools/model_rb_stream.py mfma16_*, tests/test_cpu_rb_stream_mfma16.py).
//   A  half h, K-block q = channels 16 h + n of k-step 2 s + (q & 1), 8-k block q >> 1: lanes 32 (q >> 1) + 16 h + n of that
//      k-step's packed fragment, whole 256-byte runs (mfma16_loff + s * 2048 + h * 256).  Ring slot A[2 s + h].
//   D  lane (q, n) holds row mfma16_row(n) and channels 16 h + 4 q + e: four consecutive channels of one row, as before.
// B fragments are refilled IN PLACE behind their second MFMA (the next use is 2 * (2 NJ - JT0) - 2 MFMAs later), so the buffer
// stays at 2 NJ fragments.  JT0 counts 16-row tiles.
__host__ __device__ constexpr int mfma16_row(int n) { return n < 4 ? 2 * n : n < 12 ? 2 * n - 7 : 2 * n - 16; }
__host__ __device__ constexpr int mfma16_chunk(int q) { return ((q & 1) << 1) | (q >> 1); }
__device__ __forceinline__ unsigned mfma16_loff(int lane) {
    const int q = lane >> 4, n = lane & 15;
    return (unsigned)(((q & 1) * 64 + (q >> 1) * 32 + n) * 16);
}
template <typename OpT, int MI>
__device__ __forceinline__ void kconv16_prefetch(typename Op<OpT>::frag (&A)[8][MI], __amdgpu_buffer_rsrc_t r, unsigned loff, unsigned ctb) {
    static_assert(MI == 1, "kconv16: one 32-channel tile per wave");
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int h = 0; h < 2; ++h) A[2 * s + h][0] = weight_load<OpT>(r, loff + s * 2048 + h * 256, 0);
}
template <typename OpT, int CIN, int MI, int NJ, int STRIDE, int JT0 = 0>
__device__ __forceinline__ void kconv16(f32x4 (&acc)[2 * MI][2 * NJ], typename Op<OpT>::frag (&A)[8][MI], unsigned lds_row,
                                        __amdgpu_buffer_rsrc_t r, unsigned loff, unsigned ctb, int ntaps, int dstep) {
    using frag = typename Op<OpT>::frag;
    constexpr int CC = CIN / 16, GPT = CC / 8, NT = 2 * NJ;
    static_assert(CIN % 128 == 0, "kconv16: C_in must be a multiple of 128");
    static_assert(MI == 1, "kconv16: one 32-channel tile per wave");
    static_assert(JT0 >= 0 && JT0 < NT, "kconv16: at least one column tile runs");
    constexpr unsigned TS = 16u * STRIDE;
    auto ld = [](unsigned a) { return *(const __attribute__((address_space(3))) frag*)(size_t)a; };
    frag Bf[NT];
#pragma unroll
    for (int jt = JT0; jt < NT; ++jt) {
        Bf[jt] = ld(lds_row + jt * TS);
        __builtin_amdgcn_sched_barrier(0);
    }
    const unsigned dS = (unsigned)(dstep * STRIDE);
    const int ngroups = ntaps * GPT;
    const unsigned slast = (unsigned)(ngroups - 1) * 8192u;
    unsigned soff = ngroups > 1 ? 8192u : 0u;
    int gi = 0;
    for (int g = 0; g < ngroups; ++g) {
        const unsigned nrow = (gi + 1 == GPT) ? lds_row - (unsigned)((GPT - 1) * 256) + dS : lds_row + 256u;
        unsigned b0 = lds_row, b1 = nrow;  // (opaque, as in kconv)
        asm volatile("" : "+v"(b0), "+v"(b1));
#pragma unroll
        for (int s = 0; s < 4; ++s) {
#pragma unroll
            for (int jt = JT0; jt < NT; ++jt)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    acc[h][jt] = Op<OpT>::mfma16(A[2 * s + h][0], Bf[jt], acc[h][jt]);
                    if (h == 1) Bf[jt] = ld((s < 3 ? b0 + (unsigned)((s + 1) * 64) : b1) + jt * TS);
                    if (jt == NT - 1) A[2 * s + h][0] = weight_load<OpT>(r, loff + s * 2048 + h * 256, soff);
                    __builtin_amdgcn_sched_barrier(0);
                }
        }
        lds_row = nrow;
        gi = (gi + 1 == GPT) ? 0 : gi + 1;
        soff = soff < slast ? soff + 8192u : soff;
    }
}

template <typename OpT, int CIN, int MI, int NJ, int KGROUP = ::rvcmi::KGROUP, int NB = 2>
__device__ __forceinline__ void conv_core(f32x16 (&acc)[MI][NJ], const char* lds_lane, const OpT* wlane,
                                          long ct_stride, int ntaps_p, int roff, int dstep) {
    typename Op<OpT>::frag A[NB][KGROUP][MI];
    conv_prefetch<OpT, CIN, MI, KGROUP, NB>(A, wlane, ct_stride, ntaps_p);
    conv_run<OpT, CIN, MI, NJ, KGROUP, NB>(acc, A, lds_lane, wlane, ct_stride, ntaps_p, roff, dstep);
}

// Branch-free helpers.  lrelu as max(x, slope*x) (0 < slope < 1); row masking by AND-ing the value bits so that
// the compiler cannot turn the select into divergent control flow (it did: ~45 exec-masked blocks per publish).
// (fmaxf costs a third VALU op per value -- hipcc canonicalises the operand it cannot prove quiet, `v_max_f32 t, v, v` -- but an
//  inline-asm v_max_f32 in its place pins registers: rb_stream phases 3.0k -> 4.1k cycles, 13-29 spills.  Measured, not kept.)
// (round 2 wrote max(v, slope*v) as the median of {v, slope*v, +inf}: LLVM folds a med3 with an infinite operand back into
//  v_max_f32 WITH the canonicalising v_max in front -- the ISA still had 5.5 VALU per masked value.)
__device__ __forceinline__ float lrelu_max(float v, float slope) { return __builtin_amdgcn_fmed3f(v, v * slope, __builtin_inff()); }
__device__ __forceinline__ float mask_bits(float v, unsigned m) { return __uint_as_float(__float_as_uint(v) & m); }

// lrelu(v, 0.1) of a value that is about to become an MFMA operand, as ONE v_mul + ONE v_med3: the median of {v, 0.1 v, TOP}
// is max(v, 0.1 v) whenever that is <= TOP, and TOP otherwise -- for fp16 operands TOP = 65504 is the saturation to_op<> applies
// (identical results for every |v| < 655040; beyond that the fp16 conversion overflows to inf as the reference's .half() does),
// for bf16 TOP = FLT_MAX (no fold to v_max: a finite constant).  3 VALU per published value with the row mask applied to the
// PACKED pair (one v_and per two values) instead of 5.5.
template <typename OpT>
__device__ __forceinline__ float lrelu_op(float v) {
    return __builtin_amdgcn_fmed3f(v, v * 0.1f, 3.4028235e38f);
}
template <>
__device__ __forceinline__ float lrelu_op<_Float16>(float v) {
    return __builtin_amdgcn_fmed3f(v, v * 0.1f, 65504.f);
}
// four activated values -> 4 operands (8 bytes), rows outside the utterance zeroed through the packed words
template <typename OpT, bool MASK>
__device__ __forceinline__ uint2 pack4_lrelu(float a, float b, float c, float d, unsigned m) {
    using o4 = __attribute__((ext_vector_type(4))) OpT;
    o4 o = {(OpT)lrelu_op<OpT>(a), (OpT)lrelu_op<OpT>(b), (OpT)lrelu_op<OpT>(c), (OpT)lrelu_op<OpT>(d)};
    uint2 u = __builtin_bit_cast(uint2, o);
    if constexpr (MASK) {
        u.x &= m;
        u.y &= m;
    }
    return u;
}

// Inter-stage streams Ya[j] as fp16 (option Y_F16): the three ResBlock outputs of a stage are only ever read by
// the next stage's staging loop (k_ups / k_post), which sums them, divides by 3, applies lrelu and -- k_ups -- rounds the result
// to an MFMA operand anyway.  Stored as fp16 (round to nearest even, saturating) they cost half the HBM bytes on the three
// HBM-bound consumers and half the store instructions of the producers; the fp32 residual stream INSIDE a ResBlock is untouched.
__device__ __forceinline__ _Float16 sat_h(float v) { return (_Float16)__builtin_amdgcn_fmed3f(v, -65504.f, 65504.f); }
__device__ __forceinline__ uint2 pack4_h(float a, float b, float c, float d) {
    using h4 = __attribute__((ext_vector_type(4))) _Float16;
    h4 o = {sat_h(a), sat_h(b), sat_h(c), sat_h(d)};
    return __builtin_bit_cast(uint2, o);
}
__device__ __forceinline__ void unpack8_h(const uint4 raw, float (&f)[8]) {
    using h8 = __attribute__((ext_vector_type(8))) _Float16;
    const h8 h = __builtin_bit_cast(h8, raw);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (float)h[e];
}

// acc (MFMA D layout) -> lrelu -> OpT -> LDS operand tile.  `base` already points at this lane's (row, 4*(lane>>5))
// element of the wave's first row; everything else is a compile-time offset.
template <typename OpT, int C, int MI, int NJ, int STRIDE, bool MASK>
__device__ __forceinline__ void publish_operand(char* base, const f32x16 (&acc)[MI][NJ], const unsigned (&rowmask)[NJ],
                                                int cbase = 0) {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if ((C % 32 == 0) || cbase + mi * 32 + 8 * g < C) {  // compile-time true for C % 32 == 0
                    const f32x16& t = acc[mi][jt];
                    *(uint2*)(base + jt * 32 * STRIDE + (mi * 32 + 8 * g) * 2) =
                        pack4_lrelu<OpT, MASK>(t[4 * g + 0], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3], rowmask[jt]);
                }
            }
}

// ... of the 16x16x32 shape (kconv16): tiles of 16 channels x 16 rows, one register quad each
template <typename OpT, int MIH, int NT, int STRIDE, bool MASK>
__device__ __forceinline__ void publish_operand16(char* base, const f32x4 (&acc)[MIH][NT], const unsigned (&rowmask)[NT]) {
#pragma unroll
    for (int mi = 0; mi < MIH; ++mi)
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) {
            const f32x4& t = acc[mi][jt];
            *(uint2*)(base + jt * 16 * STRIDE + mi * 16 * 2) = pack4_lrelu<OpT, MASK>(t[0], t[1], t[2], t[3], rowmask[jt]);
        }
}

// Block barrier that orders LDS traffic ONLY: __syncthreads() carries a workgroup release fence over global memory too, i.e. an
// s_waitcnt vmcnt(0) in front of every s_barrier -- which would drain the weight fragments requested for the next slot (a full
// L2 round trip, exposed four times per pair-step).  The waves of a block exchange data through LDS only.
// (Measured for k_rb_pair / k_rb_full, whose two-plus waves per SIMD already hide that round trip: +1 % time -- they keep __syncthreads.)
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

}  // namespace rvcmi
