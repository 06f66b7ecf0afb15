// The front's "fp16x2" operand mode (RVCMI_OPERAND_F16X2): fp32-grade enc_p / flow on the fp16 matrix cores.
//
// Every MFMA operand -- packed weights, staged activations, q / k / v, the softmax probabilities, the relative key embeddings, the FFN's
// ReLU output, the WN gate output -- is a (hi, lo') pair of fp16 values, hi = fp16(x), lo' = fp16((x - hi) * 2^11) (csrc/split_f16.hpp:
// the scale keeps lo' a NORMAL fp16 number down to residuals of 2^-25, so nothing depends on how the matrix cores treat subnormal inputs).  A k-step is three
// v_mfma_f32_32x32x16_f16:
//     acc  += A_hi * B_hi
//     accx += A_hi * B_lo' + A_lo' * B_hi          (lo * lo, 2^-22 relative, is dropped)
// and the epilogue takes acc + 2^-11 * accx.  Everything that is fp32 in the other modes stays fp32 (bias, LayerNorm, softmax, gates,
// masks, residual and flow streams); the epilogues are k_fr_conv's own (OpT = F16x2: operand outputs go out as two planes).
//
// Layout: PLANAR.  Each operand buffer, weight pack and LDS tile is a hi plane followed by a lo plane, each with exactly the fp16 layout.
//
// One launch form per layer (k_fr_conv<F16x2> for every conv, two launches per WN layer, k_fs_attn): the accumulator pair does not fit next to
// the fused FFN's / WN layer's second K loop in 256 registers at six waves, and the mode's point is fidelity.  The summation order of an
// output element does not depend on the grid, so a batch item is bit-equal to the clip run alone, at either tile height.
#pragma once
#include "front_kernels.hpp"

namespace rvcmi {

// Input channels are staged FsTile::CK = 256 at a time (768-channel inputs: three chunks), so that two planes of a 64-row tile fit the LDS:
// chunk-major K order (chunk, tap, k-step), the same at every tile height.
template <int CIN>
struct FsTile {
    static constexpr int CK = CIN > 256 ? 256 : CIN;
    static constexpr int NCH = CIN / CK;
    static constexpr int CCK = CK / 16;             // k-steps per tap and chunk
    static constexpr int STRIDE = Tile<CK>::STRIDE;  // bytes per LDS row of one plane
    static_assert(CIN % CK == 0 && CCK % 4 == 0, "chunks of whole 4-k-step groups");
};

__device__ __forceinline__ void fs_split8(const float (&f)[8], f16x8& hi, f16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        hi[e] = to_op<_Float16>(f[e]);
        lo[e] = to_op<_Float16>((f[e] - (float)hi[e]) * FS_SCALE);
    }
}

// Stage channels [c0, c0 + CK) of rows [g0, g0 + rows) into the hi / lo LDS planes; zero outside [0, min(T, lenrow)).
// in_op = 0: fp32 [..][cin], split here; in_op = 1: fp16 planes [..][cin], the lo plane in_plane elements behind the hi plane.
template <int CK>
__device__ __forceinline__ void fs_stage(char* smem, size_t lds_plane, const void* in, int in_op, size_t in_plane, long boff, int cin, int c0,
                                         int T, int g0, int rows, int lenrow, int NT) {
    constexpr int STRIDE = Tile<CK>::STRIDE, C8 = CK / 8;
    const int top = min(T, lenrow);
    for (int idx = threadIdx.x; idx < rows * C8; idx += NT) {
        const int r = idx / C8, c8 = idx - r * C8, gr = g0 + r, grc = min(max(gr, 0), T - 1);
        const size_t off = (size_t)boff + (size_t)grc * cin + c0 + c8 * 8;
        f16x8 hi, lo;
        if (in_op) {
            hi = *(const f16x8*)((const _Float16*)in + off);
            lo = *(const f16x8*)((const _Float16*)in + in_plane + off);
        } else {
            const float4* p = (const float4*)((const float*)in + off);
            const float4 x0 = p[0], x1 = p[1];
            const float f[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
            fs_split8(f, hi, lo);
        }
        if (!(gr >= 0 && gr < top)) {
#pragma unroll
            for (int e = 0; e < 8; ++e) hi[e] = lo[e] = (_Float16)0.f;
        }
        *(f16x8*)(smem + (size_t)r * STRIDE + c8 * 16) = hi;
        *(f16x8*)(smem + lds_plane + (size_t)r * STRIDE + c8 * 16) = lo;
    }
}

// Staging and K loop of k_fr_conv (front_kernels.hpp: same grid, same arguments, same epilogues) on operand pairs.
// Packed weights: hi plane, then the lo plane ctiles * ct_stride elements behind it.  A ring of 4 k-steps of weights is in flight.
template <int CIN, int MI, int NJ, int NW>
__device__ __forceinline__ void fs_conv_sums(const FrConvArgs& a, f32x16 (&acc)[MI][NJ], char* smem, int b, int q0, int ct0, int lenrow) {
    using FT = FsTile<CIN>;
    using frag = f16x8;
    constexpr int CK = FT::CK, NCH = FT::NCH, CC = CIN / 16, CCK = FT::CCK, STRIDE = FT::STRIDE, NT = 64 * NW, TT = NJ * 32, D = 4;
    const int lane = threadIdx.x & 63, hl = lane >> 5;
    const int rows = TT + a.ntaps - 1;
    const size_t lds_plane = (size_t)rows * STRIDE;
    const size_t in_plane = (size_t)gridDim.z * a.in_bstride;
    const int ctiles = (a.cout + 31) / 32;
    const size_t wplane = (size_t)ctiles * a.ct_stride;
    const _Float16* wl[MI];  // (a wave past the last tile re-reads it: every load stays inside the pack, its results are never stored)
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) wl[mi] = (const _Float16*)a.w + (size_t)min(ct0 + mi, ctiles - 1) * a.ct_stride + lane * 8;
    frag Ah[D][MI], Al[D][MI];
    auto loadA = [&](int u, int kstep) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
            Ah[u][mi] = *(const frag*)(wl[mi] + (size_t)kstep * 512);
            Al[u][mi] = *(const frag*)(wl[mi] + wplane + (size_t)kstep * 512);
        }
    };
    // (chunk, tap, first k-step) of the group of D k-steps to request next, in the order the loop below consumes them
    int n_chunk = 0, n_tap = 0, n_c = 0;
    auto advance = [&]() {
        n_c += D;
        if (n_c == CCK) {
            n_c = 0;
            if (++n_tap == a.ntaps) {
                n_tap = 0;
                ++n_chunk;
            }
        }
    };
#pragma unroll
    for (int u = 0; u < D; ++u) loadA(u, u);
    advance();

    f32x16 acx[MI][NJ];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][jt][e] = acx[mi][jt][e] = 0.f;

#pragma unroll 1
    for (int ch = 0; ch < NCH; ++ch) {
        if (ch > 0) __syncthreads();  // every wave is done with the previous chunk's tile
        fs_stage<CK>(smem, lds_plane, a.in, a.in_op, in_plane, (long)b * a.in_bstride, CIN, ch * CK, a.T, q0 - a.pad, rows, lenrow, NT);
        __syncthreads();
#pragma unroll 1
        for (int tap = 0; tap < a.ntaps; ++tap) {
            const char* tb = smem + (size_t)((lane & 31) + tap) * STRIDE + hl * 16;
#pragma unroll 1
            for (int c = 0; c < CCK; c += D) {
                const bool more = n_chunk < NCH;
                const int kn = more ? n_tap * CC + n_chunk * CCK + n_c : 0;  // behind the last group: an in-bounds request nobody uses
#pragma unroll
                for (int u = 0; u < D; ++u) {
                    frag Bh[NJ], Bl[NJ];
#pragma unroll
                    for (int jt = 0; jt < NJ; ++jt) {
                        Bh[jt] = *(const frag*)(tb + (c + u) * 32 + (size_t)jt * 32 * STRIDE);
                        Bl[jt] = *(const frag*)(tb + lds_plane + (c + u) * 32 + (size_t)jt * 32 * STRIDE);
                    }
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                        for (int jt = 0; jt < NJ; ++jt) {
                            acc[mi][jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[u][mi], Bh[jt], acc[mi][jt], 0, 0, 0);
                            acx[mi][jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Ah[u][mi], Bl[jt], acx[mi][jt], 0, 0, 0);
                            acx[mi][jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(Al[u][mi], Bh[jt], acx[mi][jt], 0, 0, 0);
                        }
                    loadA(u, kn + u);
                }
                if (more) advance();
            }
        }
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][jt][e] += acx[mi][jt][e] * FS_INV;
}

// k_fr_attn (front_kernels.hpp: same block shape, same online softmax, same merge) on operand pairs: q, k, v, the relative key embeddings
// and the probabilities P = exp(S - m) are (hi, lo') pairs; the relative VALUE term is fp32 arithmetic in both.
//   q / out: hi plane [B][T][H], the lo plane B * T * H elements behind it;  kf / vf: lo plane B * H * Tp elements behind the hi plane;
//   relk: [2][dk/16][64][8].
template <int DK, int NBAND>
static __global__ void __launch_bounds__(256) k_fs_attn(FrAttnArgs a) {
    using frag = f16x8;
    constexpr int KS = DK / 16, DT = DK / 32, OS = DK + 1, DG = DK / 8;
    static_assert(DK % 32 == 0, "head dim must be a multiple of 32");
    __shared__ float Rl[32 * 33];
    __shared__ float Ml[4 * 32], Ll[4 * 32];
    __shared__ float Ol[4 * 32 * OS];
    __shared__ float Sb[32 * 32 + 32];
    __shared__ float Mf[32], Lf[32];
    __shared__ float Wl[4 * 32];
    __shared__ __attribute__((aligned(16))) float Ev[32 * DK];
    const int qt = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int q0 = qt * 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, hl = lane >> 5, ql = lane & 31;
    const int T = a.T;
    const int len = a.len ? (int)min((long long)T, a.len[b]) : T;
    const int nh = a.H / DK, ntl = a.Tp / 32;
    const size_t bt_plane = (size_t)gridDim.z * T * a.H, kv_plane = (size_t)gridDim.z * a.H * a.Tp;
    const _Float16* KF = (const _Float16*)a.kf + ((size_t)b * nh + h) * ntl * (KS * 512) + lane * 8;
    const _Float16* VF = (const _Float16*)a.vf + ((size_t)b * nh + h) * ntl * (DT * 2 * 512) + lane * 8;
    auto mfma = [](frag x, frag y, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0); };

    frag Bq[KS], Bql[KS];
    {
        const _Float16* qp = (const _Float16*)a.q + ((size_t)b * T + min(q0 + ql, T - 1)) * a.H + h * DK + 8 * hl;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            Bq[s] = *(const frag*)(qp + 16 * s);
            Bql[s] = *(const frag*)(qp + bt_plane + 16 * s);
        }
    }
    constexpr int EVN = 32 * DK / 256;
    float evr[EVN];
    {
        const int nev = (2 * a.ws + 1) * DK;
#pragma unroll
        for (int u = 0; u < EVN; ++u) {
            const int i = threadIdx.x + u * 256;
            const float v = a.relv[min(i, nev - 1)];
            evr[u] = i < nev ? v : 0.f;
        }
    }
    for (int i = threadIdx.x; i < 32 * 32; i += 256) Sb[i] = -INFINITY;
    if (wave == 0) {  // R[q][r] = q . E_k[r]
        f32x16 r = {0}, rx = {0};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const frag eh = *(const frag*)((const _Float16*)a.relk + (size_t)s * 512 + lane * 8);
            const frag el = *(const frag*)((const _Float16*)a.relk + (size_t)(KS + s) * 512 + lane * 8);
            r = mfma(eh, Bq[s], r);
            rx = mfma(eh, Bql[s], rx);
            rx = mfma(el, Bq[s], rx);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) Rl[ql * 33 + (i & 3) + 8 * (i >> 2) + 4 * hl] = r[i] + rx[i] * FS_INV;
    }
    __syncthreads();

    const int q = q0 + ql;
    const bool qok = q < len;
    float m_run = -INFINITY, l_run = 0.f;
    f32x16 O[DT], Ox[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) O[d][i] = Ox[d][i] = 0.f;
    const int nkt = (T + 31) / 32;
    struct KP {
        frag k[KS], kl[KS];
    };
    struct VP {
        frag v[DT][2], vl[DT][2];
    };
    auto load_k = [&](int kt, KP& t) {
        const int kc = min(kt, nkt - 1);  // clamped: unconditional loads
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            t.k[s] = *(const frag*)(KF + ((size_t)kc * KS + s) * 512);
            t.kl[s] = *(const frag*)(KF + kv_plane + ((size_t)kc * KS + s) * 512);
        }
    };
    auto load_v = [&](int kt, VP& t) {
        const int kc = min(kt, nkt - 1);
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                t.v[d][s2] = *(const frag*)(VF + (((size_t)kc * DT + d) * 2 + s2) * 512);
                t.vl[d][s2] = *(const frag*)(VF + kv_plane + (((size_t)kc * DT + d) * 2 + s2) * 512);
            }
    };
    const int qrel = 4 * hl - q + a.ws;
    auto compute_tile = [&](int kt, const KP& tk, const VP& tv) {
        const int j0 = kt * 32;
        f32x16 S = {0}, Sx = {0};
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            S = mfma(tk.k[s], Bq[s], S);
            Sx = mfma(tk.k[s], Bql[s], Sx);
            Sx = mfma(tk.kl[s], Bq[s], Sx);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i] += Sx[i] * FS_INV;
        const bool near = (j0 >= q0 - 32 - a.ws) && (j0 <= q0 + 32 + a.ws);
        const bool plain = !near && j0 + 32 <= len && (q0 + 32 <= len || len == T);
        float mx = -INFINITY;
        if (plain) {
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, S[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int ci = (i & 3) + 8 * (i >> 2);
                const int j = j0 + ci + 4 * hl;
                float s = S[i];
                const int rel = j0 + ci + qrel;
                const bool inband = near && rel >= 0 && rel <= 2 * a.ws;
                const float rv = Rl[ql * 33 + min(max(rel, 0), 2 * a.ws)];
                s += inband ? rv : 0.f;
                s = (qok && j < len) ? s : -1e4f;  // masked_fill(mask == 0, -1e4), attentions.py:115
                s = j < T ? s : -INFINITY;         // tile padding: not a key at all
                Sb[inband ? ql * 32 + rel : 32 * 32 + (lane & 31)] = s;
                S[i] = s;
                mx = fmaxf(mx, s);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        float ps = 0.f;
        frag Bp[2], Bpl[2];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float p = __expf(S[i] - m_new);  // in [0, 1]
            ps += p;
            const _Float16 ph = (_Float16)p;
            Bp[i >> 3][i & 7] = ph;
            Bpl[i >> 3][i & 7] = (_Float16)((p - (float)ph) * FS_SCALE);
        }
        if (__builtin_amdgcn_ballot_w64(m_new > m_run) != 0) {
            const float sc = __expf(m_run - m_new);
            l_run *= sc;
#pragma unroll
            for (int d = 0; d < DT; ++d)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    O[d][i] *= sc;
                    Ox[d][i] *= sc;
                }
        }
        l_run += ps;
        m_run = m_new;
#pragma unroll
        for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                O[d] = mfma(tv.v[d][s2], Bp[s2], O[d]);
                Ox[d] = mfma(tv.v[d][s2], Bpl[s2], Ox[d]);
                Ox[d] = mfma(tv.vl[d][s2], Bp[s2], Ox[d]);
            }
    };
    {
        // the next tile's k pairs are requested before the current tile is multiplied; its v pairs ahead of the score product
        KP k0, k1;
        VP v;
        int kt = wave;
        load_k(kt, k0);
        while (kt < nkt) {
            load_k(kt + 4, k1);
            load_v(kt, v);
            compute_tile(kt, k0, v);
            kt += 4;
            if (kt >= nkt) break;
            load_k(kt + 4, k0);
            load_v(kt, v);
            compute_tile(kt, k1, v);
            kt += 4;
        }
    }
#pragma unroll
    for (int u = 0; u < EVN; ++u) Ev[threadIdx.x + u * 256] = evr[u];
    l_run += __shfl_xor(l_run, 32, 64);
    if (hl == 0) {
        Ml[wave * 32 + ql] = m_run;
        Ll[wave * 32 + ql] = l_run;
    }
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int i = 0; i < 16; ++i) Ol[(wave * 32 + ql) * OS + d * 32 + (i & 3) + 8 * (i >> 2) + 4 * hl] = O[d][i] + Ox[d][i] * FS_INV;
    __syncthreads();
    if (threadIdx.x < 32) {
        const int x = threadIdx.x;
        float M = fmaxf(fmaxf(Ml[x], Ml[32 + x]), fmaxf(Ml[64 + x], Ml[96 + x]));
        float L = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) L += Ll[w * 32 + x] * __expf(Ml[w * 32 + x] - M);
        Mf[x] = M;
        Lf[x] = L;
#pragma unroll
        for (int w = 0; w < 4; ++w) Wl[w * 32 + x] = __expf(Ml[w * 32 + x] - M) / L;
    }
    __syncthreads();
    {
        const int x = threadIdx.x & 31, dg = threadIdx.x >> 5;
        const float M = Mf[x], Li = 1.f / Lf[x];
        float pb[NBAND];
#pragma unroll
        for (int r = 0; r < NBAND; ++r) pb[r] = __expf(Sb[x * 32 + r] - M) * Li;
        float w4[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) w4[w] = Wl[w * 32 + x];
        const size_t out0 = ((size_t)b * T + min(q0 + x, T - 1)) * a.H + h * DK + dg * DG;
#pragma unroll
        for (int c4 = 0; c4 < DG / 4; ++c4) {
            const int d = dg * DG + c4 * 4;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += Ol[(w * 32 + x) * OS + d + e] * w4[w];
#pragma unroll
            for (int r = 0; r < NBAND; ++r) acc += *(const f32x4*)(Ev + r * DK + d) * pb[r];  // relative values, attentions.py:127-135
            if (q0 + x < T) fs_put4(a.out, out0 + c4 * 4, bt_plane, acc);
        }
    }
}

}  // namespace rvcmi
