// Device kernels of the RMVPE deep U-Net (csrc/unet.hip).  Activations are fp16, channels-last ([B][H][W][C]: H = frames, W = mel bins),
// accumulation and every epilogue fp32.
//
//   k_unet_conv    implicit-GEMM convolution on mfma_f32_16x16x32_f16 for the 3x3 convolution (9 taps), the 1x1 shortcut (1 tap) and the four
//                  output phases of the stride-2 transposed convolution (1, 2, 2, 4 taps).  The weight fragment is the MFMA's A operand (rows =
//                  output channels) and the pixel fragment its B operand (columns = pixels), so a lane ends with 4 consecutive output channels
//                  of one pixel: an 8-byte channels-last store.  Both fragments come straight from global memory: a lane's 8 consecutive k are
//                  8 consecutive input channels of one tap = one 16-byte load (the K dimension tap x channel is contiguous in both images).
//                  Two input tensors are read in place of their concatenation.  Epilogue: y = acc * scale + shift (the eval-mode BatchNorm, or
//                  scale = 1 / shift = bias), ReLU, THEN the residual.  With ksplit > 1 a block sums only its slice of the K loop and stores
//                  fp32 partials; k_unet_reduce adds the slices in slice order (fixed order: bit-identical from run to run) and applies the
//                  same epilogue.
//   k_unet_first   the layers with one input channel (K = 9 or 1, no MFMA): the input BatchNorm is applied while the input is staged, so the
//                  zero padding stays zero.
//   k_unet_pool    AvgPool2d(2, 2).
//
// Ragged batches (rvcmi_unet_forward_ragged): B sequences packed along the frame axis, sequence i in rows [off[i], off[i + 1]) of ONE image of
// R = off[B] rows, every length a multiple of 2^levels -- so at level l the boundaries are off[i] >> l, and the pool and the transposed
// convolution, which pair rows 2 y and 2 y + 1, never straddle one.  The only thing that differs from a dense batch is where the frame axis
// ends for a 3x3 tap: a pixel looks up the sequence that owns its row ONCE (seq_rows, a binary search of the offsets) and carries that
// sequence's first row and row count where the dense form carries b * H and H.  K loop, operand loads and epilogues are the same code.
#pragma once
#include <hip/hip_runtime.h>

namespace rvcmi {
namespace unet {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { MODE_3X3 = 0, MODE_1X1 = 1, MODE_UP = 2 };
enum { OUT_NHWC16 = 0, OUT_HEAD32 = 1 };

struct ConvArgs {
    const _Float16* x0;    // [B][H][W][C0]
    const _Float16* x1;    // [B][H][W][C1], channels C0 .. C0 + C1 - 1 of the concatenation (C1 = 0: none)
    const _Float16* w;     // MODE_3X3 / MODE_1X1: [Cout][tap][Cin]; MODE_UP: the four phases one after the other, each [Cout][tap][Cin]
    const float* scale;    // [Cout rounded up to 16]
    const float* shift;
    const _Float16* res;   // residual in the output's layout, or null
    void* out;             // OUT_NHWC16: fp16 [B][Ho][Wo][Cout];  OUT_HEAD32: fp32 [B][H][Cout][W]
    float* part;           // ksplit > 1: [ksplit][output pixels][Cout] fp32
    int B, H, W, C0, C1, Cout, mode, relu, ksplit, out_kind;
    const int* seq_off;    // ragged: [nseq + 1] ascending level-0 row offsets (B = 1, H = seq_off[nseq] >> seq_shift); null: a dense batch
    int nseq, seq_shift;   // seq_shift: the level of this layer's INPUT rows
};

// The sequence that owns row `r` of a packed image at level `shift`: -> its first row, `rows` = its row count.  off[0] == 0 and
// r < off[nseq] >> shift, so the search ends inside the array.
__device__ __forceinline__ int seq_rows(const int* __restrict__ off, int nseq, int shift, int r, int& rows) {
    int lo = 0, hi = nseq;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((off[mid] >> shift) <= r) lo = mid;
        else hi = mid;
    }
    const int first = off[lo] >> shift;
    rows = (off[lo + 1] >> shift) - first;
    return first;
}

// taps of a phase of the transposed convolution (kernel 3, stride 2, padding 1, output_padding 1): out[2y + p] takes in[y] * w[1] for p = 0 and
// in[y + 1] * w[0] + in[y] * w[2] for p = 1
__host__ __device__ inline int up_taps(int p) { return 1 + p; }

template <int CT, int WC>
__global__ void __launch_bounds__(256) k_unet_conv(const ConvArgs a) {
    constexpr int WP = 4 / WC;  // waves along the pixels
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l16 = lane & 15, g = lane >> 4;
    const int wc = wave % WC, wp = wave / WC;
    const int M = a.B * a.H * a.W;
    const int pix0 = (blockIdx.x * WP + wp) * 32;
    const int co0 = (blockIdx.y * WC + wc) * (16 * CT);
    const int phase = blockIdx.z / a.ksplit, ks = blockIdx.z - phase * a.ksplit;
    const int Cin = a.C0 + a.C1, nch = (Cin + 31) >> 5;
    const int ph_y = phase >> 1, ph_x = phase & 1;
    int ntx = 1, ntaps = 1;
    size_t woff = 0;
    if (a.mode == MODE_3X3) {
        ntx = 3;
        ntaps = 9;
    } else if (a.mode == MODE_UP) {
        ntx = up_taps(ph_x);
        ntaps = up_taps(ph_y) * ntx;
        const int before = phase == 0 ? 0 : phase == 1 ? 1 : phase == 2 ? 3 : 5;  // taps of the phases in front
        woff = (size_t)before * a.Cout * Cin;
    }
    const int niter = ntaps * nch;
    const int it0 = (int)((long long)ks * niter / a.ksplit), it1 = (int)((long long)(ks + 1) * niter / a.ksplit);

    // a pixel: column px, row py of an image of ph rows whose first row is row pr of the whole tensor (dense: image = batch item, ph = H;
    // ragged: image = the sequence that owns the row)
    int py[2], px[2], pr[2], ph[2];
    bool pv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = pix0 + i * 16 + l16;
        pv[i] = m < M;
        const int mm = pv[i] ? m : 0;
        px[i] = mm % a.W;
        const int r = mm / a.W;
        if (a.seq_off) {
            pr[i] = seq_rows(a.seq_off, a.nseq, a.seq_shift, r, ph[i]);
            py[i] = r - pr[i];
        } else {
            py[i] = r % a.H;
            pr[i] = r - py[i];
            ph[i] = a.H;
        }
    }
    const _Float16* wrow[CT];
    bool wv[CT];
#pragma unroll
    for (int j = 0; j < CT; ++j) {
        const int co = co0 + j * 16 + l16;
        wv[j] = co < a.Cout;
        wrow[j] = a.w + woff + (size_t)(wv[j] ? co : 0) * ntaps * Cin;
    }
    f32x4 acc[CT][2];
#pragma unroll
    for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

#pragma unroll 2
    for (int it = it0; it < it1; ++it) {
        const int tap = it / nch, c = ((it - tap * nch) << 5) + g * 8;
        int dy, dx;
        if (a.mode == MODE_3X3) {
            dy = tap / 3 - 1;
            dx = tap - (tap / 3) * 3 - 1;
        } else if (a.mode == MODE_UP) {
            const int ty = tap / ntx, tx = tap - ty * ntx;
            dy = (ph_y && ty == 0) ? 1 : 0;
            dx = (ph_x && tx == 0) ? 1 : 0;
        } else {
            dy = dx = 0;
        }
        const bool cv = c < Cin;
        const bool second = c >= a.C0;
        const _Float16* src = second ? a.x1 : a.x0;
        const int cs = second ? a.C1 : a.C0, cc = second ? c - a.C0 : c;
        half8 xf[2], wf[CT];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int yy = py[i] + dy, xx = px[i] + dx;
            const bool ok = pv[i] && cv && yy >= 0 && yy < ph[i] && xx >= 0 && xx < a.W;
            xf[i] = ok ? *(const half8*)(src + ((size_t)(pr[i] + yy) * a.W + xx) * cs + cc) : zero;
        }
#pragma unroll
        for (int j = 0; j < CT; ++j) wf[j] = (wv[j] && cv) ? *(const half8*)(wrow[j] + (size_t)tap * Cin + c) : zero;
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], xf[i], acc[j][i], 0, 0, 0);
    }

    // lane: pixel l16 of the subtile, output channels 4 g .. 4 g + 3 of the channel subtile
    const bool up = a.mode == MODE_UP;
    const int Ho = up ? 2 * a.H : a.H, Wo = up ? 2 * a.W : a.W;  // (Ho: of the whole tensor, for the partials' slice stride)
    const size_t Mo = (size_t)a.B * Ho * Wo;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (!pv[i]) continue;
        const int oy = up ? 2 * py[i] + ph_y : py[i], ox = up ? 2 * px[i] + ph_x : px[i];
        const size_t opix = ((size_t)(up ? 2 * pr[i] : pr[i]) + oy) * Wo + ox;
#pragma unroll
        for (int j = 0; j < CT; ++j) {
            const int co = co0 + j * 16 + g * 4;
            if (co >= a.Cout) continue;
            const f32x4 v = acc[j][i];
            if (a.ksplit > 1) {  // (only with Cout % 16 == 0)
                *(f32x4*)(a.part + ((size_t)ks * Mo + opix) * a.Cout + co) = v;
                continue;
            }
            const f32x4 sc = *(const f32x4*)(a.scale + co), sh = *(const f32x4*)(a.shift + co);
            float o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o[r] = fmaf(v[r], sc[r], sh[r]);
                if (a.relu) o[r] = fmaxf(o[r], 0.f);
            }
            if (a.out_kind == OUT_HEAD32) {
                float* out = (float*)a.out;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (co + r < a.Cout) out[((size_t)(pr[i] + py[i]) * a.Cout + co + r) * a.W + px[i]] = o[r];
            } else {
                if (a.res) {
                    const half4 rr = *(const half4*)(a.res + opix * a.Cout + co);
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] += (float)rr[r];
                }
                const half4 hv = {(_Float16)o[0], (_Float16)o[1], (_Float16)o[2], (_Float16)o[3]};
                *(half4*)((_Float16*)a.out + opix * a.Cout + co) = hv;
            }
        }
    }
}

// out[p][c .. c + 3] = epilogue(sum over the K slices, in slice order); n4 = output pixels * Cout / 4
__global__ void __launch_bounds__(256) k_unet_reduce(const float* __restrict__ part, int ksplit, size_t n4, int Cout, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, int relu, const _Float16* __restrict__ res,
                                                            _Float16* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const size_t e = i * 4;
    const int co = (int)(e % (size_t)Cout);
    f32x4 v = *(const f32x4*)(part + e);
    for (int k = 1; k < ksplit; ++k) {
        const f32x4 p = *(const f32x4*)(part + (size_t)k * n4 * 4 + e);
        v[0] += p[0];
        v[1] += p[1];
        v[2] += p[2];
        v[3] += p[3];
    }
    const f32x4 sc = *(const f32x4*)(scale + co), sh = *(const f32x4*)(shift + co);
    float o[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        o[r] = fmaf(v[r], sc[r], sh[r]);
        if (relu) o[r] = fmaxf(o[r], 0.f);
    }
    if (res) {
        const half4 rr = *(const half4*)(res + e);
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] += (float)rr[r];
    }
    const half4 hv = {(_Float16)o[0], (_Float16)o[1], (_Float16)o[2], (_Float16)o[3]};
    *(half4*)(out + e) = hv;
}

// One input channel: x fp32 [B][H][W]; staged value = fp16(x * in_scale + in_shift) inside the image, 0 outside.  w [Cout][ntaps] fp16
// (ntaps 9: 3x3 with padding 1, 1: the 1x1 shortcut).  A thread: one pixel, 8 output channels.  seq_off: as in ConvArgs, at level 0.
__global__ void __launch_bounds__(256) k_unet_first(const float* __restrict__ x, float in_scale, float in_shift, const _Float16* __restrict__ w,
                                                           int ntaps, const float* __restrict__ scale, const float* __restrict__ shift, int relu,
                                                           _Float16* __restrict__ out, int B, int H, int W, int Cout,
                                                           const int* __restrict__ seq_off, int nseq) {
    const int groups = Cout >> 3;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t M = (size_t)B * H * W;
    if (i >= M * groups) return;
    const int cg = (int)(i % groups);
    const size_t m = i / groups;
    const int xx = (int)(m % W);
    const size_t row = m / W;
    int yy = (int)(row % H), rows = H;
    size_t first = row - yy;  // first row of the image this pixel belongs to
    if (seq_off && ntaps == 9) {
        const int f = seq_rows(seq_off, nseq, 0, (int)row, rows);
        first = f;
        yy = (int)row - f;
    }
    float in[9];
    if (ntaps == 9) {
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int y2 = yy + t / 3 - 1, x2 = xx + t % 3 - 1;
            const bool ok = y2 >= 0 && y2 < rows && x2 >= 0 && x2 < W;
            in[t] = ok ? (float)(_Float16)fmaf(x[(first + y2) * W + x2], in_scale, in_shift) : 0.f;
        }
    } else {
        in[0] = (float)(_Float16)fmaf(x[m], in_scale, in_shift);
    }
    half8 hv;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int co = cg * 8 + r;
        float s = 0.f;
        if (ntaps == 9) {
#pragma unroll
            for (int t = 0; t < 9; ++t) s = fmaf((float)w[co * 9 + t], in[t], s);
        } else {
            s = (float)w[co] * in[0];
        }
        float o = fmaf(s, scale[co], shift[co]);
        if (relu) o = fmaxf(o, 0.f);
        hv[r] = (_Float16)o;
    }
    *(half8*)(out + m * Cout + cg * 8) = hv;
}

// AvgPool2d(2, 2) on [B][H][W][C] -> [B][H / 2][W / 2][C]; a thread: one output pixel, 8 channels
__global__ void __launch_bounds__(256) k_unet_pool(const _Float16* __restrict__ x, _Float16* __restrict__ out, int B, int H, int W, int C) {
    const int groups = C >> 3, Ho = H >> 1, Wo = W >> 1;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * Ho * Wo * groups) return;
    const int cg = (int)(i % groups);
    const size_t m = i / groups;
    const int xo = (int)(m % Wo), yo = (int)((m / Wo) % Ho);
    const size_t b = m / ((size_t)Wo * Ho);
    const _Float16* p = x + (((b * H + 2 * yo) * W + 2 * xo) * C) + cg * 8;
    const half8 v00 = *(const half8*)p, v01 = *(const half8*)(p + C), v10 = *(const half8*)(p + (size_t)W * C), v11 = *(const half8*)(p + (size_t)W * C + C);
    half8 hv;
#pragma unroll
    for (int r = 0; r < 8; ++r) hv[r] = (_Float16)((((float)v00[r] + (float)v01[r]) + ((float)v10[r] + (float)v11[r])) * 0.25f);
    *(half8*)(out + m * C + cg * 8) = hv;
}

}  // namespace unet
}  // namespace rvcmi
