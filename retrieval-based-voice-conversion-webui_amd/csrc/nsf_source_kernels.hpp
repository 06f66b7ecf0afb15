// Device code of the NSF-HiFi-GAN generator for gfx950 (CDNA4): the sine source and the small kernels in front of conv_pre.
//
// Reference semantics reproduced here (file:line in the reference):
//   sine source            rvc/layers/generators.py:148-194
//   tanh(Linear(1,1))      rvc/layers/nsf.py:57-61
//   cond                   rvc/layers/nsf.py:165-166
#pragma once
#include <hip/hip_runtime.h>

#include "exact_fp.hpp"
#include "mfma_conv.hpp"

namespace rvcmi {

// ------------------------------------------------------------------------------------------------
// Sine source (generators.py:148-194) + source module (nsf.py:57-61)
// ------------------------------------------------------------------------------------------------

// phase[b][t] = fmod(float(sum_{tau<t} w_tau), 1), w_tau = fmod(f0/sr*upp + 0.5, 1) - 0.5.
// torch's CPU cumsum accumulates fp32 inputs in DOUBLE and rounds each prefix to fp32
// (verified against torch 2.10); a wave-level scan in fp64 reproduces that to the last bit, unconditionally:
// every w is a multiple of 2^-25 (rad + 0.5 >= 0.5 has an ulp of 2^-24 or more, fmodf and the subtraction are exact),
// so every partial sum is an exact fp64 number in any order and the one rounding to fp32 is the same everywhere
// (tests/test_cpu_source.py holds this partition, torch's cumsum and exact integer prefix sums against each other bit for
// bit).  One block of 256 threads per utterance (the frames' slow fmod / divide chain is spread
// over 4 waves: 15 -> ~5 us for a 10 s clip; the block-level scan goes through LDS).
static __global__ void __launch_bounds__(256) k_phase_scan(const float* __restrict__ f0, float* __restrict__ phase,
                                                   int T, float sr, float upp, const int* __restrict__ lens) {
#pragma clang fp contract(off)
    __shared__ double wsum[4];
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* f = f0 + (size_t)b * T;
    float* ph = phase + (size_t)b * T;
    // (ragged batch: the item's own frame count sets the thread partition, so the fp64 prefix sums are those of a separate call)
    const int n = item_rows(lens, b, 1, T) - 1;  // increments come from frames 0..T-2
    const int per = (n + 255) / 256;
    const int beg = min(n, tid * per);
    const int end = min(n, beg + per);
    double local = 0.0;
    for (int t = beg; t < end; ++t) {
        float rad = mul_rn(div_rn(f[t], sr), upp);
        float w = sub_rn(fmodf(add_rn(rad, 0.5f), 1.0f), 0.5f);
        local += (double)w;
    }
    // inclusive wave scan of the per-thread sums, then the waves' totals through LDS
    double incl = local;
    for (int off = 1; off < 64; off <<= 1) {
        double o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    double run = incl - local;  // exclusive prefix inside the wave
    for (int w = 0; w < wave; ++w) run += wsum[w];
    if (tid == 0) ph[0] = 0.f;
    for (int t = beg; t < end; ++t) {
        float rad = mul_rn(div_rn(f[t], sr), upp);
        float w = sub_rn(fmodf(add_rn(rad, 0.5f), 1.0f), 0.5f);
        run += (double)w;
        ph[t + 1] = fmodf((float)run, 1.0f);
    }
}

// har[b][t*upp + n-1] = tanh(lw * (0.1*sin(2*pi*(f0/sr*n + phase)) * uv + amp * noise) + lb)
static __global__ void __launch_bounds__(256) k_sine_source(const float* __restrict__ f0, const float* __restrict__ phase,
                                                     const float* __restrict__ noise, float* __restrict__ har,
                                                     int T, int upp, float sr, float lw, float lb, size_t total) {
#pragma clang fp contract(off)
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    size_t frame = i / (size_t)upp;  // b*T + t
    int n = (int)(i - frame * upp) + 1;
    float f = f0[frame];
    float rad = add_rn(mul_rn(div_rn(f, sr), (float)n), phase[frame]);
    float s = mul_rn(sinf(mul_rn(6.2831855f, rad)), 0.1f);
    float uv = f > 0.f ? 1.f : 0.f;
    float amp = f > 0.f ? 0.003f : div_rn(0.1f, 3.0f);
    float nz = noise ? noise[i] : 0.f;
    float v = add_rn(mul_rn(s, uv), mul_rn(amp, nz));
    har[i] = tanhf(add_rn(mul_rn(v, lw), lb));
}

// F.interpolate(mode="linear", align_corners=False) along the last axis of [rows][Lin] -> [rows][Lout]
// (nsf.py:155-162, generators.py:76-79).
// Output sample o of one row r[Lin] -> [Lout]: the arithmetic both kernels below share, so that a row comes out the same bits from either.
__device__ __forceinline__ float interp_linear_at(const float* __restrict__ r, int Lin, int Lout, int o) {
    float scale = (float)Lin / (float)Lout;
    float src = scale * ((float)o + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    int i0 = (int)src;
    if (i0 > Lin - 1) i0 = Lin - 1;
    int i1 = i0 + (i0 < Lin - 1 ? 1 : 0);
    float l1 = src - (float)i0;
    float l0 = 1.f - l1;
    return l0 * r[i0] + l1 * r[i1];
}

static __global__ void __launch_bounds__(256) k_interp_linear(const float* __restrict__ in, float* __restrict__ out,
                                                       int Lin, int Lout, size_t total) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    size_t row = i / (size_t)Lout;
    int o = (int)(i - row * Lout);
    out[i] = interp_linear_at(in + row * (size_t)Lin, Lin, Lout, o);
}

// The same with a target length PER ITEM (rvcmi_nsf_forward_nres): rows [B * rows_per_item][Lin] -> [B * rows_per_item][Lmax], a row of
// item b interpolated to n_res[b] * mul samples exactly as k_interp_linear does it for Lout = n_res[b] * mul, zeros behind them.  An item
// whose target is Lin is copied: the single-item forward does not interpolate then (nsf.py:155, generators.py:76).
static __global__ void __launch_bounds__(256) k_interp_linear_ragged(const float* __restrict__ in, float* __restrict__ out,
                                                              const int* __restrict__ n_res, int rows_per_item, int mul, int Lin,
                                                              int Lmax, size_t total) {
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    size_t row = i / (size_t)Lmax;
    int o = (int)(i - row * Lmax);
    const int Lout = item_rows(n_res, (int)(row / (size_t)rows_per_item), mul, Lmax);  // (clamped to [mul, Lmax]: nothing is read or written outside the rows)
    const float* r = in + row * (size_t)Lin;
    float v = 0.f;
    if (o < Lout) v = Lout == Lin ? r[o] : interp_linear_at(r, Lin, Lout, o);
    out[i] = v;
}

// cond(g): a 1x1 conv over a length-1 sequence = one GEMV per utterance (nsf.py:165-166).
// One wave per output channel: the weight row is read coalesced and reduced with xor-shuffles.
static __global__ void __launch_bounds__(256) k_cond(const float* __restrict__ g, const float* __restrict__ Wc,
                                              const float* __restrict__ bc, float* __restrict__ out, int gin, int C0) {
    const int b = blockIdx.y;
    const int co = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (co >= C0) return;
    float acc = 0.f;
    for (int i = lane; i < gin; i += 64) acc = fmaf(Wc[(size_t)co * gin + i], g[(size_t)b * gin + i], acc);
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) out[(size_t)b * C0 + co] = acc + bc[co];
}

}  // namespace rvcmi
