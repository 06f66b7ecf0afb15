// Device-resident pre-/post-glue of Pipeline.vc / Pipeline.pipeline: the small host-side
// numpy / python steps between the PyTorch-ROCm feature extractors and net_g.infer, so that nothing has to leave the GPU.
//
//   x2 nearest interpolation + protect mix   infer/modules/vc/pipeline.py:140-159
//   RMVPE salience -> cents -> Hz            rvc/f0/rmvpe.py:119-164
//   _resize_f0 / _interpolate_f0             rvc/f0/f0.py:31-78
//   post_process (key shift, mel binning)    rvc/f0/gen.py:10-41
//   int16 scaling                            infer/modules/vc/pipeline.py:355-359
//
// These are HBM/latency-bound byte shuffles and short fp64 recurrences -- no MFMA here.  fp64 wherever numpy computes in
// float64 (the whole f0 chain), fp32 with contraction off wherever torch computes in float32.
#pragma once
#include <hip/hip_runtime.h>

#include "exact_fp.hpp"
#include <stdint.h>

#include "../../include/rvcmi.h"  // rvcmi_resample_row, rvcmi_f0_row

namespace rvcmi {

// feats = blend(search) per query row i (pipeline.py:129-138, see k_blend), then for output frame t < p_len:
//   x = row[t / 2]                               F.interpolate(scale_factor=2), nearest   (pipeline.py:140-144)
//   out[t] = x * pf + feats0[t/2] * (1 - pf),  pf = pitchf[t] >= 1 ? 1 : protect         (pipeline.py:153-158)
// One block per QUERY row (both of its output frames): the blended row is computed once, in registers.
// P == nullptr: no retrieval (index_rate == 0 / no index): the row is the input row.
// The body: query row qi of feats [nq, d] -> output frames qi * reps .. of out [p_len, d]; D / P are the row's own k results (read
// only when blend).  The body of k_blend_expand_batch; a single stream is that kernel at S = 1.
__device__ __forceinline__ void blend_expand_row(const float* __restrict__ feats, const float* __restrict__ D, const int64_t* __restrict__ P,
                                                 const float* __restrict__ vecs, int d, int k, int64_t pos_last, float rate, float omr,
                                                 bool blend, const float* __restrict__ pitchf, float protect, int64_t p_len, int reps,
                                                 float* __restrict__ out, int64_t qi) {
#pragma clang fp contract(off)
    float w[8];
    if (blend) {
        for (int s = 0; s < k; ++s) {
            const float inv = div_rn(1.0f, D[s]);
            w[s] = mul_rn(inv, inv);
        }
        float sum;
        if (k == 8) {
            sum = add_rn(add_rn(add_rn(w[0], w[1]), add_rn(w[2], w[3])),
                            add_rn(add_rn(w[4], w[5]), add_rn(w[6], w[7])));
        } else {
            sum = w[0];
            for (int s = 1; s < k; ++s) sum = add_rn(sum, w[s]);
        }
        for (int s = 0; s < k; ++s) w[s] = div_rn(w[s], sum);
    }
    for (int e = threadIdx.x; e < d; e += 256) {
        const float f = feats[qi * d + e];
        float x = f;
        if (blend) {
            float acc = 0.f;
            for (int s = 0; s < k; ++s) {
                int64_t p = P[s];
                if (p < 0) p = pos_last;
                const float prod = mul_rn(vecs[p * d + e], w[s]);
                acc = s == 0 ? prod : add_rn(acc, prod);
            }
            x = add_rn(mul_rn(acc, rate), mul_rn(omr, f));
        }
        for (int r = 0; r < reps; ++r) {
            const int64_t t = qi * reps + r;
            if (t >= p_len) break;
            float o = x;
            if (pitchf) {
                const float pf = pitchf[t] < 1.f ? protect : 1.f;  // pitchff[pitchf > 0] = 1; pitchff[pitchf < 1] = protect
                o = add_rn(mul_rn(x, pf), mul_rn(f, sub_rn(1.f, pf)));
            }
            out[t * d + e] = o;
        }
    }
}

// The realtime guard per SESSION (rtrvc.py:172-180 is a per-call condition; in a bank a call is one session's block):
// flags[s] = 1 when any of session s's m * k result ids is negative.  One block per session.
static __global__ void __launch_bounds__(256) k_session_short(const int64_t* __restrict__ I, int64_t per_session, int* __restrict__ flags) {
    __shared__ int any;
    if (threadIdx.x == 0) any = 0;
    __syncthreads();
    const int64_t* row = I + (int64_t)blockIdx.x * per_session;
    int mine = 0;
    for (int64_t i = threadIdx.x; i < per_session; i += 256) mine |= row[i] < 0 ? 1 : 0;
    if (mine) atomicOr(&any, 1);
    __syncthreads();
    if (threadIdx.x == 0) flags[blockIdx.x] = any;
}

// The searched rows of every session, feats [S, nq, d] rows [skip, nq), packed into q [S * (nq - skip), d] for ONE search.
static __global__ void __launch_bounds__(256) k_gather_tail_rows(const float* __restrict__ feats, int64_t nq, int64_t skip, int d,
                                                                 float* __restrict__ q) {
    const int64_t m = nq - skip;
    const int64_t r = blockIdx.x, s = blockIdx.y;
    const float* src = feats + (s * nq + skip + r) * d;
    float* dst = q + (s * m + r) * d;
    for (int e = threadIdx.x; e < d; e += 256) dst[e] = src[e];
}

// blend_expand_row per session: grid (nq, S); S = 1, skip = 0 is the single-stream form (result row qi, flags[0]).  Row qi < skip of a session is expanded un-blended; row qi >= skip uses result row
// s * (nq - skip) + qi - skip of the one search and blends unless the session's flag is set (skip_if_short).  P == nullptr: no
// retrieval at all.  feats [S, nq, d], pitchf [S, p_len] or nullptr, out [S, p_len, d].
static __global__ void __launch_bounds__(256) k_blend_expand_batch(const float* __restrict__ feats, const float* __restrict__ D,
                                                                   const int64_t* __restrict__ P, const float* __restrict__ vecs, int d,
                                                                   int k, int64_t pos_last, float rate, float omr,
                                                                   const int* __restrict__ flags, int skip_if_short, int64_t nq,
                                                                   int64_t skip, const float* __restrict__ pitchf, float protect,
                                                                   int64_t p_len, int reps, float* __restrict__ out) {
    const int64_t qi = blockIdx.x, s = blockIdx.y;
    const bool blend = P != nullptr && qi >= skip && !(skip_if_short && flags[s]);
    const int64_t ri = s * (nq - skip) + (qi - skip);
    blend_expand_row(feats + s * nq * d, blend ? D + ri * k : nullptr, blend ? P + ri * k : nullptr, vecs, d, k, pos_last, rate, omr, blend,
                     pitchf ? pitchf + s * p_len : nullptr, protect, p_len, reps, out + s * p_len * d, qi);
}

// ---- the same three steps with the retrieval controls per session (rvcmi_ivf_search_blend_expand_sessions): sess [S] on the device; a
// session with slot in [0, active) is searched and blended, its rows packed at that slot; any other leaves on a branch that is uniform
// per block (the session is blockIdx.y).  `active` is the host's count: a device copy that disagrees cannot take a block out of the
// packed buffers.
static __global__ void __launch_bounds__(256) k_gather_session_rows(const float* __restrict__ feats, int64_t nq, int64_t skip, int d,
                                                                    const rvcmi_session_blend* __restrict__ sess, int active,
                                                                    float* __restrict__ q) {
    const int64_t m = nq - skip;
    const int64_t r = blockIdx.x, s = blockIdx.y;
    const int slot = sess[s].slot;
    if (slot < 0 || slot >= active) return;
    const float* src = feats + (s * nq + skip + r) * d;
    float* dst = q + ((int64_t)slot * m + r) * d;
    for (int e = threadIdx.x; e < d; e += 256) dst[e] = src[e];
}

// blend_expand_row per session with the session's own rate and protect: grid (nq, S).  flags [active]: k_session_short over the packed
// slots.  A session without a slot (or with P == nullptr: nothing was searched) is expanded un-blended: x = f, the bits of the input.
// pitchf [S, p_len] or nullptr; a session whose protect_on is 0 gets o = x, as a null pitchf gives.  omr is the double difference rounded
// once, as the host computes it for the scalar entry.
static __global__ void __launch_bounds__(256) k_blend_expand_sessions(const float* __restrict__ feats, const float* __restrict__ D,
                                                                      const int64_t* __restrict__ P, const float* __restrict__ vecs, int d,
                                                                      int k, int64_t pos_last, const rvcmi_session_blend* __restrict__ sess,
                                                                      int active, const int* __restrict__ flags, int skip_if_short,
                                                                      int64_t nq, int64_t skip, const float* __restrict__ pitchf,
                                                                      int64_t p_len, int reps, float* __restrict__ out) {
    const int64_t qi = blockIdx.x, s = blockIdx.y;
    const rvcmi_session_blend c = sess[s];
    const bool has_slot = P != nullptr && c.slot >= 0 && c.slot < active;
    const bool blend = has_slot && qi >= skip && !(skip_if_short && flags[c.slot]);
    const int64_t ri = blend ? (int64_t)c.slot * (nq - skip) + (qi - skip) : 0;
    const float omr = (float)(1.0 - (double)c.index_rate);
    blend_expand_row(feats + s * nq * d, blend ? D + ri * k : nullptr, blend ? P + ri * k : nullptr, vecs, d, k, pos_last, c.index_rate, omr,
                     blend, (pitchf && c.protect_on) ? pitchf + s * p_len : nullptr, c.protect, p_len, reps, out + s * p_len * d, qi);
}

// RMVPE._to_local_average_cents + _decode (rmvpe.py:119-164): one wave per frame.
//   center = argmax(salience[f]) (first maximum); 9-bin window, zero-padded salience AND zero-padded cents table;
//   cents = sum(sal*cm) / sum(sal)   product in float64, weight sum in float32 (numpy's pairwise order for n = 9);
//   0 where max <= thred;  f0 = 10 * 2^(cents/1200), 0 where that equals 10.
static __global__ void __launch_bounds__(256) k_rmvpe_decode(const float* __restrict__ sal, int n, int nbins, float thred,
                                                             double* __restrict__ f0) {
#pragma clang fp contract(off)
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (f >= n) return;
    const float* s = sal + (size_t)f * nbins;
    float best = -INFINITY;
    int bi = 0;
    for (int i = lane; i < nbins; i += 64) {
        const float v = s[i];
        if (v > best) {  // strictly greater keeps the first maximum inside a lane (indices ascend)
            best = v;
            bi = i;
        }
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (ob > best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
    if (lane == 0) {
        double prod[9];
        float wv[9];
        for (int w = 0; w < 9; ++w) {
            const int b = bi - 4 + w;
            const bool in = b >= 0 && b < nbins;
            const float sv = in ? s[b] : 0.f;
            const double cm = in ? 20.0 * (double)b + 1997.3794084376191 : 0.0;
            wv[w] = sv;
            prod[w] = (double)sv * cm;
        }
        // numpy pairwise sum of 9 elements: 8 accumulators combined as a tree, then the 9th
        const double ps = (((prod[0] + prod[1]) + (prod[2] + prod[3])) + ((prod[4] + prod[5]) + (prod[6] + prod[7]))) + prod[8];
        const float ws = add_rn(add_rn(add_rn(add_rn(wv[0], wv[1]), add_rn(wv[2], wv[3])),
                                             add_rn(add_rn(wv[4], wv[5]), add_rn(wv[6], wv[7]))), wv[8]);
        double cents = ps / (double)ws;
        if (best <= thred) cents = 0.0;
        double hz = 10.0 * pow(2.0, cents / 1200.0);
        if (hz == 10.0) hz = 0.0;
        f0[f] = hz;
    }
}

// _resize_f0 (np.interp with NaN for unvoiced, f0.py:68-78) -> _interpolate_f0 (f0.py:31-66, sequential, with its
// aliasing quirks) -> post_process (gen.py:18,34-41).  Single block; src [n] fp64 -> pitch [p_len] int64, pitchf [p_len] fp32.
// Work arrays a [n] and r [p_len] (fp64): dynamic LDS when they fit (<= 20480 frames), otherwise the caller's global
// buffers ga / gr -- a whole file's f0 is computed in ONE call by the reference (pipeline.py:260-266; a 3-minute song is
// ~36k frames), so there must be no length limit.  ga may alias src (in-place NaN marking); gr may be the `pitch` output
// buffer itself (same size: the last loop reads r[i] and writes pitch[i] from the same thread).
// The body: one block's whole chain for one sequence, work arrays a [n] (source with NaN for unvoiced) and r [p_len] given by the caller.
// Shared by k_f0_post and k_f0_post_ragged, so an item of a ragged call equals the single call on it bit for bit.
__device__ __forceinline__ void f0_post_block(const double* src, int n, int p_len, int do_resize, int do_interp, double key_mul,
                                              double mel_min, double mel_max, int64_t* pitch, float* __restrict__ pitchf, double* a,
                                              double* r) {
#pragma clang fp contract(off)
    const double NaN = __longlong_as_double(0x7ff8000000000000LL);
    if (do_resize) {
        for (int i = threadIdx.x; i < n; i += 256) {
            const double v = src[i];
            a[i] = v < 0.001 ? NaN : v;
        }
    }
    __syncthreads();
    if (do_resize) {
        // np.interp(np.arange(0, n*p_len, n) / p_len, np.arange(n), source); then nan_to_num
        for (int i = threadIdx.x; i < p_len; i += 256) {
            const double x = (double)((long long)i * n) / (double)p_len;
            double res;
            if (x > (double)(n - 1)) {
                res = a[n - 1];  // right = fp[-1]
            } else {
                const int j = (int)floor(x);
                if (j == n - 1 || (double)j == x) {
                    res = a[j];
                } else {
                    const double slope = (a[j + 1] - a[j]) / ((double)(j + 1) - (double)j);
                    res = slope * (x - (double)j) + a[j];
                    if (isnan(res)) {  // "if we get nan in one direction, try the other" (numpy arr_interp)
                        res = slope * (x - (double)(j + 1)) + a[j + 1];
                        if (isnan(res) && a[j] == a[j + 1]) res = a[j];
                    }
                }
            }
            if (isnan(res)) res = 0.0;  // np.nan_to_num (values are finite or NaN here)
            r[i] = res;
        }
    } else {
        for (int i = threadIdx.x; i < p_len; i += 256) r[i] = i < n ? src[i] : 0.0;
    }
    __syncthreads();
    if (do_interp && threadIdx.x == 0) {
        // sequential emulation of F0Predictor._interpolate_f0 (ip_data aliases data).  Filled gaps become positive, so the
        // scan jumps over them; a trailing fill ends the pass (re-running it cannot change anything).
        const int N = p_len;
        double last = 0.0;
        int i = 0;
        while (i < N) {
            if (r[i] <= 0.0) {
                int j = i + 1;
                for (int jj = i + 1; jj < N; ++jj) {
                    j = jj;
                    if (r[jj] > 0.0) break;
                }
                if (j < N - 1) {
                    if (last > 0.0) {
                        const double step = (r[j] - r[i - 1]) / (double)(j - i);
                        for (int k = i; k < j; ++k) r[k] = r[i - 1] + step * (double)(k - i + 1);
                    } else {
                        for (int k = i; k < j; ++k) r[k] = r[j];
                    }
                    last = r[j - 1] > 0.0 ? r[j - 1] : last;  // what the per-element pass would have left behind
                    i = j;
                } else {
                    for (int k = i; k < N; ++k) r[k] = last;
                    break;
                }
            } else {
                last = r[i];
                ++i;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < p_len; i += 256) {
        const double f = r[i] * key_mul;  // np.multiply(f0, pow(2, f0_up_key / 12))   (read BEFORE pitch[i] is written: gr may alias it)
        double mel = 1127.0 * log(1.0 + f / 700.0);
        if (mel > 0.0) mel = (mel - mel_min) * 254.0 / (mel_max - mel_min) + 1.0;
        if (mel <= 1.0) mel = 1.0;
        if (mel > 255.0) mel = 255.0;
        pitch[i] = (int64_t)rint(mel);
        pitchf[i] = (float)f;
    }
}

static __global__ void __launch_bounds__(256) k_f0_post(const double* src, int n, int p_len, int do_resize,
                                                        int do_interp, double key_mul, double mel_min, double mel_max,
                                                        int64_t* pitch, float* __restrict__ pitchf, double* ga, double* gr) {
    extern __shared__ double sm[];
    f0_post_block(src, n, p_len, do_resize, do_interp, key_mul, mel_min, mel_max, pitch, pitchf, ga ? ga : sm, gr ? gr : sm + n);
}

// k_f0_post (resize + interpolate) for MANY sequences, one block per item: item blockIdx.x's descriptor says where its decoded rows start in
// f0 [R] (the packed output of ONE k_rmvpe_decode over all rows), how many there are, its p_len, its factor and where its results go in the
// packed pitch / pitchf [out_len].  use_global == 0: work arrays in dynamic LDS (lds_doubles of it, sized by the host for the largest
// item); else every item works in global memory as the single call does beyond 10240 frames: its own slice of f0 in place and its own
// slice of `pitch` as the r array.  The descriptors live on the device; the host has checked its copy, and an item whose device
// descriptor leaves the buffers all the same is skipped rather than followed out of bounds.
static __global__ void __launch_bounds__(256) k_f0_post_ragged(double* f0, int64_t R, const rvcmi_f0_row* __restrict__ desc, int use_global,
                                                               int lds_doubles, double mel_min, double mel_max, int64_t* pitch,
                                                               float* __restrict__ pitchf, int64_t out_len) {
    extern __shared__ double sm[];
    const rvcmi_f0_row d = desc[blockIdx.x];
    if (d.n < 1 || d.p_len < 1 || d.first_row < 0 || (int64_t)d.first_row + d.n > R || d.out_off < 0 || d.out_off + d.p_len > out_len) return;
    if (!use_global && (int64_t)d.n + d.p_len > lds_doubles) return;
    double* src = f0 + d.first_row;
    int64_t* p = pitch + d.out_off;
    f0_post_block(src, d.n, d.p_len, 1, 1, d.key_mul, mel_min, mel_max, p, pitchf + d.out_off, use_global ? src : sm,
                  use_global ? reinterpret_cast<double*>(p) : sm + d.n);
}

// audio_max = abs(audio).max() / 0.99; max_int16 = 32768; if audio_max > 1: max_int16 /= audio_max; audio *= max_int16
// (pipeline.py:355-359).  Two launches: per-block maxima, then scale (every block re-reduces the partials).
static __global__ void __launch_bounds__(256) k_absmax_partial(const float* __restrict__ x, int64_t n, float* __restrict__ part) {
    __shared__ float red[256];
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) m = fmaxf(m, fabsf(x[i]));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
static __global__ void __launch_bounds__(256) k_scale_int16_range(float* __restrict__ x, int64_t n, const float* __restrict__ part,
                                                                  int nparts) {
#pragma clang fp contract(off)
    __shared__ float red[256];
    float m = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) m = fmaxf(m, part[i]);
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    // numpy: float32 max / python float 0.99 -> float64; 32768 / that -> float64; multiply casts the scalar to float32
    const double amax = (double)red[0] / 0.99;
    double mi = 32768.0;
    if (amax > 1.0) mi /= amax;
    const float sc = (float)mi;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] = mul_rn(x[i], sc);
}

// SOLA (gui.py:1057-1090, "SOLA algorithm from DDSP-SVC"): find the offset in [0, Ls] at which the new chunk best continues
// the previous chunk's tail (normalised cross-correlation), cut there, cross-fade Lb samples, keep the next tail.
//   cor_nom[o] = sum_i x[o+i] * buf[i],  cor_den[o] = sqrt(sum_i x[o+i]^2 + 1e-8),  offset = argmax(cor_nom / cor_den)
//   y = x[offset:];  y[:Lb] = y[:Lb] * fade_in + buf * fade_out;  buf <- y[block : block + Lb];  out <- y[:block]
// The two sums are accumulated in fp64 and rounded once (the reference's F.conv1d leaves the fp32 summation order to the
// backend); everything after the argmax is the reference's fp32 expression, unfused.  One block.
//
// The offset search of k_sola_batch and k_sola_search_batch (256 threads): xs [Lb + Ls] and bs [Lb] staged in LDS, rv / ri 256
// entries of LDS for the block's argmax.  Every thread gets the offset.
__device__ __forceinline__ int sola_search(const float* xs, const float* bs, int Lb, int Ls, float* rv, int* ri) {
#pragma clang fp contract(off)
    float best = -INFINITY;
    int bo = 0;
    for (int o = threadIdx.x; o <= Ls; o += 256) {
        double nom = 0.0, en = 0.0;
        for (int i = 0; i < Lb; ++i) {
            const double v = (double)xs[o + i];
            nom += v * (double)bs[i];
            en += v * v;
        }
        const float r = div_rn((float)nom, sqrtf(add_rn((float)en, 1e-8f)));
        if (r > best) {
            best = r;
            bo = o;
        }
    }
    rv[threadIdx.x] = best;
    ri[threadIdx.x] = bo;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
            const float ov = rv[threadIdx.x + s];
            const int oi = ri[threadIdx.x + s];
            if (ov > rv[threadIdx.x] || (ov == rv[threadIdx.x] && oi < ri[threadIdx.x])) {  // torch.argmax: first maximum
                rv[threadIdx.x] = ov;
                ri[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    return ri[0];
}

// One block's whole stitch of one signal (sl: the dynamic LDS, 2 Lb + Ls floats): the body of k_sola_batch.
__device__ __forceinline__ void sola_block(const float* __restrict__ x, float* __restrict__ buf, int Lb, int Ls,
                                           const float* __restrict__ fade_in, const float* __restrict__ fade_out, int block,
                                           float* __restrict__ out, int* __restrict__ offset_out, float* sl, float* rv, int* ri) {
#pragma clang fp contract(off)
    float* xs = sl;             // [Lb + Ls]
    float* bs = sl + Lb + Ls;   // [Lb]
    for (int i = threadIdx.x; i < Lb + Ls; i += 256) xs[i] = x[i];
    for (int i = threadIdx.x; i < Lb; i += 256) bs[i] = buf[i];
    __syncthreads();
    const int off = sola_search(xs, bs, Lb, Ls, rv, ri);
    if (threadIdx.x == 0 && offset_out) *offset_out = off;
    auto y = [&](int p) {  // the shifted, cross-faded chunk at position p
        const float v = x[off + p];
        return p < Lb ? add_rn(mul_rn(v, fade_in[p]), mul_rn(bs[p], fade_out[p])) : v;
    };
    for (int i = threadIdx.x; i < block; i += 256) out[i] = y(i);
    for (int i = threadIdx.x; i < Lb; i += 256) buf[i] = y(block + i);  // old tail is in LDS: safe to overwrite
}

// A bank of S signals, one block per session (blockIdx.x); every per-session array has a row stride in elements (a row may be a
// slice of a longer rolling buffer).  fade_in / fade_out are shared.  offset_out [S] (optional).  A single stream is S = 1 with
// strides equal to the row lengths -- here and in every _batch kernel below; there is no other form.
static __global__ void __launch_bounds__(256) k_sola_batch(const float* __restrict__ x, int64_t x_stride, float* __restrict__ buf,
                                                           int64_t buf_stride, int Lb, int Ls, const float* __restrict__ fade_in,
                                                           const float* __restrict__ fade_out, int block, float* __restrict__ out,
                                                           int64_t out_stride, int* __restrict__ offset_out) {
    extern __shared__ float sl[];
    __shared__ float rv[256];
    __shared__ int ri[256];
    const int64_t s = blockIdx.x;
    sola_block(x + s * x_stride, buf + s * buf_stride, Lb, Ls, fade_in, fade_out, block, out + s * out_stride,
               offset_out ? offset_out + s : nullptr, sl, rv, ri);
}

// ------------------------------------------------------------------------------------------------
// The GUI's use_pv branch (gui.py:1076-1087): the same search, then x[off : off + Lb] is cross-faded with the previous tail by
// the phase vocoder below instead of the sin^2 fade.  Four launches: search -> pv spectrum -> pv synthesis (into scratch) ->
// stitch; the offset stays in device memory between them.
__device__ __forceinline__ void sola_search_block(const float* __restrict__ x, const float* __restrict__ buf, int Lb, int Ls,
                                                  int* __restrict__ offset_out, float* sl, float* rv, int* ri) {
    float* xs = sl;             // [Lb + Ls]
    float* bs = sl + Lb + Ls;   // [Lb]
    for (int i = threadIdx.x; i < Lb + Ls; i += 256) xs[i] = x[i];
    for (int i = threadIdx.x; i < Lb; i += 256) bs[i] = buf[i];
    __syncthreads();
    const int off = sola_search(xs, bs, Lb, Ls, rv, ri);
    if (threadIdx.x == 0) *offset_out = off;
}

// One block per session (blockIdx.x), rows by stride; offset_out [S].
static __global__ void __launch_bounds__(256) k_sola_search_batch(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ buf,
                                                                  int64_t buf_stride, int Lb, int Ls, int* __restrict__ offset_out,
                                                                  int64_t off_stride) {
    extern __shared__ float sl[];
    __shared__ float rv[256];
    __shared__ int ri[256];
    const int64_t s = blockIdx.x;
    sola_search_block(x + s * x_stride, buf + s * buf_stride, Lb, Ls, offset_out + s * off_stride, sl, rv, ri);
}

// out <- y[:block], buf <- y[block : block + Lb] with y = x[off:], y[:Lb] = pv.  buf is not read here (the pv launches have
// consumed it), so any number of blocks may write it.
__device__ __forceinline__ void sola_pv_stitch_at(const float* __restrict__ x, const int* __restrict__ offset, const float* __restrict__ pv,
                                                  int Lb, int block, float* __restrict__ out, float* __restrict__ buf, int i) {
    if (i >= block + Lb) return;
    const int off = *offset;
    const float v = i < Lb ? pv[i] : x[off + i];
    if (i < block) out[i] = v;
    else buf[i - block] = v;
}

// Session blockIdx.y; pv and offset live in the session's slice of the scratch (strides in floats / ints).
static __global__ void __launch_bounds__(256) k_sola_pv_stitch_batch(const float* __restrict__ x, int64_t x_stride, const int* __restrict__ offset,
                                                                     int64_t off_stride, const float* __restrict__ pv, int64_t pv_stride, int Lb,
                                                                     int block, float* __restrict__ out, int64_t out_stride,
                                                                     float* __restrict__ buf, int64_t buf_stride) {
    const int64_t s = blockIdx.y;
    sola_pv_stitch_at(x + s * x_stride, offset + s * off_stride, pv + s * pv_stride, Lb, block, out + s * out_stride, buf + s * buf_stride,
                      blockIdx.x * 256 + threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// phase_vocoder(a, b, fade_out, fade_in) of gui.py:27-49, n = len(a) <= RVCMI_PV_MAX_N:
//   w = sqrt(fade_out * fade_in);  Fa, Fb = rfft(a * w), rfft(b * w)                     (nb = n/2 + 1 bins)
//   absab = |Fa| + |Fb|, doubled for 0 < k < n/2 (even n) / 0 < k (odd n)
//   d = angle(Fb) - angle(Fa);  d -= 2 pi floor(d / 2 / pi + 0.5)
//   out[t] = a[t] fade_out[t]^2 + b[t] fade_in[t]^2 + w[t] / n * sum_k absab[k] cos((2 pi k + d[k]) t / n + angle(Fa)[k])
// The synthesis is not an inverse DFT (d[k] t / n couples bin and sample): an O(n * nb) sum, 1.85 M terms at n = 1920.
// Spectrum and synthesis run in fp64 from the fp32 inputs (the reference's own fp32 run is less faithful to its formula:
// its w * t reaches ~6000 rad); the cosine is fp32 on an argument reduced exactly into [-pi, pi].
// A bin whose real and imaginary sums are both exactly zero has phase 0 (the reference's angle there depends on the signed
// zeros its FFT backend returns).
#define RVCMI_PV_MAX_N 4096

// Spectrum: one wave per bin (grid-strided), lanes over samples.  LDS: the twiddle table (cos, sin)(2 pi m / n) built with
// sincospi (the quarter points are exact) and the windowed inputs, 32 n bytes.  bins: absab [nb] | phia [nb] | d / n [nb].
// b_off (optional): b is read at b + *b_off (the SOLA offset, which never leaves the device).
// (bx, gx: the block's index and the block count over the bins of ONE signal -- blockIdx.x / gridDim.x)
__device__ __forceinline__ void pv_spectrum_block(const float* __restrict__ a, const float* __restrict__ b, const int* __restrict__ b_off,
                                                  const float* __restrict__ fade_out, const float* __restrict__ fade_in, int n,
                                                  double* __restrict__ bins, double* pv_sm, int bx, int gx) {
    double2* tw = reinterpret_cast<double2*>(pv_sm);   // [n]
    double2* xy = tw + n;                              // [n]: (a w, b w)
    const float* bp = b + (b_off ? *b_off : 0);
    const int nb = n / 2 + 1;
    for (int m = threadIdx.x; m < n; m += 256) {
        double s, c;
        sincospi((double)(2 * m) / (double)n, &s, &c);
        tw[m] = make_double2(c, s);
        const double w = sqrt((double)fade_out[m] * (double)fade_in[m]);
        xy[m] = make_double2((double)a[m] * w, (double)bp[m] * w);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int k = bx * 4 + (threadIdx.x >> 6); k < nb; k += gx * 4) {
        double ra = 0.0, ia = 0.0, rb = 0.0, ib = 0.0;
        int m = (k * lane) % n;              // (k * i) mod n, i = lane + 64 j   (k * i < 2^31 for n <= 4096)
        const int step = (k * 64) % n;
        for (int i = lane; i < n; i += 64) {
            const double2 t = tw[m], x = xy[i];
            ra += x.x * t.x;
            ia -= x.x * t.y;
            rb += x.y * t.x;
            ib -= x.y * t.y;
            m += step;
            if (m >= n) m -= n;
        }
        for (int o = 32; o >= 1; o >>= 1) {
            ra += __shfl_xor(ra, o, 64);
            ia += __shfl_xor(ia, o, 64);
            rb += __shfl_xor(rb, o, 64);
            ib += __shfl_xor(ib, o, 64);
        }
        if (lane == 0) {
            double ab = sqrt(ra * ra + ia * ia) + sqrt(rb * rb + ib * ib);
            if (k >= 1 && (k < nb - 1 || (n & 1))) ab *= 2.0;
            const double pa = (ra == 0.0 && ia == 0.0) ? 0.0 : atan2(ia, ra);
            const double pb = (rb == 0.0 && ib == 0.0) ? 0.0 : atan2(ib, rb);
            double d = pb - pa;
            d = d - 2.0 * M_PI * floor(d / 2.0 / M_PI + 0.5);
            bins[k] = ab;
            bins[nb + k] = pa;
            bins[2 * nb + k] = d / (double)n;
        }
    }
}

// Session blockIdx.y: a / b rows by stride, b_off and bins in the session's slice of the scratch (strides in ints / doubles).
// The stand-alone vocoder has no offset: b_off = nullptr with off_stride = 0 at S = 1 (nullptr + 0; the body reads offset 0).
static __global__ void __launch_bounds__(256) k_pv_spectrum_batch(const float* __restrict__ a, int64_t a_stride, const float* __restrict__ b,
                                                                  int64_t b_stride, const int* __restrict__ b_off, int64_t off_stride,
                                                                  const float* __restrict__ fade_out, const float* __restrict__ fade_in, int n,
                                                                  double* __restrict__ bins, int64_t bins_stride) {
    extern __shared__ __attribute__((aligned(16))) double pv_sm[];
    const int64_t s = blockIdx.y;
    pv_spectrum_block(a + s * a_stride, b + s * b_stride, b_off + s * off_stride, fade_out, fade_in, n, bins + s * bins_stride, pv_sm,
                      blockIdx.x, gridDim.x);
}

// Synthesis: a block owns 64 consecutive samples (one per lane); its 16 waves split the bins, staged in LDS, and their
// partial sums are added in a fixed order.  Argument per term: 2 pi ((k t) mod n) / n + (d[k] / n) t + phia[k] in fp64,
// reduced by 2 pi rint(arg / 2 pi) into [-pi, pi] before the fp32 cosine; products and sums in fp64, one rounding at the end.
__device__ __forceinline__ void pv_synth_block(const float* __restrict__ a, const float* __restrict__ b, const int* __restrict__ b_off,
                                               const float* __restrict__ fade_out, const float* __restrict__ fade_in, int n,
                                               const double* __restrict__ bins, float* __restrict__ out, double* pv_sm, int bx) {
    const int nb = n / 2 + 1;
    double* ab = pv_sm;             // [nb]
    double* ph = ab + nb;           // [nb]
    double* dn = ph + nb;           // [nb]
    double* red = dn + nb;          // [16][64]
    for (int i = threadIdx.x; i < 3 * nb; i += 1024) pv_sm[i] = bins[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int t = bx * 64 + lane;
    const int tt = t < n ? t : 0;
    const double two_pi = 2.0 * M_PI, inv_two_pi = 1.0 / (2.0 * M_PI), w_n = 2.0 * M_PI / (double)n, td = (double)tt;
    int m = (wv * tt) % n;                  // (k * t) mod n for k = wv + 16 j
    const int step = (16 * tt) % n;
    double acc = 0.0;
    for (int k = wv; k < nb; k += 16) {
        double arg = (double)m * w_n + (dn[k] * td + ph[k]);
        arg -= two_pi * rint(arg * inv_two_pi);
        acc += ab[k] * (double)cosf((float)arg);
        m += step;
        if (m >= n) m -= n;
    }
    red[wv * 64 + lane] = acc;
    __syncthreads();
    if (wv == 0 && t < n) {
        double s = 0.0;
        for (int j = 0; j < 16; ++j) s += red[j * 64 + lane];
        const float* bp = b + (b_off ? *b_off : 0);
        const double fo = (double)fade_out[t], fi = (double)fade_in[t];
        const double w = sqrt(fo * fi);
        out[t] = (float)(((double)a[t] * (fo * fo) + (double)bp[t] * (fi * fi)) + s * w / (double)n);
    }
}

static __global__ void __launch_bounds__(1024) k_pv_synth_batch(const float* __restrict__ a, int64_t a_stride, const float* __restrict__ b,
                                                                int64_t b_stride, const int* __restrict__ b_off, int64_t off_stride,
                                                                const float* __restrict__ fade_out, const float* __restrict__ fade_in, int n,
                                                                const double* __restrict__ bins, int64_t bins_stride, float* __restrict__ out,
                                                                int64_t out_stride) {
    extern __shared__ __attribute__((aligned(16))) double pv_sm[];
    const int64_t s = blockIdx.y;
    pv_synth_block(a + s * a_stride, b + s * b_stride, b_off + s * off_stride, fade_out, fade_in, n, bins + s * bins_stride,
                   out + s * out_stride, pv_sm, blockIdx.x);
}

// ------------------------------------------------------------------------------------------------
// The realtime GUI's envelope mix (gui.py:1023-1056), in place on wav [n]:
//   rms1, rms2 = librosa.feature.rms(input[:n] / wav, frame_length = 4 zc, hop_length = zc)   (k_frame_rms_batch below)
//   both -> F.interpolate(linear, align_corners=True, size=n+1)[:-1];  rms2 = max(rms2, 1e-3);
//   wav *= pow(rms1 / rms2, float32(1 - rate))
// The interpolation is torch's CPU kernel: scale = (in-1)/(out-1) in fp32, src = scale * o, floor, clamp.
__device__ __forceinline__ float interp_linear_ac(const float* __restrict__ r, int nin, int64_t nout, int64_t o) {
#pragma clang fp contract(off)
    if ((int64_t)nin == nout) return r[o];
    const float scale = nout > 1 ? div_rn((float)(nin - 1), (float)(nout - 1)) : 0.f;
    const float src = mul_rn(scale, (float)o);
    int i0 = (int)floorf(src);
    if (i0 > nin - 1) i0 = nin - 1;
    const int i1 = i0 + (i0 < nin - 1 ? 1 : 0);
    const float l1 = fminf(fmaxf(sub_rn(src, (float)i0), 0.f), 1.f);
    const float l0 = sub_rn(1.f, l1);
    return add_rn(mul_rn(l0, r[i0]), mul_rn(l1, r[i1]));
}

__device__ __forceinline__ void envelope_mix_at(float* __restrict__ wav, int64_t n, const float* __restrict__ rms1,
                                                const float* __restrict__ rms2, int nf, float e, int64_t t) {
    if (t >= n) return;
    const float r1 = interp_linear_ac(rms1, nf, n + 1, t);
    const float r2 = fmaxf(interp_linear_ac(rms2, nf, n + 1, t), 1e-3f);
    wav[t] = mul_rn(wav[t], powf(div_rn(r1, r2), e));
}

// Session blockIdx.y: wav rows by stride; rms [S][2][nf] (the session's two envelopes side by side).
static __global__ void __launch_bounds__(256) k_envelope_mix_batch(float* __restrict__ wav, int64_t wav_stride, int64_t n,
                                                                   const float* __restrict__ rms, int nf, float e) {
    const int64_t s = blockIdx.y;
    const float* r = rms + s * 2 * nf;
    envelope_mix_at(wav + s * wav_stride, n, r, r + nf, nf, e, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// ------------------------------------------------------------------------------------------------
// change_rms (infer/modules/vc/pipeline.py:26-46): the output's loudness envelope mixed with the input's.
//   rms_i = librosa.feature.rms(y, frame_length = sr//2*2, hop_length = sr//2)   (centred frames, zero padding -- the
//           default of the librosa >= 0.10.2 the reference requires), one point per half second;
//   both envelopes linearly interpolated to len(data2) (F.interpolate, align_corners=False); rms2 = max(rms2, 1e-6);
//   data2 *= rms1^(1-rate) * rms2^(rate-1).
// The frame energy is accumulated in fp64 (numpy sums the float32 squares in float32; its summation order for this strided
// view is not pinned by anything in the reference, see oracle/glue_oracle.py:change_rms) and rounded to fp32 before the sqrt.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void frame_rms_block(const float* __restrict__ y, int64_t n, int frame, int hop, int nframes,
                                                float* __restrict__ rms, double* red, int f) {
    if (f >= nframes) return;
    const int64_t lo = (int64_t)f * hop - frame / 2;
    double acc = 0.0;
    for (int i = threadIdx.x; i < frame; i += 256) {
        const int64_t t = lo + i;
        if (t >= 0 && t < n) {
            const float v = y[t];
            acc += (double)mul_rn(v, v);  // abs2 in float32, like librosa's util.abs2(dtype=float32)
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s2 = 128; s2 >= 1; s2 >>= 1) {
        if ((int)threadIdx.x < s2) red[threadIdx.x] += red[threadIdx.x + s2];
        __syncthreads();
    }
    if (threadIdx.x == 0) rms[f] = sqrtf((float)(red[0] / (double)frame));
}

// Session blockIdx.y: y rows by stride, rms rows by rms_stride floats.
static __global__ void __launch_bounds__(256) k_frame_rms_batch(const float* __restrict__ y, int64_t y_stride, int64_t n, int frame, int hop,
                                                                int nframes, float* __restrict__ rms, int64_t rms_stride) {
    __shared__ double red[256];
    const int64_t s = blockIdx.y;
    frame_rms_block(y + s * y_stride, n, frame, hop, nframes, rms + s * rms_stride, red, blockIdx.x);
}

// The same for the sessions that are on (Sess: rvcmi_session_mix or rvcmi_session_gate, on the device); the blocks of the others leave
// before the body, uniformly per block, and write nothing.
template <typename Sess>
static __global__ void __launch_bounds__(256) k_frame_rms_sessions(const float* __restrict__ y, int64_t y_stride, int64_t n, int frame, int hop,
                                                                   int nframes, float* __restrict__ rms, int64_t rms_stride,
                                                                   const Sess* __restrict__ sess) {
    __shared__ double red[256];
    const int64_t s = blockIdx.y;
    if (!sess[s].on) return;
    frame_rms_block(y + s * y_stride, n, frame, hop, nframes, rms + s * rms_stride, red, blockIdx.x);
}

// k_envelope_mix_batch with the exponent per session; a session that is off keeps its row.
static __global__ void __launch_bounds__(256) k_envelope_mix_sessions(float* __restrict__ wav, int64_t wav_stride, int64_t n,
                                                                      const float* __restrict__ rms, int nf,
                                                                      const rvcmi_session_mix* __restrict__ sess) {
    const int64_t s = blockIdx.y;
    const rvcmi_session_mix c = sess[s];
    if (!c.on) return;
    const float* r = rms + s * 2 * nf;
    envelope_mix_at(wav + s * wav_stride, n, r, r + nf, nf, c.exponent, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

__device__ __forceinline__ float interp_linear_1d(const float* __restrict__ r, int nin, int64_t nout, int64_t o) {
    // F.interpolate(mode="linear", align_corners=False): src = scale*(o+0.5)-0.5 clamped at 0, scale = nin/nout (fp32)
    const float scale = (float)nin / (float)nout;
    float src = sub_rn(mul_rn(scale, add_rn((float)o, 0.5f)), 0.5f);
    if (src < 0.f) src = 0.f;
    int i0 = (int)src;
    if (i0 > nin - 1) i0 = nin - 1;
    const int i1 = i0 + (i0 < nin - 1 ? 1 : 0);
    const float l1 = sub_rn(src, (float)i0);
    const float l0 = sub_rn(1.f, l1);
    return add_rn(mul_rn(l0, r[i0]), mul_rn(l1, r[i1]));
}

static __global__ void __launch_bounds__(256) k_change_rms(float* __restrict__ data2, int64_t n2, const float* __restrict__ rms1, int nf1,
                                                           const float* __restrict__ rms2, int nf2, float e1, float e2) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n2) return;
    const float r1 = interp_linear_1d(rms1, nf1, n2, t);
    float r2 = interp_linear_1d(rms2, nf2, n2, t);
    r2 = fmaxf(r2, 1e-6f);
    data2[t] = mul_rn(data2[t], mul_rn(powf(r1, e1), powf(r2, e2)));
}

// ------------------------------------------------------------------------------------------------
// The realtime GUI's input gate (gui.py:950-963) for a bank, session blockIdx.y.  Three launches:
//   k_gate_stage_batch     x = rms_buffer | block  (4 zc + blk samples) into the session's staging row
//   k_frame_rms_batch      the frame RMS of x, frame 4 zc, hop zc (all blk / zc + 5 centred frames; the gate reads frames 2 ..)
//   k_input_gate_batch     out[j] = x[2 zc + j] for j < blk + 2 zc, zero where frame (j + zc / 2) / zc is quiet; rms_buffer <- x[-4 zc:]
// librosa.amplitude_to_db(rms)[i] < threhold is decided WITHOUT a logarithm: it is monotone in the float32 RMS, so the host derives the
// two float32 cutoffs (realtime.input_gate_cutoffs) and frame i is quiet iff rms[i] < cut_a and max(rms) < cut_b (the 80 dB clip under the
// loudest frame); a NaN among the frames makes no frame quiet, as numpy's max propagates it.
static __global__ void __launch_bounds__(256) k_gate_stage_batch(const float* __restrict__ block, int64_t block_stride,
                                                                 const float* __restrict__ rbuf, int64_t rbuf_stride, int zc, int blk,
                                                                 float* __restrict__ x, int64_t x_stride) {
    const int64_t s = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 4 * zc + blk) return;
    x[s * x_stride + i] = i < 4 * zc ? rbuf[s * rbuf_stride + i] : block[s * block_stride + (i - 4 * zc)];
}

// The gate of ONE session (the body of k_input_gate_batch and k_input_gate_sessions; every thread of the block calls it): xs its staged x,
// r its gate frames (the frame RMS from frame 2 on), dst / rbuf its rows; red [256] and has_nan in LDS.
__device__ __forceinline__ void input_gate_block(const float* __restrict__ xs, const float* __restrict__ r, int zc, int blk, float cut_a,
                                                 float cut_b, float* __restrict__ dst, float* __restrict__ rbuf, float* red, int* has_nan) {
    const int nf = blk / zc + 3;
    if (threadIdx.x == 0) *has_nan = 0;
    __syncthreads();
    float m = 0.f;  // an RMS is never negative
    int nan = 0;
    for (int i = threadIdx.x; i < nf; i += 256) {
        const float v = r[i];
        nan |= v != v ? 1 : 0;
        m = fmaxf(m, v);
    }
    red[threadIdx.x] = m;
    if (nan) atomicOr(has_nan, 1);
    __syncthreads();
    for (int s2 = 128; s2 >= 1; s2 >>= 1) {
        if ((int)threadIdx.x < s2) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s2]);
        __syncthreads();
    }
    const bool may = !*has_nan && red[0] < cut_b;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < blk + 2 * zc) {
        const bool quiet = may && r[(j + zc / 2) / zc] < cut_a;
        dst[j] = quiet ? 0.f : xs[2 * zc + j];
    }
    if (j < 4 * zc) rbuf[j] = xs[blk + j];
}

// rms: the session's blk / zc + 5 frames as k_frame_rms_batch wrote them (rms_stride floats apart); the gate's frame i is rms[2 + i].
static __global__ void __launch_bounds__(256) k_input_gate_batch(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ rms,
                                                                 int64_t rms_stride, int zc, int blk, float cut_a, float cut_b,
                                                                 float* __restrict__ dst, int64_t dst_stride, float* __restrict__ rbuf,
                                                                 int64_t rbuf_stride) {
    __shared__ float red[256];
    __shared__ int has_nan;
    const int64_t s = blockIdx.y;
    input_gate_block(x + s * x_stride, rms + s * rms_stride + 2, zc, blk, cut_a, cut_b, dst + s * dst_stride, rbuf + s * rbuf_stride, red,
                     &has_nan);
}

// The stage and the gate with the cutoffs per session (rvcmi_glue_input_gate_sessions).  A session that is off is not staged; the gate
// kernel copies its raw block to the last blk samples of its dst row and touches neither the 2 zc samples in front nor its rms_buffer row
// (the stream that does not call the gate).  Both branches are uniform per block.
static __global__ void __launch_bounds__(256) k_gate_stage_sessions(const float* __restrict__ block, int64_t block_stride,
                                                                    const float* __restrict__ rbuf, int64_t rbuf_stride, int zc, int blk,
                                                                    float* __restrict__ x, int64_t x_stride,
                                                                    const rvcmi_session_gate* __restrict__ sess) {
    const int64_t s = blockIdx.y;
    if (!sess[s].on) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 4 * zc + blk) return;
    x[s * x_stride + i] = i < 4 * zc ? rbuf[s * rbuf_stride + i] : block[s * block_stride + (i - 4 * zc)];
}

static __global__ void __launch_bounds__(256) k_input_gate_sessions(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ rms,
                                                                    int64_t rms_stride, int zc, int blk,
                                                                    const rvcmi_session_gate* __restrict__ sess,
                                                                    const float* __restrict__ block, int64_t block_stride,
                                                                    float* __restrict__ dst, int64_t dst_stride, float* __restrict__ rbuf,
                                                                    int64_t rbuf_stride) {
    __shared__ float red[256];
    __shared__ int has_nan;
    const int64_t s = blockIdx.y;
    const rvcmi_session_gate c = sess[s];
    if (!c.on) {
        const int j = blockIdx.x * 256 + threadIdx.x;
        if (j < blk) dst[s * dst_stride + 2 * zc + j] = block[s * block_stride + j];
        return;
    }
    input_gate_block(x + s * x_stride, rms + s * rms_stride + 2, zc, blk, c.cut_a, c.cut_b, dst + s * dst_stride, rbuf + s * rbuf_stride, red,
                     &has_nan);
}

// Polyphase FIR resampling as torchaudio.transforms.Resample applies it (rtrvc.py:248-259: the formant-shifted block comes out
// of the generator at upp_res samples per 10 ms and is brought back to tgt_sr/100): out[j*nf + p] = sum_k w[p][k] * xpad[j*of + k],
// xpad = x padded with `width` zeros in front (and zeros behind), k < K = 2*width + of.  One thread per output sample, fp32,
// taps added in ascending k (torchaudio's F.conv1d leaves the order to the backend).  HBM/latency-bound: n_out * K MACs,
// K ~ 430 for the 423 -> 400 ratio of a +1 semitone shift at 40 kHz; the 400 x 437 coefficient table stays in L2.
__device__ __forceinline__ void resample_poly_at(const float* __restrict__ x, int64_t n, const float* __restrict__ w, int of, int nf, int K,
                                                 int width, float* __restrict__ out, int64_t n_out, int64_t i) {
    if (i >= n_out) return;
    const int64_t j = i / nf;
    const int p = (int)(i - j * nf);
    const float* wp = w + (size_t)p * K;
    const int64_t base = j * of - width;  // index of tap 0 in the unpadded signal
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const int64_t t = base + k;
        const float xv = (t >= 0 && t < n) ? x[t] : 0.f;
        acc = fmaf(wp[k], xv, acc);
    }
    out[i] = acc;
}

// Session blockIdx.y: x and out rows by stride, one coefficient table.
static __global__ void __launch_bounds__(256) k_resample_poly_batch(const float* __restrict__ x, int64_t x_stride, int64_t n,
                                                                    const float* __restrict__ w, int of, int nf, int K, int width,
                                                                    float* __restrict__ out, int64_t out_stride, int64_t n_out) {
    const int64_t s = blockIdx.y;
    resample_poly_at(x + s * x_stride, n, w, of, nf, K, width, out + s * out_stride, n_out, (int64_t)blockIdx.x * 256 + threadIdx.x);
}

// Session blockIdx.y resamples with ITS OWN ratio (the bank's formant shift per session, rtrvc.py:248-259): row s's table starts at
// w + desc[s].w_off, its reduced rates / K / width and the samples n it reads are the descriptor's; the output is dense, n_out per row.
// A row whose descriptor says of == nf is the head copy of its input (the reference does not resample it).  Same arithmetic per sample
// as k_resample_poly_batch (resample_poly_at), so a row equals that kernel with the row's table bit for bit.
static __global__ void __launch_bounds__(256) k_resample_poly_ragged(const float* __restrict__ x, int64_t x_stride, const float* __restrict__ w,
                                                                     int64_t w_floats, const rvcmi_resample_row* __restrict__ desc, int64_t n_max,
                                                                     float* __restrict__ out, int64_t out_stride, int64_t n_out) {
    const int64_t s = blockIdx.y;
    const rvcmi_resample_row d = desc[s];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = d.n < 0 ? 0 : (d.n < n_max ? d.n : n_max);  // (never past the n_max samples the host checked the row stride for)
    const bool copy = d.orig == d.new_;
    // a descriptor that does not describe a table inside the buffer (the host cannot read it: it lives on the device) yields a row of zeros
    const bool ok = copy || (d.orig >= 1 && d.new_ >= 1 && d.K >= 1 && d.width >= 0 && d.w_off >= 0 && d.w_off + (int64_t)d.new_ * d.K <= w_floats);
    if (copy || !ok) {
        if (i < n_out) out[s * out_stride + i] = (ok && i < n) ? x[s * x_stride + i] : 0.f;
        return;
    }
    resample_poly_at(x + s * x_stride, n, w + d.w_off, d.orig, d.new_, d.K, d.width, out + s * out_stride, n_out, i);
}

}  // namespace rvcmi
