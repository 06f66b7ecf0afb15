// scipy.signal.filtfilt(b, a, x) with scipy's defaults (padtype="odd", padlen = 3 max(len(a), len(b)), method="pad") on the device:
// the reference's input preparation (infer/modules/vc/pipeline.py:23,221: a 5th-order Butterworth high-pass at 48 Hz, fp64).
//
//   ext = odd extension of x by padlen samples at each end            (2 x[0] - x[padlen..1], x, 2 x[n-1] - x[n-2..n-1-padlen])
//   y1  = lfilter(b, a, ext,      zi = lfilter_zi(b, a) * ext[0])
//   y2  = lfilter(b, a, y1[::-1], zi = lfilter_zi(b, a) * y1[-1])
//   out = y2[::-1][padlen : -padlen]
//
// lfilter is direct form II transposed, every operation rounded on its own in fp64:
//
//   y = b0 x + z0;   z_k = (b_{k+1} x + z_{k+1}) - a_{k+1} y   (k < order - 1);   z_{order-1} = b_order x - a_order y
//
// A recurrence is one dependent chain (add, mul, sub per sample), and the pipeline's filter has five poles of radius 0.981 .. 0.994:
// ANY other order of operations ends about 5e-8 from scipy, and the filter state cannot be carried across blocks in direct-form
// coordinates (powers of the companion matrix overflow long before they decay).  So no state is transferred at all.  One thread
// ("lane") produces FILT_LANE consecutive outputs of a pass; it starts `warm` samples earlier from the steady state of a constant
// input, zi * in[start], runs the recurrence over the warm-up without storing, and by the time it reaches its own outputs the wrong
// start has decayed below 2^-64 of itself (the wrapper derives `warm` from the eigen-decomposition of the companion matrix:
// cond(V) rho^warm < 2^-64).  A lane whose warm-up would begin before the signal begins at sample 0 with zi * in[0] -- scipy's own
// initial state -- and therefore computes scipy's bits: an input with n + 2 padlen <= warm + FILT_LANE is BIT-equal to scipy,
// longer ones carry the rounding noise of an independent fp64 evaluation (the same level as scipy's own deviation from the exact
// result).  The lanes of a pass are independent, so a pass takes about warm + FILT_LANE chain steps whatever
// the length of the file, and a ragged batch is one launch per pass.
//
// The odd extension and the time reversal of the second pass are index arithmetic: no padded or reversed copy exists.  The
// extension is evaluated in the input's own type (scipy's odd_ext runs on the float32 array when x is float32) and then widened.
// The backward pass can also write np.pad(out, pad, mode="reflect") next to out: each lane stores its value at the one or two
// mirrored positions as well, a pure copy.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

namespace rvcmi {

constexpr int RVCMI_FILT_MAX_ORDER = 8;
constexpr int FILT_LANE = 1024;   // outputs per lane; `warm` is a multiple of it
constexpr int FILT_WAVE = 64;     // one wave per block: the few hundred lanes of a file spread over as many SIMDs as possible
constexpr int64_t RVCMI_FILT_MAX_LEN = (int64_t)1 << 28;  // samples per item (4.6 hours at 16 kHz): bounds the grid and the 2 GiB of scratch an item takes
constexpr int FILT_UNROLL = 8;    // samples per prefetch group: the next group's loads are in flight while this one's chain runs

struct FiltCoef {  // a[0] == 1 (the wrapper normalises as lfilter does); entries above `order` are unused
    double b[RVCMI_FILT_MAX_ORDER + 1];
    double a[RVCMI_FILT_MAX_ORDER + 1];
    double zi[RVCMI_FILT_MAX_ORDER];
};

// Single-rounded fp64 operations (exact_fp.hpp explains why the pragma has to sit inside the helper): a contraction of
// b x + z or of (..) - a y into v_fma_f64 changes the rounding trajectory of the whole file.
__device__ __forceinline__ double dmul_rn(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double dadd_rn(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double dsub_rn(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float odd_reflect(float edge, float v) {
#pragma clang fp contract(off)
    return 2.0f * edge - v;
}
__device__ __forceinline__ double odd_reflect(double edge, double v) {
#pragma clang fp contract(off)
    return 2.0 * edge - v;
}

// ext[k], k in [0, n + 2 padlen), in the input's type; the entry point guarantees n > padlen, so every index below is inside [0, n)
template <typename T>
__device__ __forceinline__ T filt_ext(const T* __restrict__ x, int64_t n, int padlen, int64_t k) {
    const int64_t i = k - padlen;
    if (i < 0) return odd_reflect(x[0], x[-i]);
    if (i >= n) return odd_reflect(x[n - 1], x[2 * n - 2 - i]);
    return x[i];
}

// One pass.  grid (ceil(lanes of the longest item / 64), B), 64 threads.  BACK = false: in = ext(x), out -> y1[0, N).
// BACK = true: in[p] = y1[N - 1 - p], out[p] -> result[N - 1 - p - padlen] where that lies in [0, n).
// y1 of item b: scratch + offsets[b] + 2 padlen b.  result of item b: out + offsets[b]; padded: out_pad + offsets[b] + 2 pad b.
template <int ORD, typename T, bool BACK>
static __global__ void __launch_bounds__(FILT_WAVE) k_filt_pass(const T* __restrict__ x, const int64_t* __restrict__ offsets, int64_t total,
                                                                int64_t max_len, FiltCoef c, int padlen, int warm, double* y1,
                                                                double* __restrict__ out, double* __restrict__ out_pad, int64_t pad) {
    const int b = blockIdx.y;
    const int64_t o0 = offsets[b];
    const int64_t n = offsets[b + 1] - o0;
    // an item the wrapper would have refused (not longer than padlen), or offsets that do not describe the buffers: nothing is touched
    if (o0 < 0 || n <= padlen || n > max_len || o0 + n > total) return;
    const int64_t N = n + 2 * (int64_t)padlen;
    const int64_t p0 = ((int64_t)blockIdx.x * FILT_WAVE + threadIdx.x) * FILT_LANE;
    if (p0 >= N) return;
    const int64_t p1 = p0 + FILT_LANE < N ? p0 + FILT_LANE : N;
    const int64_t s = p0 > warm ? p0 - warm : 0;
    const T* xb = x + o0;
    double* yb = y1 + o0 + 2 * (int64_t)padlen * b;
    double* ob = out + o0;
    double* pb = out_pad ? out_pad + o0 + 2 * pad * b : nullptr;
    if (pad >= n) pb = nullptr;  // np.pad's reflection needs n > pad (the wrapper refuses the call)

    // a group of samples -> registers, in the type they are stored in (the forward pass widens at use, so that the loads of the
    // next group stay in flight while this group is filtered)
    using In = typename std::conditional<BACK, double, T>::type;
    auto load = [&](In (&v)[FILT_UNROLL], int64_t p) {
        if constexpr (!BACK) {
            if (p >= padlen && p + FILT_UNROLL <= padlen + n) {
#pragma unroll
                for (int u = 0; u < FILT_UNROLL; ++u) v[u] = xb[p - padlen + u];
            } else {
#pragma unroll
                for (int u = 0; u < FILT_UNROLL; ++u) v[u] = p + u < N ? filt_ext(xb, n, padlen, p + u) : (T)0;
            }
        } else {
#pragma unroll
            for (int u = 0; u < FILT_UNROLL; ++u) v[u] = p + u < N ? yb[N - 1 - p - u] : 0.0;
        }
    };

    In cur[FILT_UNROLL], nxt[FILT_UNROLL] = {};
    load(cur, s);
    double z[ORD];
#pragma unroll
    for (int k = 0; k < ORD; ++k) z[k] = dmul_rn(c.zi[k], (double)cur[0]);  // lfilter_zi(b, a) * in[s]
    // one sample of lfilter, as the header states it: -> y
    auto step = [&](double xv) {
        const double y = dadd_rn(dmul_rn(c.b[0], xv), z[0]);
#pragma unroll
        for (int k = 0; k < ORD - 1; ++k) z[k] = dsub_rn(dadd_rn(dmul_rn(c.b[k + 1], xv), z[k + 1]), dmul_rn(c.a[k + 1], y));
        z[ORD - 1] = dsub_rn(dmul_rn(c.b[ORD], xv), dmul_rn(c.a[ORD], y));
        return y;
    };
    // the warm-up: p0 - s is a multiple of FILT_UNROLL (p0 and `warm` are multiples of FILT_LANE); nothing is stored, so a group of
    // samples is one straight run of arithmetic
    int64_t p = s;
    for (; p < p0; p += FILT_UNROLL) {
        load(nxt, p + FILT_UNROLL);  // (p + FILT_UNROLL <= p0 < N): in flight while this group is filtered
#pragma unroll
        for (int u = 0; u < FILT_UNROLL; ++u) step((double)cur[u]);
#pragma unroll
        for (int u = 0; u < FILT_UNROLL; ++u) cur[u] = nxt[u];
    }
    // the lane's own outputs
    for (; p < p1; p += FILT_UNROLL) {
        if (p + FILT_UNROLL < p1) load(nxt, p + FILT_UNROLL);
#pragma unroll
        for (int u = 0; u < FILT_UNROLL; ++u) {
            const double y = step((double)cur[u]);  // (past the end: zeros, never stored)
            const int64_t q = p + u;
            if (q < p1) {
                if (!BACK) {
                    yb[q] = y;
                } else {
                    const int64_t i = N - 1 - q - padlen;
                    if (i >= 0 && i < n) {
                        ob[i] = y;
                        if (pb) {  // np.pad(result, pad, mode="reflect"): padded[pad + i], and the mirror images of i at either end
                            pb[pad + i] = y;
                            if (i >= 1 && i <= pad) pb[pad - i] = y;
                            if (i <= n - 2 && i >= n - 1 - pad) pb[pad + 2 * (n - 1) - i] = y;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < FILT_UNROLL; ++u) cur[u] = nxt[u];
    }
}

}  // namespace rvcmi
