// Issue-model micro-benchmark for one- and two-wave-per-SIMD MFMA K loops on gfx950 (round 3).  Every variant runs the same
// structure as the generator's K loop -- per k-step MI*NJ v_mfma_f32_32x32x16_f16, NJ ds_read_b128 (B fragments, LA k-steps ahead),
// MI global_load_dwordx4 (A fragments, one 8-k-step ring refilled in place) -- plus FILL independent VALU instructions per MFMA,
// and reports cycles per MFMA per SIMD.  It answers: what does one extra instruction in an MFMA gap cost a lone wave (the
// model T = max(32, a + b n) fitted in DESIGN.md), does one s_waitcnt per k-step instead of one per MFMA matter, what do
// MI = 2 tiles (half the B reads) buy, and how much of it a second wave per SIMD hides.
// Build / run:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -o kloop2 kloop2.hip && ./kloop2   (output of round 3:
// profiles/r03_ubench_kloop2_issue_model.txt);  ./kloop2 shape  runs the MFMA shape arms further down instead
#include <hip/hip_runtime.h>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
using lds_cptr = const __attribute__((address_space(3))) char*;
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(size_t)(lds_cptr)p; }
__device__ __forceinline__ f16x8 lds_ld(unsigned a) { return *(const __attribute__((address_space(3))) f16x8*)(size_t)a; }

// WAIT: 0 = the compiler's own s_waitcnt (one per MFMA), 1 = one manual s_waitcnt lgkmcnt per k-step in front of the MFMAs
// LOADS: bit 0 = A global loads on, bit 1 = B ds_reads on
template <int MI, int NJ, int LA, int FILL, int WAIT, int LOADS, int NWV>
__global__ void __launch_bounds__(64 * NWV, NWV / 4) kloop2(const _Float16* w, int ksteps, int reps, float* out, unsigned long long* ticks) {
    extern __shared__ __attribute__((aligned(256))) char smem[];
    constexpr int STRIDE = 272, ROWS = 32 * NJ + 64;
    for (int i = threadIdx.x; i < ROWS * STRIDE / 4; i += 64 * NWV) ((float*)smem)[i] = 0.001f * (i % 97);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned xl = lds_addr(smem) + (unsigned)(lane & 31) * STRIDE + (unsigned)(lane >> 5) * 16;
    const _Float16* wl = w + (size_t)(wave & 3) * MI * ksteps * 512 + lane * 8;
    f32x16 acc[MI][NJ];
    for (int mi = 0; mi < MI; ++mi) for (int jt = 0; jt < NJ; ++jt) for (int e = 0; e < 16; ++e) acc[mi][jt][e] = 0.f;
    float fz[8];
    for (int i = 0; i < 8; ++i) fz[i] = 0.25f * (lane + i);
    f16x8 A[8][MI], Bf[LA + 1][NJ];
    for (int k = 0; k < 8; ++k) for (int mi = 0; mi < MI; ++mi) A[k][mi] = *(const f16x8*)(wl + (size_t)(mi * ksteps + k) * 512);
    for (int q = 0; q < LA; ++q) for (int jt = 0; jt < NJ; ++jt) Bf[q][jt] = lds_ld(xl + q * 32 + jt * 32 * STRIDE);
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int r = 0; r < reps; ++r) {
        unsigned xr = xl;            // running B base: one LDS row further per 8 k-steps (a tap), like the conv's tap loop
        const _Float16* wr = wl;     // running A base
        for (int k0 = 0; k0 < ksteps; k0 += 8 * (LA + 1)) {  // unrolled so that ring indices are static
            const _Float16* wn = (k0 + 8 * (LA + 1) < ksteps) ? wr + 8 * (LA + 1) * 512 : wl;  // next group (wraps at the end of the conv)
#pragma unroll
            for (int kk = 0; kk < 8 * (LA + 1); ++kk) {
                const unsigned nb = xr + (unsigned)(((kk + LA) & 7) * 32) + (unsigned)(((kk + LA) >> 3) * STRIDE);
                const _Float16* an = (kk + 8 < 8 * (LA + 1)) ? wr + (kk + 8) * 512 : wn + (kk + 8 - 8 * (LA + 1)) * 512;
                if (WAIT == 1 && (LOADS & 2)) __builtin_amdgcn_s_waitcnt(0xC07F | ((NJ * (LA - 1) > 15 ? 15 : NJ * (LA - 1)) << 8));
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int jt = 0; jt < NJ; ++jt) {
                        acc[mi][jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[kk & 7][mi], Bf[kk % (LA + 1)][jt], acc[mi][jt], 0, 0, 0);
                        const int i = mi * NJ + jt;
                        if ((LOADS & 2) && i < NJ) Bf[(kk + LA) % (LA + 1)][i] = lds_ld(nb + i * 32 * STRIDE);
                        if ((LOADS & 1) && i >= MI * NJ - MI) A[kk & 7][i - (MI * NJ - MI)] = *(const f16x8*)(an + (size_t)(i - (MI * NJ - MI)) * ksteps * 512);
#pragma unroll
                        for (int f = 0; f < FILL; ++f) {  // one VALU each, pinned to this gap (pure arithmetic is otherwise re-ordered by ISel)
                            float t = fz[f & 7];
                            asm volatile("v_mul_f32 %0, 0.5, %0" : "+v"(t));
                            fz[f & 7] = t;
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
            }
            xr += (LA + 1) * STRIDE;
            wr += 8 * (LA + 1) * 512;
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    float s = 0.f;
    for (int mi = 0; mi < MI; ++mi) for (int jt = 0; jt < NJ; ++jt) for (int e = 0; e < 16; ++e) s += acc[mi][jt][e];
    for (int i = 0; i < 8; ++i) s += fz[i];
    out[blockIdx.x * 64 * NWV + threadIdx.x] = s;
    if (lane == 0) ticks[blockIdx.x * NWV + wave] = t1 - t0;
}

template <int MI, int NJ, int LA, int FILL, int WAIT, int LOADS, int NWV>
void run(const char* note) {
    const int ksteps = 96, blocks = 256, reps = 100;  // 96 k-steps = a k = 11 conv at C = 128 (88) rounded to the unroll
    std::vector<_Float16> hw((size_t)4 * MI * ksteps * 512);
    for (size_t i = 0; i < hw.size(); ++i) hw[i] = (_Float16)(0.01f * ((int)(i % 13) - 6));
    _Float16* w; float* out; unsigned long long* ticks;
    hipMalloc(&w, hw.size() * 2); hipMemcpy(w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
    hipMalloc(&out, blocks * 64 * NWV * 4); hipMalloc(&ticks, blocks * NWV * 8);
    const size_t smem = (size_t)(32 * NJ + 64) * 272;
    auto kern = &kloop2<MI, NJ, LA, FILL, WAIT, LOADS, NWV>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * NWV), smem, 0, w, ksteps, 2, out, ticks);
    hipDeviceSynchronize();
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(64 * NWV), smem, 0, w, ksteps, reps, out, ticks);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> h(blocks * NWV);
    hipMemcpy(h.data(), ticks, h.size() * 8, hipMemcpyDeviceToHost);
    double avg = 0; for (auto v : h) avg += v; avg /= h.size();
    const double nm = (double)reps * ksteps * MI * NJ;
    const double tf = 2.0 * 32 * 32 * 16 * nm * NWV * blocks / (ms * 1e-3) / 1e12;
    printf("MI=%d NJ=%d LA=%d FILL=%d WAIT=%d LOADS=%d waves/SIMD=%d : %6.1f cycles per SIMD-MFMA  (%.0f TF/s, eff. clock %.2f GHz)  %s\n", MI, NJ, LA, FILL,
           WAIT, LOADS, NWV / 4, avg / nm / (NWV / 4), tf, avg / (ms * 1e-3) / 1e9, note);
    hipFree(w); hipFree(out); hipFree(ticks);
}

// ---- MFMA shape arms (`./kloop2 shape`, output profiles/kloop_shape_time.txt) -------------------------------------------------
// k_rb_stream's tile (32 channels x 192 rows per wave, one wave per SIMD) on v_mfma_f32_32x32x16_f16 against v_mfma_f32_16x16x32_f16,
// on SEEDED RANDOM operands (the chip holds its clock by load, and the 0.001 * (i % 97) image above is all but constant: on such
// operands the two shapes tie).  Both arms walk the same LDS image and the same packed weights [k_step][lane][8] in units of 32 k:
//   32: 2 k-steps x 6 tiles of 32 rows = 12 MFMAs, 12 B reads (one k-step ahead in a second buffer), 2 A fragments of 1 KB
//   16: 12 tiles of 16 rows x 2 channel halves = 24 MFMAs, 12 B reads (one per PAIR of MFMAs, refilled in place after the second),
//       2 A fragments of 1 KB gathered in 256-byte runs out of the two k-steps' fragments
// The A ring holds 128 k (8 fragments) and the B buffer 12 fragments in both; every MFMA gap is pinned with sched_barrier.
// B lane map of the 16 shape: K-block q = lane / 16 reads channel chunk {0, 2, 1, 3}[q] of the 32 k, and column n = lane % 16 reads
// an even row for n in 0-3, 12-15 and an odd one for n in 4-11, so that each ds_read_b128 lane group ({0-3,12-15,20-27}, ...) touches
// 16 distinct 16-byte slots with rows of 17 slots (the natural order puts two lanes of a group on one slot).
typedef float f32x4 __attribute__((ext_vector_type(4)));
__host__ __device__ constexpr int row16(int n) { return n < 4 ? 2 * n : n < 12 ? 2 * (n - 4) + 1 : 2 * (n - 8); }
__host__ __device__ constexpr int chunk16(int q) { return ((q & 1) << 1) | (q >> 1); }

template <int SHAPE, int LOADS>
__global__ void __launch_bounds__(256, 1) kshape(const _Float16* w, const _Float16* x, int ksteps, int reps, float* out, unsigned long long* ticks) {
    extern __shared__ __attribute__((aligned(256))) char smem[];
    constexpr int STRIDE = 272, ROWS = 256, NT = SHAPE == 32 ? 6 : 12, NE = SHAPE == 32 ? 16 : 4;
    using accv = typename std::conditional<SHAPE == 32, f32x16, f32x4>::type;
    for (int i = threadIdx.x; i < ROWS * STRIDE / 16; i += 256) ((f16x8*)smem)[i] = ((const f16x8*)x)[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned xl;
    const _Float16* wl = w + (size_t)wave * ksteps * 512;
    if (SHAPE == 32) {
        xl = lds_addr(smem) + (unsigned)(lane & 31) * STRIDE + (unsigned)(lane >> 5) * 16;
        wl += lane * 8;
    } else {
        const int q = lane >> 4, n = lane & 15;
        xl = lds_addr(smem) + (unsigned)row16(n) * STRIDE + (unsigned)chunk16(q) * 16;
        wl += ((q & 1) * 64 + (q >> 1) * 32 + n) * 8;  // k-step 2s + (q & 1), lanes 32 (q >> 1) + 16 h + n of the packed fragment
    }
    accv acc[2][NT];  // 32: [0][jt] only
    for (int h = 0; h < 2; ++h) for (int jt = 0; jt < NT; ++jt) for (int e = 0; e < NE; ++e) acc[h][jt][e] = 0.f;
    f16x8 A[8], Bf[12];  // A: 32 -> [k-step & 7], 16 -> [(32-k step & 3) * 2 + h];  Bf: 32 -> [(k-step & 1) * 6 + jt], 16 -> [jt]
    if (SHAPE == 32) {
        for (int k = 0; k < 8; ++k) A[k] = *(const f16x8*)(wl + (size_t)k * 512);
        for (int jt = 0; jt < 6; ++jt) Bf[jt] = lds_ld(xl + jt * 32 * STRIDE);
    } else {
        for (int k = 0; k < 8; ++k) A[k] = *(const f16x8*)(wl + (size_t)(k >> 1) * 1024 + (k & 1) * 128);
        for (int jt = 0; jt < 12; ++jt) Bf[jt] = lds_ld(xl + jt * 16 * STRIDE);
    }
    const unsigned long long t0 = __builtin_readcyclecounter();
    for (int r = 0; r < reps; ++r) {
        unsigned xr = xl;
        const _Float16* wr = wl;
        for (int k0 = 0; k0 < ksteps; k0 += 16) {  // 16 k-steps = two taps at C = 128, unrolled so that ring indices are static
            const _Float16* wn = (k0 + 16 < ksteps) ? wr + 16 * 512 : wl;
            if constexpr (SHAPE == 32) {
#pragma unroll
                for (int kk = 0; kk < 16; ++kk) {
                    const unsigned nb = xr + (unsigned)(((kk + 1) & 7) * 32) + (unsigned)(((kk + 1) >> 3) * STRIDE);
                    const _Float16* an = (kk + 8 < 16) ? wr + (kk + 8) * 512 : wn + (kk + 8 - 16) * 512;
#pragma unroll
                    for (int jt = 0; jt < 6; ++jt) {
                        acc[0][jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[kk & 7], Bf[(kk & 1) * 6 + jt], acc[0][jt], 0, 0, 0);
                        if (LOADS & 2) Bf[((kk + 1) & 1) * 6 + jt] = lds_ld(nb + jt * 32 * STRIDE);
                        if ((LOADS & 1) && jt == 5) A[kk & 7] = *(const f16x8*)an;
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            } else {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const unsigned nb = xr + (unsigned)(((s + 1) & 3) * 64) + (unsigned)(((s + 1) >> 2) * STRIDE);
                    const _Float16* an = (s + 4 < 8) ? wr + (s + 4) * 1024 : wn + (s + 4 - 8) * 1024;
#pragma unroll
                    for (int jt = 0; jt < 12; ++jt)
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            acc[h][jt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[(s & 3) * 2 + h], Bf[jt], acc[h][jt], 0, 0, 0);
                            if ((LOADS & 2) && h == 1) Bf[jt] = lds_ld(nb + jt * 16 * STRIDE);
                            if ((LOADS & 1) && jt == 11) A[(s & 3) * 2 + h] = *(const f16x8*)(an + h * 128);
                            __builtin_amdgcn_sched_barrier(0);
                        }
                }
            }
            xr += 2 * STRIDE;
            wr += 16 * 512;
        }
    }
    const unsigned long long t1 = __builtin_readcyclecounter();
    float s = 0.f;
    for (int h = 0; h < (SHAPE == 32 ? 1 : 2); ++h) for (int jt = 0; jt < NT; ++jt) for (int e = 0; e < NE; ++e) s += acc[h][jt][e];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (lane == 0) ticks[blockIdx.x * 4 + wave] = t1 - t0;
}

struct ShapeBufs { _Float16 *w, *x; float* out; unsigned long long* ticks; };

template <int SHAPE, int LOADS>
void run_shape(const ShapeBufs& b, int round) {
    const int ksteps = 96, blocks = 256, reps = 2000, launches = 4;  // about 20 ms per launch: long enough for the clock to settle
    const size_t smem = (size_t)256 * 272;
    auto kern = &kshape<SHAPE, LOADS>;
    hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    for (int i = 0; i < 2; ++i) hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), smem, 0, b.w, b.x, ksteps, reps, b.out, b.ticks);
    hipDeviceSynchronize();
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    hipEventRecord(e0);
    for (int i = 0; i < launches; ++i) hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), smem, 0, b.w, b.x, ksteps, reps, b.out, b.ticks);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms = 0; hipEventElapsedTime(&ms, e0, e1);
    ms /= launches;
    std::vector<unsigned long long> h(blocks * 4);
    hipMemcpy(h.data(), b.ticks, h.size() * 8, hipMemcpyDeviceToHost);  // the last launch's
    double avg = 0; for (auto v : h) avg += v; avg /= h.size();
    const double units = (double)reps * ksteps * 6;  // of 32 768 FLOP per wave: one 32x32x16 or two 16x16x32
    const double tf = 32768.0 * units * 4 * blocks / (ms * 1e-3) / 1e12;
    printf("round %d shape=%s LOADS=%d waves/SIMD=1 : %6.2f cycles per 32768 FLOP per SIMD  (%.0f TF/s, eff. clock %.3f GHz)  [%s]\n", round,
           SHAPE == 32 ? "32x32x16" : "16x16x32", LOADS, avg / units, tf, avg / (ms * 1e-3) / 1e9, LOADS ? "shipped mix" : "bare MFMAs");
    hipEventDestroy(e0); hipEventDestroy(e1);
}

int main_shape() {
    const int ksteps = 96, blocks = 256;
    unsigned long long st = 0x9E3779B97F4A7C15ull;  // seeded: xorshift64*, operands uniform in [-1, 1)
    auto rnd = [&]() {
        st ^= st >> 12; st ^= st << 25; st ^= st >> 27;
        return (_Float16)((float)((st * 0x2545F4914F6CDD1Dull) >> 40) * (2.f / 16777216.f) - 1.f);
    };
    std::vector<_Float16> hw((size_t)4 * ksteps * 512), hx((size_t)256 * 272 / 2);
    for (auto& v : hw) v = rnd();
    for (auto& v : hx) v = rnd();
    ShapeBufs b;
    hipMalloc(&b.w, hw.size() * 2); hipMemcpy(b.w, hw.data(), hw.size() * 2, hipMemcpyHostToDevice);
    hipMalloc(&b.x, hx.size() * 2); hipMemcpy(b.x, hx.data(), hx.size() * 2, hipMemcpyHostToDevice);
    hipMalloc(&b.out, blocks * 256 * 4); hipMalloc(&b.ticks, blocks * 4 * 8);
    for (int q = 0; q < 4; ++q) {  // the B lane map of the 16 shape: 16 distinct slots per ds_read_b128 lane group
        const int grp[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
        unsigned seen = 0;
        for (int i = 0; i < 16; ++i) {
            const int l = grp[q & 1][i] + 32 * (q >> 1);
            seen |= 1u << ((row16(l & 15) * 17 + chunk16(l >> 4)) & 15);
        }
        if (seen != 0xFFFFu) { printf("B lane map: bank conflict in lane group %d\n", q); return 1; }
    }
    printf("-- MFMA shape, k_rb_stream's tile (32 channels x 192 rows per wave), one wave per SIMD, seeded random fp16 operands in LDS and weights\n");
    printf("-- three rounds, shapes interleaved, one process; 256 blocks x 4 waves, 96 k-steps of 16 per conv, 2000 convs per launch\n");
    for (int round = 1; round <= 3; ++round) {
        run_shape<32, 0>(b, round);
        run_shape<16, 0>(b, round);
        run_shape<32, 3>(b, round);
        run_shape<16, 3>(b, round);
    }
    hipFree(b.w); hipFree(b.x); hipFree(b.out); hipFree(b.ticks);
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "shape") return main_shape();
    printf("-- one wave per SIMD, MI=1 NJ=6 (k_rb_stream's tile): ablations\n");
    run<1, 6, 1, 0, 0, 0, 4>("MFMA only");
    run<1, 6, 1, 0, 0, 1, 4>("A loads only");
    run<1, 6, 1, 0, 0, 2, 4>("B reads only");
    run<1, 6, 1, 0, 0, 3, 4>("the K loop as shipped (B one k-step ahead, compiler waits)");
    run<1, 6, 2, 0, 0, 3, 4>("B two k-steps ahead");
    run<1, 6, 2, 0, 1, 3, 4>("B two k-steps ahead, ONE s_waitcnt per k-step");
    printf("-- cost of fillers for a lone wave (MI=1 NJ=6, full loads)\n");
    run<1, 6, 2, 1, 1, 3, 4>("");
    run<1, 6, 2, 2, 1, 3, 4>("");
    run<1, 6, 2, 4, 1, 3, 4>("");
    run<1, 6, 2, 6, 1, 3, 4>("");
    printf("-- fillers beside bare MFMAs (no loads)\n");
    run<1, 6, 1, 1, 0, 0, 4>("");
    run<1, 6, 1, 2, 0, 0, 4>("");
    run<1, 6, 1, 3, 0, 0, 4>("");
    run<1, 6, 1, 4, 0, 0, 4>("");
    run<1, 6, 1, 6, 0, 0, 4>("");
    run<1, 6, 1, 8, 0, 0, 4>("");
    printf("-- MI=2 tiles (half the B reads per MFMA)\n");
    run<2, 3, 2, 0, 0, 3, 4>("compiler waits");
    run<2, 3, 2, 0, 1, 3, 4>("one wait per k-step");
    run<2, 3, 2, 2, 1, 3, 4>("");
    run<2, 3, 2, 4, 1, 3, 4>("");
    run<2, 4, 2, 0, 1, 3, 4>("MI=2 NJ=4");
    printf("-- NJ=3 halves (k_rb_stream3's slots), one wave per SIMD\n");
    run<1, 3, 2, 0, 0, 3, 4>("compiler waits");
    run<1, 3, 2, 0, 1, 3, 4>("one wait per k-step");
    run<1, 3, 2, 4, 1, 3, 4>("");
    printf("-- two waves per SIMD (8-wave block), NJ=3\n");
    run<1, 3, 2, 0, 0, 3, 8>("compiler waits");
    run<1, 3, 2, 0, 1, 3, 8>("one wait per k-step");
    run<1, 3, 2, 2, 1, 3, 8>("");
    run<1, 3, 2, 4, 1, 3, 8>("");
    run<1, 3, 2, 6, 1, 3, 8>("");
    run<1, 3, 2, 8, 1, 3, 8>("");
    run<2, 2, 2, 0, 1, 3, 8>("MI=2 NJ=2");
    run<2, 2, 2, 4, 1, 3, 8>("MI=2 NJ=2");
    return 0;
}
