// Host-only: the (hi, lo') pair of fp16 values that carries one fp32 MFMA operand in the front's "fp16x2" mode.
//
//     hi  = fp16(x)                     round-to-nearest-even, saturating at +-65504 like the device's to_op<_Float16>
//     lo' = fp16((x - hi) * 2^11)       the residual, SCALED: a normal fp16 number unless the residual is below 2^-25 in size
//     x  ~= hi + lo' * 2^-11            to 2^-21 relative (2^-22 typical) for |x| in fp16's normal range
//
// Unscaled, the residual of a weight of size 0.03 (about 1.5e-5) would lie below fp16's smallest normal number (6.1e-5), and whether the
// matrix cores keep subnormal inputs is not something the mode may depend on.  A product a * b is taken as
//     a_hi * b_hi  +  2^-11 * (a_hi * b_lo' + a_lo' * b_hi)
// (the lo * lo term, 2^-22 relative, is dropped); the kernels keep the bracket in an accumulator of its own and fold it in once.
// The conversions are written in integer arithmetic: no dependence on the compiler's _Float16 support (the CPU test is built with g++).
#pragma once
#include <cstdint>
#include <cstring>

namespace rvcmi {

constexpr int SPLIT_F16_SHIFT = 11;
constexpr float SPLIT_F16_SCALE = 2048.f;           // 2^11
constexpr float SPLIT_F16_INV = 1.f / 2048.f;       // 2^-11, what the epilogue folds the cross terms in with

// fp32 -> fp16 bits, round-to-nearest-even; finite values beyond the range saturate to +-65504, NaN stays NaN
static inline uint16_t split_f32_to_f16_sat(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
    const uint32_t a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);  // NaN
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7bffu);  // >= 65520 rounds past the largest finite fp16 (inf included): saturate
    if (a < 0x33000000u) return sign;                         // < 2^-25: rounds to zero (2^-25 itself ties to even = 0)
    const int e = (int)(a >> 23) - 127;
    uint32_t m = (a & 0x7fffffu) | 0x800000u;                 // 24-bit significand
    int shift;                                                // bits dropped from m
    uint32_t base;
    if (e >= -14) {
        shift = 13;
        base = (uint32_t)(e + 14) << 10;                      // m's leading 1 (bit 10 after the shift) adds the last exponent step
    } else {
        shift = 13 + (-14 - e);                               // subnormal result: spacing 2^-24
        base = 0;
    }
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) ++r;         // a carry walks into the exponent field, which is what rounding up means
    return (uint16_t)(sign | (base + r));
}

static inline float split_f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    uint32_t u;
    if (e == 0) {
        if (m == 0) {
            u = sign;
        } else {  // subnormal: m * 2^-24, exact in fp32
            float f = (float)m * (1.f / 16777216.f);
            memcpy(&u, &f, 4);
            u |= sign;
        }
    } else if (e == 31) {
        u = sign | 0x7f800000u | (m << 13);
    } else {
        u = sign | ((e + 112u) << 23) | (m << 13);
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct SplitF16 {
    uint16_t hi, lo;  // fp16 bit patterns; lo holds lo' = (x - hi) * 2^11
};

static inline SplitF16 split_f16(float x) {
    SplitF16 s;
    s.hi = split_f32_to_f16_sat(x);
    const float r = x - split_f16_to_f32(s.hi);  // exact in fp32 (Sterbenz) unless x was saturated
    s.lo = split_f32_to_f16_sat(r * SPLIT_F16_SCALE);
    return s;
}

static inline float join_f16(SplitF16 s) { return split_f16_to_f32(s.hi) + split_f16_to_f32(s.lo) * SPLIT_F16_INV; }

}  // namespace rvcmi
