// Stand-alone host program over csrc/split_f16.hpp (the (hi, lo') fp16 pair of the front's fp16x2 operand mode; no GPU, no HIP).
// Built and driven by tests/test_cpu_front_split.py with -fsanitize=address,undefined; nothing of it is loaded into Python.
//
//   split IN OUT   IN: raw float32 values; OUT: for each value the fp16 bit patterns hi, lo' (uint16 each) and join_f16 (float32)
//   selfcheck      hi + lo' * 2^-11 against x over every fp16 value, its neighbours and a weight-sized sweep
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../retrieval-based-voice-conversion-webui_amd/csrc/split_f16.hpp"

using namespace rvcmi;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

static int split_file(const char* in, const char* out) {
    FILE* f = fopen(in, "rb");
    CHECK(f);
    std::vector<float> x;
    float v;
    while (fread(&v, sizeof(v), 1, f) == 1) x.push_back(v);
    fclose(f);
    FILE* g = fopen(out, "wb");
    CHECK(g);
    for (float xi : x) {
        const SplitF16 s = split_f16(xi);
        const float j = join_f16(s);
        CHECK(fwrite(&s.hi, 2, 1, g) == 1 && fwrite(&s.lo, 2, 1, g) == 1 && fwrite(&j, 4, 1, g) == 1);
    }
    fclose(g);
    printf("split ok: %zu values\n", x.size());
    return 0;
}

static void check_value(double x, double* worst) {
    const float xf = (float)x;
    const SplitF16 s = split_f16(xf);
    const double j = (double)split_f16_to_f32(s.hi) + (double)split_f16_to_f32(s.lo) / 2048.0;
    const double a = std::fabs((double)xf);
    if (a >= 6.103515625e-05 && a <= 65504.0) {  // fp16's normal range
        const double rel = std::fabs(j - (double)xf) / a;
        if (rel > *worst) *worst = rel;
        CHECK(rel <= 1.0 / 2097152.0);  // 2^-21
        // lo' is a NORMAL fp16 number unless the residual itself is below 2^-25 (dropping such a lo' costs at most 2^-25 absolute)
        CHECK((s.lo & 0x7c00u) != 0 || std::fabs((double)xf - (double)split_f16_to_f32(s.hi)) < 2.98023223876953125e-08);
    } else if (a < 6.103515625e-05) {
        CHECK(std::fabs(j - (double)xf) <= 1.4551915228366852e-11);  // 2^-36: hi subnormal (spacing 2^-24), lo' keeps the rest
    }
    CHECK(join_f16(s) == (float)j || std::fabs(join_f16(s) - (float)j) <= 1e-7f * (float)a);
}

static int selfcheck() {
    double worst = 0.0;
    for (unsigned h = 0; h < 0x10000u; ++h) {  // every fp16 value: exact (lo' = 0), and its fp32 neighbourhood
        if (((h >> 10) & 0x1fu) == 31u) continue;
        const float f = split_f16_to_f32((uint16_t)h);
        CHECK(split_f32_to_f16_sat(f) == (uint16_t)h || f == 0.f);
        const SplitF16 s = split_f16(f);
        CHECK(s.hi == (uint16_t)h && (s.lo & 0x7fffu) == 0);
        for (double k : {-0.49, -0.25, 0.1, 0.3, 0.499}) check_value((double)f * (1.0 + k / 1024.0), &worst);
    }
    for (int i = -2000; i <= 2000; ++i) check_value(0.03 + i * 7.3e-6, &worst);   // weight-sized
    for (int i = -2000; i <= 2000; ++i) check_value(-0.03 + i * 7.3e-6, &worst);
    for (int i = -500; i <= 500; ++i) check_value(6.103515625e-05 * (1.0 + i / 1000.0), &worst);  // around the smallest normal
    CHECK(split_f16(70000.f).hi == 0x7bffu && split_f16(-1e30f).hi == 0xfbffu);  // saturation, never inf
    CHECK(split_f16(0.f).hi == 0 && split_f16(0.f).lo == 0 && split_f16(-0.f).hi == 0x8000u);
    CHECK(split_f16(65504.f).hi == 0x7bffu && split_f16(65504.f).lo == 0);
    printf("selfcheck ok: worst relative error %.3e (2^-21 = 4.768e-07)\n", worst);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "split")) return split_file(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "selfcheck")) return selfcheck();
    fprintf(stderr, "usage: %s split IN OUT | selfcheck\n", argv[0]);
    return 2;
}
