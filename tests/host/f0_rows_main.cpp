// Stand-alone check of csrc/f0_rows.hpp, the host-only validation of rvcmi_glue_rmvpe_f0_ragged's descriptors (no HIP, no Python):
// built by tests/test_cpu_f0_rows.py with the sanitizers on.  Prints "f0 rows ok" when every case gives the expected verdict.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../retrieval-based-voice-conversion-webui_amd/csrc/f0_rows.hpp"

using rvcmi::F0RowsPlan;
using rvcmi::f0_rows_check;

static rvcmi_f0_row row(int first, int n, int p_len, int64_t out_off, double key_mul = 1.0) {
    rvcmi_f0_row r;
    std::memset(&r, 0, sizeof r);
    r.first_row = first, r.n = n, r.p_len = p_len, r.out_off = out_off, r.key_mul = key_mul;
    return r;
}

static int failures = 0;

static void expect(const char* what, const std::vector<rvcmi_f0_row>& rows, int64_t R, int64_t out_len, bool ok, int use_global = -1,
                   size_t lds = 0) {
    F0RowsPlan plan = {false, 0};
    const char* why = f0_rows_check(rows.data(), (int)rows.size(), R, out_len, &plan);
    bool good = (why == nullptr) == ok;
    if (good && ok && use_global >= 0) good = plan.use_global == (use_global != 0) && plan.lds_doubles == lds;
    std::printf("%-55s %s%s%s\n", what, good ? "ok" : "FAILED", why ? ": " : "", why ? why : "");
    if (!good) ++failures;
}

int main() {
    static_assert(sizeof(rvcmi_f0_row) == 32 && alignof(rvcmi_f0_row) == 8, "the descriptor is 32 bytes, 8-byte aligned");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    expect("two items, a gap row between them", {row(0, 3, 5, 0), row(4, 4, 6, 5)}, 8, 11, true, 0, 10);
    expect("items in any order", {row(4, 4, 6, 5), row(0, 3, 5, 0)}, 8, 11, true, 0, 10);
    expect("gaps between the outputs", {row(0, 3, 5, 2), row(3, 4, 6, 9)}, 7, 20, true, 0, 10);
    expect("10240 + 10240 frames: the last size in LDS", {row(0, 10240, 10240, 0), row(10240, 3, 7, 10240)}, 10243, 10247, true, 0, 20480);
    expect("one frame more: every item in global memory", {row(0, 10240, 10241, 0), row(10240, 3, 7, 10241)}, 10243, 10248, true, 1, 0);
    expect("no item", {}, 8, 11, false);
    expect("n = 0", {row(0, 0, 5, 0)}, 8, 11, false);
    expect("p_len = 0", {row(0, 3, 0, 0)}, 8, 11, false);
    expect("negative first row", {row(-1, 3, 5, 0)}, 8, 11, false);
    expect("a source past R", {row(6, 3, 5, 0)}, 8, 11, false);
    expect("first_row + n overflows an int", {row(2147483647, 2147483647, 5, 0)}, 8, 11, false);
    expect("overlapping sources", {row(0, 4, 5, 0), row(3, 4, 6, 5)}, 8, 11, false);
    expect("the same source twice", {row(0, 4, 5, 0), row(0, 4, 6, 5)}, 8, 11, false);
    expect("overlapping outputs", {row(0, 3, 5, 0), row(4, 4, 6, 4)}, 8, 11, false);
    expect("an output past the end", {row(0, 3, 5, 0), row(4, 4, 6, 6)}, 8, 11, false);
    expect("a negative output offset", {row(0, 3, 5, -1)}, 8, 11, false);
    expect("out_off + p_len overflows", {row(0, 3, 5, std::numeric_limits<int64_t>::max() - 2)}, 8, 11, false);
    expect("key factor inf", {row(0, 3, 5, 0, inf)}, 8, 11, false);
    expect("key factor NaN", {row(0, 3, 5, 0, nan)}, 8, 11, false);
    expect("key factor 0", {row(0, 3, 5, 0, 0.0)}, 8, 11, false);
    expect("R = 0", {row(0, 3, 5, 0)}, 0, 11, false);
    if (failures) {
        std::printf("%d case(s) failed\n", failures);
        return 1;
    }
    std::printf("f0 rows ok\n");
    return 0;
}
