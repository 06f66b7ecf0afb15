// Host-only checks of rvcmi_glue_rmvpe_f0_ragged's descriptors (no HIP here: tests/host/f0_rows_main.cpp compiles this with a plain C++
// compiler).  The kernel reads the device copy of what is checked here, so everything that could take a block out of its buffers is
// refused before anything is launched.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/rvcmi.h"

namespace rvcmi {

constexpr size_t F0_LDS_BYTES = 160 * 1024;  // the dynamic LDS k_f0_post and k_f0_post_ragged may ask for (the one place it is written)

struct F0RowsPlan {
    bool use_global;     // some item's work arrays do not fit the LDS: every item works in global memory
    size_t lds_doubles;  // n + p_len of the largest item (the launch's dynamic LDS), 0 in global mode
};

// nullptr when the descriptors are fine (then *plan is filled), else what is wrong with them.
inline const char* f0_rows_check(const rvcmi_f0_row* rows, int nseq, int64_t R, int64_t out_len, F0RowsPlan* plan) {
    if (!rows || nseq < 1) return "at least one item";
    if (R < 1 || R > (1ll << 30) || out_len < 1) return "1 <= R <= 2^30 packed rows and a non-empty output";
    std::vector<std::pair<int64_t, int64_t>> src((size_t)nseq), dst((size_t)nseq);
    int64_t largest = 0;
    for (int i = 0; i < nseq; ++i) {
        const rvcmi_f0_row& d = rows[i];
        if (d.n < 1 || d.p_len < 1) return "an item with n < 1 or p_len < 1";
        if (!std::isfinite(d.key_mul) || !(d.key_mul > 0.0)) return "a key factor that is not finite and positive (the key is not finite)";
        if (d.first_row < 0 || (int64_t)d.first_row + d.n > R) return "source rows outside the packed salience";
        if (d.out_off < 0 || d.out_off > out_len - d.p_len) return "an output range outside the packed output";
        src[(size_t)i] = {(int64_t)d.first_row, (int64_t)d.first_row + d.n};
        dst[(size_t)i] = {d.out_off, d.out_off + d.p_len};
        largest = std::max<int64_t>(largest, (int64_t)d.n + d.p_len);
    }
    std::sort(src.begin(), src.end());
    std::sort(dst.begin(), dst.end());
    for (int i = 1; i < nseq; ++i) {
        if (src[(size_t)i].first < src[(size_t)i - 1].second) return "source ranges of two items overlap";
        if (dst[(size_t)i].first < dst[(size_t)i - 1].second) return "output ranges of two items overlap";
    }
    plan->use_global = (size_t)largest * sizeof(double) > F0_LDS_BYTES;
    plan->lds_doubles = plan->use_global ? 0 : (size_t)largest;
    return nullptr;
}

}  // namespace rvcmi
