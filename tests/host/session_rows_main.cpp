// Stand-alone check of csrc/session_rows.hpp, the host-only validation and planning of the per-session bank entries
// (rvcmi_ivf_search_blend_expand_sessions, rvcmi_glue_envelope_mix_sessions, rvcmi_glue_input_gate_sessions; no HIP, no Python): built by
// tests/test_cpu_rt_bank_sliders.py with the sanitizers on.  Prints "session rows ok" when every case gives the expected verdict.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../retrieval-based-voice-conversion-webui_amd/csrc/session_rows.hpp"

using namespace rvcmi;

static int failures = 0;

static void report(const char* what, bool good, const char* why) {
    std::printf("%-62s %s%s%s\n", what, good ? "ok" : "FAILED", why ? ": " : "", why ? why : "");
    if (!good) ++failures;
}

static rvcmi_session_blend bl(float rate, float protect, int slot, int on) { return rvcmi_session_blend{rate, protect, slot, on}; }

static void blend(const char* what, const std::vector<rvcmi_session_blend>& v, int64_t nq, int64_t skip, int64_t p_len, bool index, bool pitchf,
                  bool ok, int active = -1, int64_t rows = -1, int any_protect = -1) {
    SessionBlendPlan plan = {-7, -7, -7};
    const char* why = session_blend_check(v.empty() ? nullptr : v.data(), (int)v.size(), nq, skip, p_len, index, pitchf, &plan);
    bool good = (why == nullptr) == ok;
    if (good && ok && active >= 0) good = plan.active == active && plan.rows == rows && plan.any_protect == any_protect;
    report(what, good, why);
}

static void mix(const char* what, const std::vector<rvcmi_session_mix>& v, bool ok, int active = -1) {
    int n = -7;
    const char* why = session_mix_check(v.empty() ? nullptr : v.data(), (int)v.size(), &n);
    report(what, (why == nullptr) == ok && (!ok || active < 0 || n == active), why);
}

static void gate(const char* what, const std::vector<rvcmi_session_gate>& v, bool ok, int active = -1) {
    int n = -7;
    const char* why = session_gate_check(v.empty() ? nullptr : v.data(), (int)v.size(), &n);
    report(what, (why == nullptr) == ok && (!ok || active < 0 || n == active), why);
}

int main() {
    static_assert(sizeof(rvcmi_session_blend) == 16 && sizeof(rvcmi_session_mix) == 8 && sizeof(rvcmi_session_gate) == 16, "descriptor sizes");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::nanf("");
    // retrieval: nq 9, skip 4, p_len 17 -- the shapes of the device test
    blend("two of three sessions blend", {bl(0.75f, 0.33f, 0, 1), bl(0.f, 1.f, -1, 0), bl(0.3f, 0.49f, 1, 1)}, 9, 4, 17, true, true, true, 2, 10, 1);
    blend("no session blends: nothing to search", {bl(0.f, 0.33f, -1, 1), bl(0.f, 1.f, -1, 0)}, 9, 4, 17, true, true, true, 0, 0, 1);
    blend("all blend, no protect, no pitchf", {bl(0.5f, 1.f, 0, 0), bl(0.25f, 1.f, 1, 0), bl(1.f, 1.f, 2, 0)}, 9, 4, 17, true, false, true, 3, 15, 0);
    blend("no index, a protect per session", {bl(0.f, 0.33f, -1, 1), bl(0.f, 1.f, -1, 0)}, 9, 4, 17, false, true, true, 0, 0, 1);
    blend("skip_rows == nq: slots, no rows", {bl(0.5f, 1.f, 0, 0)}, 9, 9, 18, true, false, true, 1, 0, 0);
    blend("S = 65535", std::vector<rvcmi_session_blend>(65535, bl(0.f, 1.f, -1, 0)), 9, 4, 17, true, false, true, 0, 0, 0);
    blend("S = 0", {}, 9, 4, 17, true, true, false);
    blend("S = 65536", std::vector<rvcmi_session_blend>(65536, bl(0.f, 1.f, -1, 0)), 9, 4, 17, true, false, false);
    blend("p_len > 2 nq", {bl(0.75f, 0.33f, 0, 1)}, 9, 4, 19, true, true, false);
    blend("negative p_len", {bl(0.75f, 0.33f, 0, 1)}, 9, 4, -1, true, true, false);
    blend("nq = 0", {bl(0.75f, 0.33f, 0, 1)}, 0, 0, 0, true, true, false);
    blend("skip_rows > nq", {bl(0.75f, 0.33f, 0, 1)}, 9, 10, 17, true, true, false);
    blend("negative skip_rows", {bl(0.75f, 0.33f, 0, 1)}, 9, -1, 17, true, true, false);
    blend("NaN index_rate", {bl(nan, 0.33f, 0, 1)}, 9, 4, 17, true, true, false);
    blend("inf protect", {bl(0.75f, inf, 0, 1)}, 9, 4, 17, true, true, false);
    blend("slots do not start at 0", {bl(0.75f, 1.f, 1, 0)}, 9, 4, 17, true, false, false);
    blend("slots skip a number", {bl(0.75f, 1.f, 0, 0), bl(0.5f, 1.f, 2, 0)}, 9, 4, 17, true, false, false);
    blend("the same slot twice", {bl(0.75f, 1.f, 0, 0), bl(0.5f, 1.f, 0, 0)}, 9, 4, 17, true, false, false);
    blend("slot -2", {bl(0.75f, 1.f, -2, 0)}, 9, 4, 17, true, false, false);
    blend("slot INT_MAX", {bl(0.75f, 1.f, std::numeric_limits<int>::max(), 0)}, 9, 4, 17, true, false, false);
    blend("a slot without an index", {bl(0.75f, 1.f, 0, 0)}, 9, 4, 17, false, false, false);
    blend("protect_on without pitchf", {bl(0.f, 0.33f, -1, 1)}, 9, 4, 17, true, false, false);
    blend("protect_on = 2", {bl(0.f, 0.33f, -1, 2)}, 9, 4, 17, true, true, false);
    // envelope mix
    mix("rates 0, 0.5, 1: two on", {{1.f, 1}, {0.5f, 1}, {0.f, 0}}, true, 2);
    mix("all off", {{0.f, 0}, {0.f, 0}}, true, 0);
    mix("a negative exponent (rate above 1) that is off", {{-0.5f, 0}}, true, 0);
    mix("S = 0", {}, false);
    mix("NaN exponent", {{1.f, 1}, {nan, 1}}, false);
    mix("NaN exponent of a session that is off", {{nan, 0}}, false);
    mix("inf exponent", {{inf, 1}}, false);
    mix("on = 3", {{1.f, 3}}, false);
    // input gate
    gate("two on, one off", {{0.01f, 100.f, 1, 0}, {0.f, 0.f, 0, 0}, {0.1f, inf, 1, 0}}, true, 2);
    gate("cut_a = 0: never quiet", {{0.f, 0.f, 1, 0}}, true, 1);
    gate("S = 0", {}, false);
    gate("NaN cut_a", {{nan, 1.f, 1, 0}}, false);
    gate("NaN cut_b of a session that is off", {{0.f, nan, 0, 0}}, false);
    gate("negative cutoff", {{-1.f, 1.f, 1, 0}}, false);
    gate("on = -1", {{0.f, 0.f, -1, 0}}, false);
    gate("reserved_ != 0", {{0.f, 0.f, 1, 5}}, false);
    if (failures) {
        std::printf("%d case(s) failed\n", failures);
        return 1;
    }
    std::printf("session rows ok\n");
    return 0;
}
