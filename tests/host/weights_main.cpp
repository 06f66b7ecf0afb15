// Stand-alone driver of csrc/weights.hpp (WeightTable, Carve) for tests/test_cpu_weights.py: built with a plain C++ compiler under
// -fsanitize=address,undefined together with csrc/error.cpp, run as a child process.  Prints one "ok <case>" line per case and
// "weights ok" at the end; the first failed expectation prints what it saw and exits 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>

#include "../../retrieval-based-voice-conversion-webui_amd/csrc/weights.hpp"

using namespace rvcmi;

namespace {

rvcmi_tensor tensor(const char* name, const float* data, std::initializer_list<int64_t> shape) {
    rvcmi_tensor t;
    memset(&t, 0, sizeof t);
    t.name = name;
    t.data = data;
    t.ndim = (int)shape.size();
    int i = 0;
    for (int64_t s : shape)
        if (i < 4) t.shape[i++] = s;
    return t;
}

void fail(const char* what, const std::string& saw) {
    printf("FAILED %s: %s\n", what, saw.c_str());
    exit(1);
}

// f must end in the error `code` with a message that contains `text`
void expect_error(const char* what, int code, const char* text, const std::function<void()>& f) {
    const int rc = guarded(f);
    const std::string msg = rvcmi_last_error();
    if (rc != code) fail(what, "code " + std::to_string(rc) + " (" + msg + ")");
    if (msg.find(text) == std::string::npos) fail(what, "message '" + msg + "' lacks '" + text + "'");
    printf("ok %s: %d %s\n", what, rc, msg.c_str());
}

void expect(const char* what, bool ok) {
    if (!ok) fail(what, "expectation not met");
    printf("ok %s\n", what);
}

}  // namespace

int main() {
    const float a[6] = {1, 2, 3, 4, 5, 6}, b[2] = {7, 8}, c[6] = {9, 9, 9, 9, 9, 9};
    {
        const rvcmi_tensor w[] = {tensor("a.weight", a, {2, 3}), tensor("b.bias", b, {2})};
        WeightTable t(w, 2, "test_create");
        expect("found", t.get("a.weight", {2, 3}) == a && t.get("b.bias", {2}) == b && t.has("b.bias") && !t.has("c") && t.find("a.weight") == &w[0] &&
                            t.find("c") == nullptr && t.size() == 2 && t.used() == 2);
        t.require_all_used("thing");
        expect_error("missing", RVCMI_ERR_MISSING, "missing weight tensor 'c.weight'", [&] { t.get("c.weight", {2}); });
        expect_error("message names the caller", RVCMI_ERR_MISSING, "test_create", [&] { t.get("c.weight", {2}); });
        expect_error("wrong rank", RVCMI_ERR_INVALID, "a.weight", [&] { t.get("a.weight", {6}); });
        expect_error("wrong extent", RVCMI_ERR_INVALID, "dim 1 is 3, expected 4", [&] { t.get("a.weight", {2, 4}); });
        expect_error("rank 5 asked for", RVCMI_ERR_INVALID, "a.weight", [&] { t.get("a.weight", {1, 1, 1, 2, 3}); });
    }
    {
        rvcmi_tensor w[] = {tensor("r5", a, {1, 1, 1, 2}), tensor("nodata", nullptr, {2})};
        w[0].ndim = 5;  // a rank the struct cannot describe: shape[4] must never be read
        WeightTable t(w, 2, "test_create");
        expect_error("rank 5 supplied", RVCMI_ERR_INVALID, "r5", [&] { t.get("r5", {1, 1, 1, 2}); });
        expect_error("null data", RVCMI_ERR_INVALID, "no data", [&] { t.get("nodata", {2}); });
        expect("a refused tensor does not count as used", t.used() == 0);
    }
    {
        const rvcmi_tensor w[] = {tensor("a", a, {6}), tensor(nullptr, b, {2})};
        expect_error("null name", RVCMI_ERR_INVALID, "tensor 1 has no name", [&] { WeightTable t(w, 2, "test_create"); });
        expect_error("null array", RVCMI_ERR_INVALID, "null", [&] { WeightTable t(nullptr, 2, "test_create"); });
        WeightTable empty(nullptr, 0, "test_create");
        expect("an empty table", empty.size() == 0 && !empty.has("a"));
    }
    {
        const rvcmi_tensor w[] = {tensor("a", a, {6}), tensor("extra", b, {2}), tensor("other.x", b, {2})};
        WeightTable t(w, 3, "test_create");
        t.get("a", {6});
        expect_error("one left over", RVCMI_ERR_INVALID, "3 tensors were supplied, the recognised thing has 1", [&] { t.require_all_used("thing"); });
        expect_error("left over under a counted prefix", RVCMI_ERR_INVALID, "2 tensors", [&] { t.require_all_used("thing", {"a", "ex"}); });
        t.require_all_used("thing", {"a"});  // the others are outside the prefixes: not this caller's business
        t.get("a", {6});
        expect("asking twice counts once", t.used() == 1);
    }
    {
        const rvcmi_tensor w[] = {tensor("a", a, {6}), tensor("a", c, {2, 3})};
        WeightTable t(w, 2, "test_create");
        expect("duplicate: the last wins", t.size() == 1 && t.get("a", {2, 3}) == c);
        expect_error("duplicate: the first is gone", RVCMI_ERR_INVALID, "a", [&] { t.get("a", {6}); });
    }
    {
        const size_t sizes[] = {0, 1, 255, 256, 257}, want[] = {0, 0, 256, 512, 768}, rounded[] = {0, 256, 256, 256, 512};
        Carve cv;
        size_t sum = 0;
        bool ok = true;
        for (int i = 0; i < 5; ++i) {
            const size_t at = cv.take(sizes[i]);
            sum += rounded[i];
            ok = ok && at == want[i] && at % 256 == 0 && cv.off == sum && align256(sizes[i]) == rounded[i];
        }
        expect("carve", ok && cv.off == 1280);
        expect("align256 near the top", align256(((size_t)1 << 40) + 1) == ((size_t)1 << 40) + 256);
    }
    printf("weights ok\n");
    return 0;
}
