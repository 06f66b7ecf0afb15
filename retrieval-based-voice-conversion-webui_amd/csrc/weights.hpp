// Named host weights of a create call (the `rvcmi_tensor` array of include/rvcmi.h) and the 256-byte offset planner of the workspaces.
// Host-only like ivf_format.hpp: no HIP here, so the stand-alone test program (tests/host/weights_main.cpp) builds it with a plain C++
// compiler and sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <map>
#include <set>
#include <string>

#include "../../include/rvcmi.h"
#include "error.hpp"

namespace rvcmi {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// Hands out consecutive 256-byte aligned offsets: take(bytes) -> where the part starts; `off` is the total so far.
struct Carve {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += align256(bytes);
        return at;
    }
};

// name -> tensor.  Of two entries with one name the last wins.  `who` prefixes every message and must outlive the table.
struct WeightTable {
    const char* who;
    std::map<std::string, const rvcmi_tensor*> m;
    std::set<const rvcmi_tensor*> taken;  // what get() has handed out

    WeightTable(const rvcmi_tensor* w, int n, const char* who_) : who(who_) {
        if (!w && n) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: null weight array", who);
        for (int i = 0; i < n; ++i) {
            if (!w[i].name) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: tensor %d has no name", who, i);
            m[w[i].name] = &w[i];
        }
    }
    const rvcmi_tensor* find(const std::string& name) const {
        auto it = m.find(name);
        return it == m.end() ? nullptr : it->second;
    }
    bool has(const std::string& name) const { return find(name) != nullptr; }
    size_t size() const { return m.size(); }
    size_t used() const { return taken.size(); }

    // The fp32 data of `name`, which must have exactly this shape.
    const float* get(const std::string& name, std::initializer_list<int64_t> shape) {
        const rvcmi_tensor* t = find(name);
        if (!t) RVCMI_FAIL(RVCMI_ERR_MISSING, "%s: missing weight tensor '%s'", who, name.c_str());
        if (shape.size() > 4 || t->ndim != (int)shape.size())
            RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: weight '%s' has %d dimensions, expected %d", who, name.c_str(), t->ndim, (int)shape.size());
        int i = 0;
        for (int64_t s : shape) {
            if (t->shape[i] != s)
                RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: weight '%s': dim %d is %lld, expected %lld", who, name.c_str(), i, (long long)t->shape[i], (long long)s);
            ++i;
        }
        if (!t->data) RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: weight '%s' has no data", who, name.c_str());
        taken.insert(t);
        return (const float*)t->data;
    }

    // Refuses a table that holds tensors the caller never asked for (a geometry it does not serve).  With prefixes, only names that
    // begin with one of them count as supplied.
    void require_all_used(const char* what, std::initializer_list<const char*> prefixes = {}) const {
        size_t supplied = 0;
        for (const auto& kv : m) {
            bool counts = prefixes.size() == 0;
            for (const char* p : prefixes) counts = counts || kv.first.compare(0, strlen(p), p) == 0;
            supplied += counts;
        }
        if (supplied != used())
            RVCMI_FAIL(RVCMI_ERR_INVALID, "%s: %d tensors were supplied, the recognised %s has %d", who, (int)supplied, what, (int)used());
    }
};

}  // namespace rvcmi
