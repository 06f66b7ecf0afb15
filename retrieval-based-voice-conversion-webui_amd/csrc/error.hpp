// Error reporting across the C ABI: the thread's last message (rvcmi_last_error), the exception that carries a return code, and
// the wrapper every extern "C" body runs in.  No HIP here: host-only modules (ivf_format.hpp, ivf_kmeans.hpp) and their
// stand-alone test program use it with a plain C++ compiler.  Implemented in error.cpp.
#pragma once
#include <exception>

#include "../../include/rvcmi.h"

namespace rvcmi {

void set_error(const char* fmt, ...);

struct Error {
    int code;
};

#define RVCMI_FAIL(code_, ...)            \
    do {                                  \
        ::rvcmi::set_error(__VA_ARGS__);  \
        throw ::rvcmi::Error{(code_)};    \
    } while (0)

// Every extern "C" body runs inside this so that nothing throws across the ABI.
template <typename F>
int guarded(F&& f) {
    try {
        f();
        return RVCMI_OK;
    } catch (const Error& e) {
        return e.code;
    } catch (const std::exception& e) {
        set_error("exception: %s", e.what());
        return RVCMI_ERR_INVALID;
    } catch (...) {
        set_error("unknown exception");
        return RVCMI_ERR_INVALID;
    }
}

}  // namespace rvcmi
