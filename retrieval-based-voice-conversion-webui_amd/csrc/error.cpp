// The library-wide error state and version of include/rvcmi.h (error.hpp).  Plain C++: no HIP.
#include "error.hpp"

#include <cstdarg>
#include <cstdio>
#include <string>

namespace rvcmi {

static thread_local std::string g_last_error;
void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

}  // namespace rvcmi

extern "C" {

const char* rvcmi_last_error(void) { return rvcmi::g_last_error.c_str(); }
int rvcmi_version(void) { return RVCMI_VERSION; }

}  // extern "C"
