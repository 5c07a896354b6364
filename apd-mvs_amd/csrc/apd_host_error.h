// apd_host_error.h -- how the library's host code reports an error: the message goes into the caller's thread-local string (the C
// ABI's, the exchange's or the fusions': three strings, three getters), the code is returned.
#pragma once

#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdio.h>

#include <string>

namespace apd {

// slot = the printf-formatted message; returns code, so that `return set_error(...)` is the whole error path
__attribute__((format(printf, 3, 4))) inline int set_error(std::string &slot, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    slot = buf;
    return code;
}

}  // namespace apd

// Returns from the enclosing function when a HIP call fails, with what `hip_failed(expr, error, file, line)` returns.  hip_failed
// is whatever that name means at the point of use: a function of the file (C ABI, exchange: "<expr> failed: <hip string>
// (<file>:<line>)") or a member of the fusion call ("<entry point>: <expr>: <hip string>").  Both end in set_error.
// The runtime also keeps a failed call's error for the thread's next hipGetLastError(), which is how every launch here is checked:
// it is taken here, or the refused call (apd_device_memory of a device that does not exist) fails the thread's next launch
// (apd_image_create: "invalid device ordinal") -- tests/test_gpu_exchange_shapes.py.
#define HIP_TRY(expr)                                                 \
    do {                                                              \
        hipError_t e_ = (expr);                                       \
        if (e_ != hipSuccess) {                                       \
            (void)hipGetLastError();                                  \
            return hip_failed(#expr, e_, __FILE__, __LINE__);         \
        }                                                             \
    } while (0)
