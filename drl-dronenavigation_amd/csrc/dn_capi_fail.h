// dn_capi_fail.h -- how the host units of the C ABI (dn_capi.cpp, dn_capi_envfree.cpp) refuse a call: a dn_status code and the
// thread-local message that dn_last_error returns.  The message buffer and fail() are defined once, in dn_capi.cpp.
#pragma once

#include "../../include/dronenav.h"

#include <hip/hip_runtime.h>

// Writes the calling thread's message (printf form) and returns st, so that a check reads `return fail(...)`.
__attribute__((visibility("hidden"))) int32_t fail(dn_status st, const char *fmt, ...);

// The message quotes the failing expression: keep launches written out inside DN_HIP(...), not behind a helper.
#define DN_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail(e_ == hipErrorOutOfMemory ? DN_ERR_OUT_OF_MEMORY : DN_ERR_HIP, "%s failed: %s", #expr, \
                        hipGetErrorString(e_));                                                   \
    } while (0)
