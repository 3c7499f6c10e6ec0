// rtm_host.h — what the host side of every entry point does alike where it needs HIP: turn a failed HIP call into a refusal,
// select the device, ask whether the launches it queued were accepted.  Host-only inline functions, no device code; included
// by the .hip units next to rtm_internal.h (which holds the refusals themselves: fail, invalid, unsupported).  What is a stage's own (its parameter ranges, aliasing rules, size limits and their messages) stays in
// the stage's file.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "rtm_internal.h"

namespace rtm {

// (fail / invalid / unsupported, which need nothing of HIP: rtm_internal.h)
// `expr` is a HIP call: on failure, its text and HIP's message become the last error and the function returns RTM_ERR_HIP
#define RTM_HIP_CHECK(expr)                                                                  \
    do {                                                                                     \
        const hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) {                                                             \
            (void)hipGetLastError(); /* do not leave a sticky error for the host app */     \
            return ::rtm::fail(RTM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__)); \
        }                                                                                    \
    } while (0)

// hipSetDevice for a stage call that keeps no state
inline int use_device(int device) {
    const hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) return RTM_OK;
    (void)hipGetLastError();  // do not leave a sticky error for the host app
    return fail(RTM_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
}

// after a call's launches: RTM_OK, or "<stage> kernel launch: <HIP's message>"
inline int launched(const char* stage) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return RTM_OK;
    return fail(RTM_ERR_HIP, std::string(stage) + " kernel launch: " + hipGetErrorString(e));
}

// the alignment asked of the work buffers that are carved into parts
inline bool aligned256(const void* p) { return ((uintptr_t)p & 255) == 0; }

}  // namespace rtm
