// The error path of the device stages' handles (frontend.hip, inflate.hip, deflate.hip, overlap.hip, train.hip): one formatter, one check of a
// HIP call, one check of the device number.  Host side only.  Each stage keeps a wrapper that picks the string a message goes to -- the
// handle's, or the per-process one where there is no handle (yet) -- and its *_last_error returns that string.
// (engine.hip and comm.hip keep their own: the first is part of build.csrc_digest, the second aborts its RCCL communicator on the way out.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

// fail("...", ...): the printf-style message, cut at 511 bytes, into `slot`; returns 1, what every entry point returns on failure
struct HipFail {
    std::string &slot;
    int operator()(const char *fmt, ...) const {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        slot = buf;
        return 1;
    }
};

// returns from the calling function through `fail` (a HipFail) when a HIP call does not succeed
#define CLAIR_HIP_TRY(fail, call)                                                                      \
    do {                                                                                               \
        hipError_t err__ = (call);                                                                     \
        if (err__ != hipSuccess)                                                                       \
            return (fail)("%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
    } while (0)

// 0 when `device` is one of the visible GPUs.  `only`: the stage's own sentence, what runs on an MI355X only (and where its host twin is)
inline int hip_device_check(const HipFail &fail, int device, const char *only) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1) return fail("no HIP device is visible: %s", only);
    if (device < 0 || device >= n_dev) return fail("device %d out of range [0,%d)", device, n_dev);
    return 0;
}
