// Allocations that are freed with their owner: what the handles of engine.hip, frontend.hip and inflate.hip hold.  Host side only; kernels take
// plain pointers (as<T>()).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

struct DeviceMemory {
    static hipError_t get(void **p, size_t n) { return hipMalloc(p, n); }
    static hipError_t give(void *p) { return hipFree(p); }
};
struct PinnedMemory {
    static hipError_t get(void **p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
    static hipError_t give(void *p) { return hipHostFree(p); }
};

template <typename Memory> struct OwnedBuffer {
    void *p = nullptr;
    size_t bytes = 0;
    OwnedBuffer() = default;
    OwnedBuffer(const OwnedBuffer &) = delete;
    OwnedBuffer &operator=(const OwnedBuffer &) = delete;
    ~OwnedBuffer() { reset(); }
    void reset() { if (p) (void)Memory::give(p); p = nullptr; bytes = 0; }
    hipError_t ensure(size_t n) {      // exactly n bytes (at least one): kept when it has them, freed and allocated anew when the size changes
        n = std::max<size_t>(n, 1);
        if (p && bytes == n) return hipSuccess;
        reset();
        const hipError_t e = Memory::get(&p, n);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    template <typename T> T *as() const { return (T *)p; }
};
using DeviceBuffer = OwnedBuffer<DeviceMemory>;   // a device allocation
using PinnedBuffer = OwnedBuffer<PinnedMemory>;   // its page-locked twin on the host
