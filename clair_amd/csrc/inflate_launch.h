// inflate_bgzf_kernel (inflate.hip) for another stage of this library that keeps the inflated bytes on the device (bam_index.hip): the launch
// alone, on the caller's stream, every pointer a device pointer.  The caller has checked what clair_inflate_blocks checks (csize 26 .. 65536,
// out_len 0 .. 65536, both ranges inside their buffers) and leaves 32 readable bytes behind the compressed data.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace clair_inf {

hipError_t launch_bgzf(hipStream_t stream, const uint8_t *cdata, int n, const int64_t *in_at, const int32_t *csize, const int64_t *out_at,
                       const int32_t *out_len, uint8_t *out, int32_t *status);

}  // namespace clair_inf
