// deflate_bgzf_kernel (deflate.hip) for the stages of this library that compress a batch of BGZF blocks (clair_deflate_blocks; bam_sort.hip,
// whose sorted records are on the device already): the launch alone, on the caller's stream, every pointer a device pointer.  Block i of n:
// in_len[i] <= 65280 bytes at data + in_at[i], in_at[i] a multiple of 4, whole dwords readable behind the last byte -> one BGZF block in
// out[i * 65536 ..], its size in csize[i].  The caller has checked the lengths and the ranges.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace clair_def {

hipError_t launch_deflate_bgzf(hipStream_t stream, const uint8_t *data, int n, const int32_t *in_at, const int32_t *in_len, uint8_t *out, int32_t *csize);

}  // namespace clair_def
