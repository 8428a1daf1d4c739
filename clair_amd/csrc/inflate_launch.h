// inflate_bgzf_kernel (inflate.hip) for the stages of this library that inflate a batch of blocks (clair_inflate_blocks; bam_index.hip, which
// keeps the inflated bytes on the device): the per-block arrays of a batch as one layout, and the launch alone, on the caller's stream, every
// pointer a device pointer.  The caller has checked the batch (check_blocks, inflate_core.h: csize 26 .. 65536, out_len 0 .. 65536, the
// compressed ranges inside their buffer), and the output ranges, and leaves 32 readable bytes behind the compressed data.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace clair_inf {

// the arrays of a batch of up to N blocks, carved from one 8-byte-aligned buffer of N * META_PER_BLOCK bytes: what the host fills
// (the first N * META_FILLED bytes) in front, the status words the kernel writes behind
constexpr size_t META_FILLED = 2 * 8 + 2 * 4, META_PER_BLOCK = META_FILLED + 4;
struct BlockMeta {
    int64_t *in_at, *out_at;
    int32_t *csize, *out_len, *status;
};
inline BlockMeta carve_meta(void *base, size_t N) {
    BlockMeta m;
    m.in_at = (int64_t *)base;
    m.out_at = m.in_at + N;
    m.csize = (int32_t *)(m.out_at + N);
    m.out_len = m.csize + N;
    m.status = m.out_len + N;
    return m;
}

hipError_t launch_bgzf(hipStream_t stream, const uint8_t *cdata, int n, const BlockMeta &meta, uint8_t *out);

}  // namespace clair_inf
