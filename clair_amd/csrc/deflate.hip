// clair_deflate_*: BGZF blocks compressed on the device (include/clair_amd.h).  This file holds the kernel and the handle; the compressor
// itself is csrc/deflate_core.h, shared with the host twin (hostsrc/host_deflate.cpp), whose header states the rule.  It is a translation
// unit of its own, outside the forward pass's sources (build.csrc_digest), which it does not touch.
//
// A workgroup is one wave (64 lanes) and owns one BGZF block from its first input byte to its size word: blocks are independent, no
// workgroup waits for another.  In LDS (clair_def::Work): the block's input (63.75 KiB: matches are measured in LDS, never in HBM), the hash
// table (16384 positions of 16 bits, 32 KiB), one deflate block's tokens (8192 words, 32 KiB), the staging window of output words (8 KiB),
// the CRC-32 byte table (1 KiB) and the counts, trees, codes and per-lane scratch (8.2 KiB): 144.9 KiB of the CU's 160 KiB, so one block is
// resident per CU.  Every loop is bounded by the block's length, the token count or a constant.  The lanes share the input load, the match
// measurement, the table update, the symbol counts (LDS adds), the packing of the tokens' bits (prefix sum of their lengths, words combined
// by LDS OR), the CRC-32 and the coalesced stores of whole output words; the greedy walk over a step's matches runs on values that are the same
// in every lane (one turn per token); lane 0 builds the three Huffman codes and writes the block headers.  The size word and BSIZE are ordinary vector stores by lane 0.
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>

#define CLAIR_DEF_FN __device__ inline
#define CLAIR_INF_FN __device__ inline
#define CLAIR_DEF_WAVE 1
#include "device_buffer.h"
#include "deflate_core.h"
#include "deflate_launch.h"

namespace clair_def {

struct DeviceCtx {
    Work *w;                     // LDS
    uint32_t *out32;             // the block's 64 KiB slot
    uint32_t lane_;

    __device__ Work &work() { return *w; }
    __device__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    __device__ void fence() { __threadfence(); }             // the wave's earlier stores to its slot are done before its later ones
    __device__ uint32_t uniform(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ uint32_t lane_id() const { return lane_; }
    __device__ void or_word(uint32_t *p, uint32_t v) { atomicOr(p, v); }
    __device__ void add_word(uint32_t *p, uint32_t v) { atomicAdd(p, v); }
    __device__ void store_word(uint32_t index, uint32_t v) {
        if (index < SLOT / 4) out32[index] = v;
    }
    __device__ void store_bsize(uint32_t v) { ((uint16_t *)out32)[8] = (uint16_t)v; }
};

// grid: one workgroup of 64 per block.  in_at: 4-byte aligned offsets into data, in_len <= 65280 (checked by the host); data is padded so that
// whole dwords can be read; out: n slots of 64 KiB.
__global__ __launch_bounds__(64) void deflate_bgzf_kernel(const uint8_t *__restrict__ data, int n, const int32_t *__restrict__ in_at,
                                                           const int32_t *__restrict__ in_len, uint8_t *__restrict__ out, int32_t *__restrict__ csize) {
    __shared__ __attribute__((aligned(16))) Work work;
    const int b = (int)blockIdx.x;
    if (b >= n) return;
    const uint32_t lane = threadIdx.x;
    uint32_t len = (uint32_t)in_len[b];
    if (len > MAX_IN) len = MAX_IN;
    const uint32_t *src = (const uint32_t *)(data + in_at[b]);
    for (uint32_t j = lane; j * 4 < len; j += LANES) work.in32[j] = src[j];

    DeviceCtx c;
    c.w = &work;
    c.out32 = (uint32_t *)(out + (size_t)b * SLOT);
    c.lane_ = lane;
    c.sync();
    const uint32_t cs = deflate_bgzf(c, len);
    if (lane == 0) csize[b] = (int32_t)cs;
}

hipError_t launch_deflate_bgzf(hipStream_t stream, const uint8_t *data, int n, const int32_t *in_at, const int32_t *in_len, uint8_t *out, int32_t *csize) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(deflate_bgzf_kernel, dim3((unsigned)n), dim3(64), 0, stream, data, n, in_at, in_len, out, csize);
    return hipGetLastError();
}

}  // namespace clair_def

// -- the handle: a StagedStream sized from max_blocks at creation
#include <cstring>

#include "staged_stream.h"

struct clair_deflate : StagedStream {};

namespace {

constexpr int64_t DEF_MAX_IN = clair_def::MAX_IN, DEF_SLOT = clair_def::SLOT;
// per block: in_at, in_len, csize (int32)
constexpr int64_t DEF_META_PER_BLOCK = 3 * 4;

std::string g_def_error;
inline HipFail def_fail(clair_deflate *h) { return {h ? h->error : g_def_error}; }

}  // namespace

extern "C" {

const char *clair_deflate_last_error(const clair_deflate_t *h) { return h ? h->error.c_str() : g_def_error.c_str(); }

int clair_deflate_create(int device, int max_blocks, clair_deflate_t **out) {
    if (!out) return def_fail(nullptr)("out is NULL");
    *out = nullptr;
    if (max_blocks < 1 || max_blocks > 16384) return def_fail(nullptr)("max_blocks %d: 1 .. 16384", max_blocks);
    if (hip_device_check(def_fail(nullptr), device, "the device deflate runs on an MI355X only (the host deflate is --bgzf_deflate host)")) return 1;
    clair_deflate *h = new clair_deflate;
    const size_t in_cap = (size_t)max_blocks * DEF_MAX_IN + 16;      // (+ 16: the kernel reads whole dwords)
    if (h->open(def_fail(nullptr), device, max_blocks, in_cap, (size_t)max_blocks * DEF_SLOT, (size_t)max_blocks * DEF_META_PER_BLOCK, in_cap)) {
        clair_deflate_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}

void clair_deflate_destroy(clair_deflate_t *h) {
    if (!h) return;
    h->close();
    delete h;
}

int clair_deflate_blocks(clair_deflate_t *h, const uint8_t *data, int64_t bytes, int n, const int64_t *in_at, const int32_t *in_len,
                         uint8_t *out, int32_t *csize) {
    if (!h) return def_fail(nullptr)("deflate handle is NULL");
    if (n < 0 || n > h->max_blocks) return def_fail(h)("%d blocks in a batch: 0 .. max_blocks = %d", n, h->max_blocks);
    if (n == 0) return 0;
    if (!in_at || !in_len || !out || !csize || (!data && bytes > 0)) return def_fail(h)("NULL argument");
    if (bytes < 0) return def_fail(h)("%lld bytes of data", (long long)bytes);
    for (int i = 0; i < n; ++i) {
        if (in_len[i] < 0 || in_len[i] > DEF_MAX_IN) return def_fail(h)("block %d: %d bytes (0 .. 65280)", i, in_len[i]);
        if (in_at[i] < 0 || in_at[i] > bytes - in_len[i]) return def_fail(h)("block %d: bytes [%lld, +%d) outside the %lld given", i, (long long)in_at[i], in_len[i], (long long)bytes);
    }
    CLAIR_HIP_TRY(def_fail(h), hipSetDevice(h->device));
    const size_t N = (size_t)h->max_blocks;
    int32_t *m_at = h->h_meta.as<int32_t>(), *m_len = m_at + N, *m_csize = m_len + N;
    uint8_t *h_in = h->h_in.as<uint8_t>(), *h_out = h->h_out.as<uint8_t>();
    int64_t total = 0;                           // the blocks' bytes packed at 4-byte boundaries: at most n * 65280
    for (int i = 0; i < n; ++i) {
        m_at[i] = (int32_t)total;
        m_len[i] = in_len[i];
        if (in_len[i]) memcpy(h_in + total, data + in_at[i], (size_t)in_len[i]);
        total += ((int64_t)in_len[i] + 3) & ~(int64_t)3;
    }
    int32_t *d_at = h->d_meta.as<int32_t>(), *d_len = d_at + N, *d_csize = d_len + N;
    if (total) CLAIR_HIP_TRY(def_fail(h), hipMemcpyAsync(h->d_in.p, h_in, (size_t)total, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(def_fail(h), hipMemcpyAsync(h->d_meta.p, h->h_meta.p, N * 2 * 4, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(def_fail(h), clair_def::launch_deflate_bgzf(h->stream, h->d_in.as<const uint8_t>(), n, d_at, d_len, h->d_out.as<uint8_t>(), d_csize));
    CLAIR_HIP_TRY(def_fail(h), hipMemcpyAsync(h_out, h->d_out.p, (size_t)n * DEF_SLOT, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(def_fail(h), hipMemcpyAsync(m_csize, d_csize, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(def_fail(h), hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) {
        const int32_t cs = m_csize[i];
        if (cs < 26 || cs > DEF_SLOT) return def_fail(h)("block %d: the kernel reports %d bytes", i, cs);
        csize[i] = cs;
        memcpy(out + (size_t)i * DEF_SLOT, h_out + (size_t)i * DEF_SLOT, (size_t)cs);
        memset(out + (size_t)i * DEF_SLOT + cs, 0, (size_t)(DEF_SLOT - cs));
    }
    return 0;
}

}  // extern "C"
