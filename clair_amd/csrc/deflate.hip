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

}  // namespace clair_def

// -- the handle: one stream, page-locked staging for both directions and the device buffers, sized from max_blocks at creation and reused
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

namespace {

constexpr int64_t DEF_MAX_IN = clair_def::MAX_IN, DEF_SLOT = clair_def::SLOT;
std::string g_def_error;

}  // namespace

struct clair_deflate {
    int device = 0;
    int max_blocks = 0;
    hipStream_t stream = nullptr;
    PinnedBuffer h_in, h_out, h_meta;
    DeviceBuffer d_in, d_out, d_meta;
    std::string error;
};

namespace {

int def_fail(clair_deflate *h, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->error = buf; else g_def_error = buf;
    return 1;
}

#define DEF_TRY(h, call)                                                                                   \
    do {                                                                                                   \
        hipError_t err__ = (call);                                                                         \
        if (err__ != hipSuccess)                                                                           \
            return def_fail((h), "%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
    } while (0)

// per block: in_at, in_len, csize (int32)
constexpr int64_t DEF_META_PER_BLOCK = 3 * 4;

int deflate_init(clair_deflate *h) {
    DEF_TRY(nullptr, hipSetDevice(h->device));
    DEF_TRY(nullptr, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    const size_t in_cap = (size_t)h->max_blocks * DEF_MAX_IN + 16, out_cap = (size_t)h->max_blocks * DEF_SLOT;
    const size_t meta = (size_t)h->max_blocks * DEF_META_PER_BLOCK;
    DEF_TRY(nullptr, h->h_in.ensure(in_cap));
    DEF_TRY(nullptr, h->h_out.ensure(out_cap));
    DEF_TRY(nullptr, h->h_meta.ensure(meta));
    DEF_TRY(nullptr, h->d_in.ensure(in_cap));                // the kernel reads whole dwords
    DEF_TRY(nullptr, h->d_out.ensure(out_cap));
    DEF_TRY(nullptr, h->d_meta.ensure(meta));
    DEF_TRY(nullptr, hipMemsetAsync(h->d_in.p, 0, in_cap, h->stream));       // on the handle's own stream: ordered before its first copy
    return 0;
}

}  // namespace

extern "C" {

const char *clair_deflate_last_error(const clair_deflate_t *h) { return h ? h->error.c_str() : g_def_error.c_str(); }

int clair_deflate_create(int device, int max_blocks, clair_deflate_t **out) {
    if (!out) return def_fail(nullptr, "out is NULL");
    *out = nullptr;
    if (max_blocks < 1 || max_blocks > 16384) return def_fail(nullptr, "max_blocks %d: 1 .. 16384", max_blocks);
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1)
        return def_fail(nullptr, "no HIP device is visible: the device deflate runs on an MI355X only (the host deflate is --bgzf_deflate host)");
    if (device < 0 || device >= n_dev) return def_fail(nullptr, "device %d out of range [0,%d)", device, n_dev);
    clair_deflate *h = new clair_deflate;
    h->device = device;
    h->max_blocks = max_blocks;
    if (deflate_init(h)) {
        clair_deflate_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}

void clair_deflate_destroy(clair_deflate_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (DeviceBuffer *b : {&h->d_in, &h->d_out, &h->d_meta}) b->reset();     // before the stream goes, not in ~clair_deflate
    for (PinnedBuffer *b : {&h->h_in, &h->h_out, &h->h_meta}) b->reset();
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int clair_deflate_blocks(clair_deflate_t *h, const uint8_t *data, int64_t bytes, int n, const int64_t *in_at, const int32_t *in_len,
                         uint8_t *out, int32_t *csize) {
    if (!h) return def_fail(nullptr, "deflate handle is NULL");
    if (n < 0 || n > h->max_blocks) return def_fail(h, "%d blocks in a batch: 0 .. max_blocks = %d", n, h->max_blocks);
    if (n == 0) return 0;
    if (!in_at || !in_len || !out || !csize || (!data && bytes > 0)) return def_fail(h, "NULL argument");
    if (bytes < 0) return def_fail(h, "%lld bytes of data", (long long)bytes);
    for (int i = 0; i < n; ++i) {
        if (in_len[i] < 0 || in_len[i] > DEF_MAX_IN) return def_fail(h, "block %d: %d bytes (0 .. 65280)", i, in_len[i]);
        if (in_at[i] < 0 || in_at[i] > bytes - in_len[i]) return def_fail(h, "block %d: bytes [%lld, +%d) outside the %lld given", i, (long long)in_at[i], in_len[i], (long long)bytes);
    }
    DEF_TRY(h, hipSetDevice(h->device));
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
    if (total) DEF_TRY(h, hipMemcpyAsync(h->d_in.p, h_in, (size_t)total, hipMemcpyHostToDevice, h->stream));
    DEF_TRY(h, hipMemcpyAsync(h->d_meta.p, h->h_meta.p, N * 2 * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(clair_def::deflate_bgzf_kernel, dim3((unsigned)n), dim3(64), 0, h->stream, h->d_in.as<const uint8_t>(), n, (const int32_t *)d_at,
                       (const int32_t *)d_len, h->d_out.as<uint8_t>(), d_csize);
    DEF_TRY(h, hipGetLastError());
    DEF_TRY(h, hipMemcpyAsync(h_out, h->d_out.p, (size_t)n * DEF_SLOT, hipMemcpyDeviceToHost, h->stream));
    DEF_TRY(h, hipMemcpyAsync(m_csize, d_csize, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    DEF_TRY(h, hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) {
        const int32_t cs = m_csize[i];
        if (cs < 26 || cs > DEF_SLOT) return def_fail(h, "block %d: the kernel reports %d bytes", i, cs);
        csize[i] = cs;
        memcpy(out + (size_t)i * DEF_SLOT, h_out + (size_t)i * DEF_SLOT, (size_t)cs);
        memset(out + (size_t)i * DEF_SLOT + cs, 0, (size_t)(DEF_SLOT - cs));
    }
    return 0;
}

}  // extern "C"
