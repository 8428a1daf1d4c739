// clair_inflate_*: BGZF blocks inflated on the device (include/clair_amd.h).  This file holds the kernel and the handle; the decoder itself
// is csrc/inflate_core.h, shared with the host twin (hostsrc/host_inflate.cpp).  It is a translation unit of its own, outside the
// forward pass's sources (build.csrc_digest), which it does not touch.
//
// A workgroup is one wave (64 lanes) and owns one BGZF block from its first compressed byte to its status word: blocks are independent, no
// workgroup waits for another.  In LDS: the block's whole output (64 KiB: matches are read from LDS, never from HBM), the Huffman tables
// (Tables, 5.2 KiB), a 2 KiB ring of compressed bytes the wave fills 1 KiB at a time with one 16-byte load per lane, and the CRC-32 byte table
// (1 KiB): 72.3 KiB, so two blocks are resident per CU (160 KiB).  Every lane runs the symbol loop on the same values (the values that
// steer it pass through readfirstlane, so the loop's state lives in scalar registers and its branches are scalar); lane 0 stores literals;
// the lanes share table construction, match and stored-block copies, the CRC-32 (a chunk per lane, combined modulo the polynomial) and the
// coalesced store of the block to global memory.  The status word is an ordinary vector store by lane 0.
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>

#define CLAIR_INF_FN __device__ inline
#include "device_buffer.h"
#include "inflate_core.h"

namespace clair_inf {

constexpr uint32_t RING_WORDS = 512, CHUNK_WORDS = 256;      // two chunks of 1 KiB
constexpr uint32_t WINDOW = 65536;

struct DeviceCtx {
    const uint8_t *base;         // the 16-byte boundary at or below the deflate stream (inside the block's own 18-byte header)
    uint32_t n_in;               // bytes from base to the stream's end
    uint32_t lo_chunk;           // the ring holds chunks lo_chunk and lo_chunk + 1
    uint8_t *win;                // LDS
    uint32_t *ring;              // LDS
    Tables *t;                   // LDS
    uint32_t lane_;

    __device__ void sync() {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
    __device__ uint32_t uniform(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ uint32_t lane() const { return lane_; }
    __device__ uint32_t lanes() const { return 64; }
    __device__ Tables &tables() { return *t; }

    // chunk -> its half of the ring: 16 bytes per lane, zeros from the 16-byte boundary above the stream's end on (the handle pads its buffer)
    __device__ void load_chunk(uint32_t chunk) {
        const uint32_t at = chunk * (CHUNK_WORDS * 4) + lane_ * 16;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (at < n_in) v = *(const uint4 *)(base + at);
        *(uint4 *)(ring + (chunk & 1) * CHUNK_WORDS + lane_ * 4) = v;
    }
    __device__ uint32_t word(uint32_t i) {                   // i * 4 < n_in (need())
        const uint32_t chunk = i / CHUNK_WORDS;
        if (chunk != lo_chunk) {
            sync();
            if (chunk != lo_chunk + 1) load_chunk(chunk);
            load_chunk(chunk + 1);
            lo_chunk = chunk;
            sync();
        }
        uint32_t w = uniform(ring[i & (RING_WORDS - 1)]);
        const uint32_t over = i * 4 + 4 > n_in ? i * 4 + 4 - n_in : 0;     // 0 .. 3 bytes beyond the stream
        if (over) w &= 0xffffffffu >> (8 * over);
        return w;
    }
    __device__ void put(uint32_t pos, uint32_t byte) {
        if (lane_ == 0 && pos < WINDOW) win[pos] = (uint8_t)byte;
    }
    __device__ void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        sync();
        for (uint32_t k = lane_; k < len; k += 64) {
            const uint32_t from = pos - dist + (k < dist ? k : k % dist);   // below pos: bytes that are final
            if (pos + k < WINDOW) win[pos + k] = win[from];
        }
        sync();
    }
    __device__ void stored(uint32_t pos, uint32_t at, uint32_t len) {        // at + len <= n_in
        for (uint32_t k = lane_; k < len; k += 64)
            if (pos + k < WINDOW) win[pos + k] = base[at + k];
        sync();
    }
};

// grid: one workgroup of 64 per block.  in_at / csize: the whole BGZF block inside cdata (csize >= 26, checked by the host); out_len <= 65536.
__global__ __launch_bounds__(64) void inflate_bgzf_kernel(const uint8_t *__restrict__ cdata, int n, const int64_t *__restrict__ in_at,
                                                           const int32_t *__restrict__ csize, const int64_t *__restrict__ out_at,
                                                           const int32_t *__restrict__ out_len, uint8_t *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ __attribute__((aligned(16))) uint32_t win32[WINDOW / 4];
    __shared__ __attribute__((aligned(16))) uint32_t ring[RING_WORDS];
    __shared__ uint32_t crc_table[256];
    __shared__ Tables tables;
    const int b = (int)blockIdx.x;
    if (b >= n) return;
    const uint32_t lane = threadIdx.x;
    const uint8_t *block = cdata + in_at[b];
    const uint32_t cs = (uint32_t)csize[b], isize = (uint32_t)out_len[b];
    const uint8_t *stream = block + 18;
    const uint32_t skew = (uint32_t)((uintptr_t)stream & 15);
    for (uint32_t i = lane; i < 256; i += 64) crc_table[i] = crc_table_entry(i);

    DeviceCtx c;
    c.base = stream - skew;
    c.n_in = skew + cs - 26;
    c.win = (uint8_t *)win32;
    c.ring = ring;
    c.t = &tables;
    c.lane_ = lane;
    c.lo_chunk = skew / (CHUNK_WORDS * 4);       // 0
    c.load_chunk(c.lo_chunk);
    c.load_chunk(c.lo_chunk + 1);
    c.sync();

    uint32_t produced = 0;
    const bool ended = inflate(c, skew, c.n_in, isize + 1, &produced);
    c.sync();

    uint32_t crc = 0;
    const uint32_t want = (uint32_t)block[cs - 8] | (uint32_t)block[cs - 7] << 8 | (uint32_t)block[cs - 6] << 16 | (uint32_t)block[cs - 5] << 24;
    if (ended && produced == isize) {
        const uint8_t *win = c.win;
        const auto byte_at = [win](uint32_t i) { return (uint32_t)win[i]; };
        uint32_t share = crc_lane_share(byte_at, crc_table, produced, lane, 64);
        if (lane == 0) share ^= crc_init_share(produced);
        for (int off = 32; off > 0; off >>= 1) share ^= (uint32_t)__shfl_xor((int)share, off, 64);
        crc = ~share;
    }
    const int st = bgzf_status(ended, produced, isize, crc, want);
    if (lane == 0) status[b] = st;

    // the block to global memory: bytes up to the first 4-byte boundary of the destination, whole dwords, the tail's bytes
    const uint32_t count = ended ? (produced < isize ? produced : isize) : 0;
    uint8_t *dst = out + out_at[b];
    const uint32_t head = (uint32_t)(-(intptr_t)dst & 3) < count ? (uint32_t)(-(intptr_t)dst & 3) : count;
    const uint32_t dwords = (count - head) / 4, tail_at = head + dwords * 4;
    if (lane < head) dst[lane] = c.win[lane];
    uint32_t *dst32 = (uint32_t *)(dst + head);
    for (uint32_t j = lane; j < dwords; j += 64) {
        const uint32_t lo = win32[j], hi = j + 1 < WINDOW / 4 ? win32[j + 1] : 0u;   // bytes [4j + head, 4j + head + 4) of the window
        dst32[j] = head ? (lo >> (8 * head)) | (hi << (32 - 8 * head)) : lo;
    }
    if (lane < count - tail_at) dst[tail_at + lane] = c.win[tail_at + lane];
}

}  // namespace clair_inf

#include "inflate_launch.h"

hipError_t clair_inf::launch_bgzf(hipStream_t stream, const uint8_t *cdata, int n, const BlockMeta &meta, uint8_t *out) {
    hipLaunchKernelGGL(inflate_bgzf_kernel, dim3((unsigned)n), dim3(64), 0, stream, cdata, n, (const int64_t *)meta.in_at, (const int32_t *)meta.csize,
                       (const int64_t *)meta.out_at, (const int32_t *)meta.out_len, out, meta.status);
    return hipGetLastError();
}

// -- the handle: a StagedStream sized from max_blocks at creation
#include <cstring>

#include "staged_stream.h"

struct clair_inflate : StagedStream {
    int64_t cap = 0;                             // bytes of each data buffer: max_blocks * BLOCK_MAX
};

namespace {

constexpr int64_t BLOCK_MAX = 65536;             // a BGZF block, compressed or inflated

std::string g_inf_error;
inline HipFail inf_fail(clair_inflate *h) { return {h ? h->error : g_inf_error}; }

}  // namespace

extern "C" {

const char *clair_inflate_last_error(const clair_inflate_t *h) { return h ? h->error.c_str() : g_inf_error.c_str(); }

int clair_inflate_create(int device, int max_blocks, clair_inflate_t **out) {
    if (!out) return inf_fail(nullptr)("out is NULL");
    *out = nullptr;
    if (max_blocks < 1 || max_blocks > 16384) return inf_fail(nullptr)("max_blocks %d: 1 .. 16384", max_blocks);
    if (hip_device_check(inf_fail(nullptr), device, "the device inflate runs on an MI355X only (the host inflate is --bam_inflate host)")) return 1;
    clair_inflate *h = new clair_inflate;
    h->cap = (int64_t)max_blocks * BLOCK_MAX;
    const size_t meta = (size_t)max_blocks * clair_inf::META_PER_BLOCK;
    // (d_in + 32: the kernel reads whole 16-byte pieces around each stream)
    if (h->open(inf_fail(nullptr), device, max_blocks, (size_t)h->cap, (size_t)h->cap, meta, (size_t)h->cap + 32)) {
        clair_inflate_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}

void clair_inflate_destroy(clair_inflate_t *h) {
    if (!h) return;
    h->close();
    delete h;
}

int clair_inflate_blocks(clair_inflate_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                         const int64_t *out_at, const int32_t *out_len, uint8_t *out, int32_t *status) {
    if (!h) return inf_fail(nullptr)("inflate handle is NULL");
    if (n > 0 && (!cdata || !in_at || !csize || !out_at || !out_len || !out || !status)) return inf_fail(h)("NULL argument");
    if (n > 0 && (cbytes < 0 || cbytes > h->cap)) return inf_fail(h)("%lld compressed bytes: 0 .. %lld", (long long)cbytes, (long long)h->cap);
    if (clair_inf::check_blocks(inf_fail(h), n, h->max_blocks, cbytes, in_at, csize, out_len)) return 1;
    if (n == 0) return 0;
    int64_t out_lo = INT64_MAX, out_hi = 0;
    for (int i = 0; i < n; ++i) {
        if (out_at[i] < 0 || out_at[i] > h->cap - out_len[i]) return inf_fail(h)("block %d: output [%lld, +%d) outside the handle's %lld bytes", i, (long long)out_at[i], out_len[i], (long long)h->cap);
        out_lo = std::min(out_lo, out_at[i]);
        out_hi = std::max(out_hi, out_at[i] + out_len[i]);
    }
    CLAIR_HIP_TRY(inf_fail(h), hipSetDevice(h->device));
    const size_t N = (size_t)h->max_blocks;
    const clair_inf::BlockMeta m = clair_inf::carve_meta(h->h_meta.p, N), d = clair_inf::carve_meta(h->d_meta.p, N);
    uint8_t *h_in = h->h_in.as<uint8_t>(), *h_out = h->h_out.as<uint8_t>(), *d_in = h->d_in.as<uint8_t>(), *d_out = h->d_out.as<uint8_t>();
    memcpy(h_in, cdata, (size_t)cbytes);
    memcpy(m.in_at, in_at, (size_t)n * 8);
    memcpy(m.out_at, out_at, (size_t)n * 8);
    memcpy(m.csize, csize, (size_t)n * 4);
    memcpy(m.out_len, out_len, (size_t)n * 4);
    CLAIR_HIP_TRY(inf_fail(h), hipMemcpyAsync(d_in, h_in, (size_t)cbytes, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(inf_fail(h), hipMemcpyAsync(h->d_meta.p, h->h_meta.p, N * clair_inf::META_FILLED, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(inf_fail(h), clair_inf::launch_bgzf(h->stream, d_in, n, d, d_out));
    if (out_hi > out_lo) CLAIR_HIP_TRY(inf_fail(h), hipMemcpyAsync(h_out + out_lo, d_out + out_lo, (size_t)(out_hi - out_lo), hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(inf_fail(h), hipMemcpyAsync(m.status, d.status, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(inf_fail(h), hipStreamSynchronize(h->stream));
    for (int i = 0; i < n; ++i) {
        status[i] = m.status[i];
        if (m.status[i] == 0 && out_len[i]) memcpy(out + out_at[i], h_out + out_at[i], (size_t)out_len[i]);
    }
    return 0;
}

int clair_inflate_blocks_cb(void *handle, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                            const int64_t *out_at, const int32_t *out_len, uint8_t *out, int32_t *status) {
    return clair_inflate_blocks((clair_inflate_t *)handle, cdata, cbytes, n, in_at, csize, out_at, out_len, out, status);
}

}  // extern "C"
