// What the stages that order BAM records on the device share (bam_sort.hip, markdup.hip): the stable radix sort over 64-bit keys, the scan
// policy that counts kept records and their bytes, the unaligned wave-per-record copy, and (host side) the output cut into payloads
// (PayloadOut, emit_payloads).  Device translation units only; the kernels have
// internal linkage, so that every translation unit that includes this header carries its own.
//
//   the radix sort   stable, least significant digit first, 8 bits a pass over (key, uint32 index) pairs in ping-pong buffers.
//                    radix_prep_kernel writes the indices and ORs key ^ key[0] over all keys (wave shuffles, one atomicOr a wave): a pass
//                    whose digit is the same in every key is skipped.  A pass: radix_hist_kernel counts the digits of a tile of
//                    256 threads x 8 keys in LDS (256 counters, 1 KiB; integer adds, so the counts do not depend on their order) and writes
//                    them digit-major, hist[digit][tile]; the scan makes them exclusive; radix_scatter_kernel re-reads the tile and writes
//                    each pair to base[digit][tile] + rank.  rank is a pure function of the tile's contents: wave w owns keys
//                    [512 w, 512 w + 512) of the tile in 8 rounds of 64 consecutive keys (coalesced 8-byte loads); in a round the lanes
//                    with equal digits find each other by eight __ballot's, a key's rank is the wave's running counter of its digit plus
//                    the popcount of the matching lanes below it, and the highest matching lane adds the match count to the counter; after
//                    a barrier thread d turns the four waves' counters of digit d into running offsets, in wave order.  LDS: 4 waves x 256
//                    counters x 4 B = 4 KiB, no staging (keys and ranks stay in registers).  Access pattern: a round reads and writes
//                    count[w][digit], one dword per lane at a data-dependent bank (digit mod 32 for the write, lanes with one digit
//                    broadcast on the read); the offsets pass reads and writes consecutive dwords by consecutive lanes.
//   the copy         copy_kernel, a wave per record.  A copy writes bytes [dst, dst + len) and no other: single bytes up to the first 4-byte
//                    boundary of the destination and behind the last, whole dwords between, each put together from the two aligned source
//                    dwords it straddles (reads may reach 3 bytes around the source record, inside its buffer's padding; never writes).
//                    The loop is bounded by the record's length.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "bam_front.h"
#include "bam_sort_core.h"
#include "deflate_launch.h"
#include "device_buffer.h"
#include "device_scan.h"
#include "hip_status.h"

namespace clair_bsort {

constexpr int SCAN_ITEMS = 4;                    // of the scans: 1024 items per workgroup
constexpr int64_t SCAN_BLOCK = 256 * SCAN_ITEMS;
constexpr int WAVE_KEYS = 64 * RADIX_ITEMS;      // keys of a tile one wave owns

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

// ---- compaction: how many records are kept before this one, and how many bytes they hold
struct Kept {
    uint32_t n, pad;
    int64_t bytes;
};
struct KeepScan {
    using T = Kept;
    const uint8_t *keep;
    const uint32_t *len;
    static __device__ inline T identity() { return T{0, 0, 0}; }
    static __device__ inline T join(T a, T b) { return T{a.n + b.n, 0, a.bytes + b.bytes}; }
    static __device__ inline T up(T x, int d) { return T{__shfl_up(x.n, d, 64), 0, (int64_t)__shfl_up((long long)x.bytes, d, 64)}; }
    __device__ inline T item(int64_t i) const { return keep[i] ? T{1, 0, (int64_t)len[i]} : T{0, 0, 0}; }
};
template <typename P> struct WriteBefore {       // out[i] = the sum of the items before i
    static constexpr int PAST_END = 0;
    typename P::T *out;
    static __device__ inline typename P::T seed() { return 0; }
    __device__ inline void write(const P &, int64_t i, int64_t, typename P::T before, typename P::T) const { out[i] = before; }
};

// ---- the copy.  Record i of n: len_of[r] bytes from src + src_at[r], r = index[i] (i itself when index is NULL), to dst + dst_at[i]; a
// negative dst_at[i] or an index[i] >= n copies nothing.  grid: a wave per record, four to a workgroup.
__device__ inline void copy_record(const uint8_t *src, uint8_t *dst, uint32_t len, uint32_t lane) {
    uint32_t head = (uint32_t)((4 - ((uintptr_t)dst & 3)) & 3);
    if (head > len) head = len;
    const uint32_t words = (len - head) >> 2, tail_at = head + (words << 2);
    if (lane < head) dst[lane] = src[lane];
    const uintptr_t s0 = (uintptr_t)(src + head);
    const uint32_t shift = (uint32_t)(s0 & 3) * 8;
    const uint32_t *sa = (const uint32_t *)(s0 & ~(uintptr_t)3);
    uint32_t *da = (uint32_t *)(dst + head);
    if (shift == 0) {
        for (uint32_t j = lane; j < words; j += 64) da[j] = sa[j];
    } else {
        for (uint32_t j = lane; j < words; j += 64) da[j] = sa[j] >> shift | sa[j + 1] << (32 - shift);
    }
    if (lane < len - tail_at) dst[tail_at + lane] = src[tail_at + lane];
}
static __global__ __launch_bounds__(256) void copy_kernel(const uint8_t *src, const int64_t *__restrict__ src_at, const uint32_t *__restrict__ index,
                                                          const uint32_t *__restrict__ len_of, const int64_t *__restrict__ dst_at, int64_t n, uint8_t *dst) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int64_t d = dst_at[i];
    if (d < 0) return;
    const int64_t r = index ? (int64_t)index[i] : i;
    if (r >= n) return;
    copy_record(src + src_at[r], dst + d, len_of[r], threadIdx.x & 63);
}

// ---- the radix sort
__device__ inline uint32_t digit_of(uint64_t key, int shift) { return (uint32_t)(key >> shift) & (RADIX_DIGITS - 1); }
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// the valid lanes of the wave whose digit is this lane's (every lane of the wave calls it)
__device__ inline uint64_t matching_lanes(uint32_t d, bool valid) {
    uint64_t same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < RADIX_BITS; ++b) {
        const bool bit = d >> b & 1;
        const uint64_t has = __ballot(valid && bit);
        same &= bit ? has : ~has;
    }
    return same;
}

static __global__ __launch_bounds__(256) void radix_prep_kernel(const uint64_t *__restrict__ keys, int64_t n, uint32_t *__restrict__ idx, unsigned long long *differing) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    unsigned long long x = 0;
    if (i < n) { idx[i] = (uint32_t)i; x = keys[i] ^ keys[0]; }
    for (int d = 32; d > 0; d >>= 1) x |= __shfl_xor(x, d, 64);
    if ((threadIdx.x & 63) == 0 && x) atomicOr(differing, x);
}

// grid: a workgroup of 256 per tile.  hist[digit * n_tiles + tile]
static __global__ __launch_bounds__(256) void radix_hist_kernel(const uint64_t *__restrict__ keys, int64_t n, int shift, int64_t n_tiles, uint32_t *__restrict__ hist) {
    __shared__ uint32_t count[RADIX_DIGITS];
    count[threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * RADIX_TILE + (int64_t)(threadIdx.x >> 6) * WAVE_KEYS + (threadIdx.x & 63);
#pragma unroll
    for (int j = 0; j < RADIX_ITEMS; ++j) {
        const int64_t i = first + j * 64;
        if (i < n) atomicAdd(&count[digit_of(keys[i], shift)], 1u);
    }
    __syncthreads();
    hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = count[threadIdx.x];
}

// base: the exclusive scan of hist.  Every pair of the tile goes to base[digit][tile] + its stable rank among the tile's equal digits.
static __global__ __launch_bounds__(256) void radix_scatter_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx, int64_t n, int shift,
                                                                   int64_t n_tiles, const uint32_t *__restrict__ base, uint64_t *__restrict__ keys_out,
                                                                   uint32_t *__restrict__ idx_out) {
    __shared__ uint32_t count[4][RADIX_DIGITS];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) count[i][threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * RADIX_TILE + (int64_t)w * WAVE_KEYS + lane;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    uint64_t key[RADIX_ITEMS];
    uint32_t rank[RADIX_ITEMS];
#pragma unroll
    for (int j = 0; j < RADIX_ITEMS; ++j) {
        const int64_t i = first + j * 64;
        const bool valid = i < n;
        key[j] = valid ? keys[i] : 0;
        const uint32_t d = digit_of(key[j], shift);
        const uint64_t same = matching_lanes(d, valid);
        const uint32_t old = count[w][d];        // every lane of the round has read before the round's leaders write
        rank[j] = old + (uint32_t)__popcll(same & below);
        wave_sync();
        if (valid && (same >> lane) == 1) count[w][d] = old + (uint32_t)__popcll(same);      // the highest lane of each digit
        wave_sync();
    }
    __syncthreads();
    {                                            // thread d: the tile's base of digit d, then the four waves in wave order
        uint32_t run = base[(int64_t)threadIdx.x * n_tiles + blockIdx.x];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t c = count[i][threadIdx.x];
            count[i][threadIdx.x] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RADIX_ITEMS; ++j) {
        const int64_t i = first + j * 64;
        if (i >= n) continue;
        const int64_t dst = (int64_t)count[w][digit_of(key[j], shift)] + rank[j];
        if (dst < n) { keys_out[dst] = key[j]; idx_out[dst] = idx[i]; }
    }
}

// at least `need` bytes with the first `used` kept: grown by half, the old bytes copied over
inline int grow(const HipFail &fail, hipStream_t stream, DeviceBuffer &b, size_t used, size_t need) {
    if (b.p && b.bytes >= need) return 0;
    DeviceBuffer bigger;
    CLAIR_HIP_TRY(fail, bigger.ensure(std::max(need, b.bytes + b.bytes / 2) + 256));
    if (used) CLAIR_HIP_TRY(fail, hipMemcpyAsync(bigger.p, b.p, used, hipMemcpyDeviceToDevice, stream));
    CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
    std::swap(b.p, bigger.p);
    std::swap(b.bytes, bigger.bytes);
    return 0;
}

// payloads [first, first + n) of the `total` bytes at `data` (device; every payload of 65280 bytes starts at a multiple of 65280, PAD readable
// behind the last byte), n <= EMIT_MAX.  compressed != 0: deflate_bgzf_kernel over the device-resident bytes, block i in
// out[i * 65536 .. + sizes[i]); compressed == 0: the bytes themselves, packed, sizes[i] bytes each.
constexpr int EMIT_MAX = 64;
inline int emit_payloads(const HipFail &fail, hipStream_t stream, const uint8_t *data, int64_t total, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes,
                         DeviceBuffer &e_meta, DeviceBuffer &e_out) {
    if (!out || !sizes || first < 0 || n < 0 || n > EMIT_MAX) return fail("emit: bad arguments (at most %d payloads a call)", EMIT_MAX);
    if (n == 0) return 0;
    if ((first + n - 1) * PAYLOAD >= total) return fail("emit: payloads [%lld, +%d) of %lld bytes", (long long)first, n, (long long)total);
    int32_t meta[3 * EMIT_MAX];                  // in_at, in_len, csize
    for (int i = 0; i < n; ++i) {
        meta[i] = (int32_t)(i * PAYLOAD);
        meta[EMIT_MAX + i] = (int32_t)std::min(PAYLOAD, total - (first + i) * PAYLOAD);
    }
    data += first * PAYLOAD;
    if (!compressed) {
        const int64_t bytes = (int64_t)(n - 1) * PAYLOAD + meta[EMIT_MAX + n - 1];
        CLAIR_HIP_TRY(fail, hipMemcpyAsync(out, data, (size_t)bytes, hipMemcpyDeviceToHost, stream));
        CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
        for (int i = 0; i < n; ++i) sizes[i] = meta[EMIT_MAX + i];
        return 0;
    }
    // the deflate over the device-resident bytes: only the blocks and their sizes come back
    CLAIR_HIP_TRY(fail, e_meta.ensure(sizeof meta));
    CLAIR_HIP_TRY(fail, e_out.ensure((size_t)EMIT_MAX * SLOT));
    int32_t *d_meta = e_meta.as<int32_t>();
    CLAIR_HIP_TRY(fail, hipMemcpyAsync(d_meta, meta, 2 * EMIT_MAX * 4, hipMemcpyHostToDevice, stream));
    CLAIR_HIP_TRY(fail, clair_def::launch_deflate_bgzf(stream, data, n, d_meta, d_meta + EMIT_MAX, e_out.as<uint8_t>(), d_meta + 2 * EMIT_MAX));
    CLAIR_HIP_TRY(fail, hipMemcpyAsync(out, e_out.p, (size_t)n * SLOT, hipMemcpyDeviceToHost, stream));
    CLAIR_HIP_TRY(fail, hipMemcpyAsync(sizes, d_meta + 2 * EMIT_MAX, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
    CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
    for (int i = 0; i < n; ++i)
        if (sizes[i] < 26 || sizes[i] > SLOT) return fail("payload %lld: the kernel reports %d bytes", (long long)(first + i), sizes[i]);
    return 0;
}

// the output of a stage that writes records: the bytes it has for the file on the device, cut into payloads; what no whole payload takes
// is carried to the front of the next bytes.  Owned by a stage's handle, freed (reset) before the handle's stream goes.  Everything is
// enqueued on `stream`; cut waits for it.
struct PayloadOut {
    DeviceBuffer d_bytes, d_carry, e_meta, e_out;
    int64_t total = 0, carry = 0;

    void rewind() { total = carry = 0; }         // a new file
    void reset() {
        for (DeviceBuffer *b : {&d_bytes, &d_carry, &e_meta, &e_out}) b->reset();
    }
    uint8_t *data() const { return d_bytes.as<uint8_t>(); }
    // room for the carried bytes, `bytes` more and PAD; the carried bytes put in front -> *at: where the new ones go
    int begin(const HipFail &fail, hipStream_t stream, int64_t bytes, uint8_t **at) {
        CLAIR_HIP_TRY(fail, clair_bix::at_least(d_bytes, (size_t)(carry + bytes + clair_bix::PAD)));
        CLAIR_HIP_TRY(fail, clair_bix::at_least(d_carry, (size_t)(PAYLOAD + clair_bix::PAD)));
        if (carry) CLAIR_HIP_TRY(fail, hipMemcpyAsync(d_bytes.p, d_carry.p, (size_t)carry, hipMemcpyDeviceToDevice, stream));
        *at = data() + carry;
        return 0;
    }
    // `added` bytes were put behind the carried ones: PAD zeroed behind them, -> *payloads ready for emit (with `last` the partial one
    // too), the rest carried
    int cut(const HipFail &fail, hipStream_t stream, int64_t added, bool last, int64_t *payloads) {
        const int64_t all = carry + added;
        CLAIR_HIP_TRY(fail, hipMemsetAsync(data() + all, 0, (size_t)clair_bix::PAD, stream));
        *payloads = payloads_of(all, last);
        const int64_t rest = all - std::min(all, *payloads * PAYLOAD);
        if (rest) CLAIR_HIP_TRY(fail, hipMemcpyAsync(d_carry.p, data() + *payloads * PAYLOAD, (size_t)rest, hipMemcpyDeviceToDevice, stream));
        CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
        total = all;
        carry = rest;
        return 0;
    }
    int emit(const HipFail &fail, hipStream_t stream, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) {
        return emit_payloads(fail, stream, data(), total, first, n, compressed, out, sizes, e_meta, e_out);
    }
};

// the sort's buffers and its driver: owned by a stage's handle, freed (reset) before the handle's stream goes
struct RadixSort {
    DeviceBuffer key[2], idx[2], hist, base, scan, differing;

    void reset() {
        for (DeviceBuffer *b : {&key[0], &key[1], &idx[0], &idx[1], &hist, &base, &scan, &differing}) b->reset();
    }
    // the stable order of keys [n] (device), n >= 1: -> *perm (device, this object's until the next sort), *passes run
    int sort(const HipFail &fail, hipStream_t stream, const uint64_t *keys, int64_t n, const uint32_t **perm, int *passes) {
        using clair_bix::at_least;
        using clair_scan::totals_kernel;
        using clair_scan::walk_kernel;
        using clair_scan::write_kernel;
        const int64_t n_tiles = (n + RADIX_TILE - 1) / RADIX_TILE, table = n_tiles * RADIX_DIGITS, nb = (table + SCAN_BLOCK - 1) / SCAN_BLOCK;
        using Digits = clair_scan::SumScan<uint32_t, uint32_t>;
        for (int i = 0; i < 2; ++i) {
            CLAIR_HIP_TRY(fail, at_least(key[i], (size_t)n * 8));
            CLAIR_HIP_TRY(fail, at_least(idx[i], (size_t)n * 4));
        }
        CLAIR_HIP_TRY(fail, at_least(hist, (size_t)table * 4));
        CLAIR_HIP_TRY(fail, at_least(base, (size_t)table * 4));
        CLAIR_HIP_TRY(fail, at_least(scan, (size_t)(nb + 1) * 4));
        CLAIR_HIP_TRY(fail, differing.ensure(8));
        unsigned long long *d_differing = differing.as<unsigned long long>();
        CLAIR_HIP_TRY(fail, hipMemsetAsync(d_differing, 0, 8, stream));
        hipLaunchKernelGGL(radix_prep_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, stream, keys, n, idx[0].as<uint32_t>(), d_differing);
        CLAIR_HIP_TRY(fail, hipGetLastError());
        unsigned long long differ = 0;
        CLAIR_HIP_TRY(fail, hipMemcpyAsync(&differ, d_differing, 8, hipMemcpyDeviceToHost, stream));
        CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
        const uint64_t *src_key = keys;
        const uint32_t *src_idx = idx[0].as<uint32_t>();
        uint32_t *d_hist = hist.as<uint32_t>(), *d_base = base.as<uint32_t>(), *d_scan = scan.as<uint32_t>();
        int to = 1;
        *passes = 0;
        for (int pass = 0; pass < RADIX_PASSES; ++pass) {
            const int shift = pass * RADIX_BITS;
            if (!(differ >> shift & (RADIX_DIGITS - 1))) continue;               // the digit is the same in every key
            uint64_t *dst_key = key[to].as<uint64_t>();
            uint32_t *dst_idx = idx[to].as<uint32_t>();
            hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, src_key, n, shift, n_tiles, d_hist);
            const Digits digits{d_hist};
            hipLaunchKernelGGL((totals_kernel<Digits, SCAN_ITEMS>), dim3((unsigned)nb), dim3(256), 0, stream, digits, table, d_scan);
            hipLaunchKernelGGL((walk_kernel<Digits, false>), dim3(1), dim3(256), 0, stream, Digits{d_scan}, nb, d_scan, d_scan + nb);
            hipLaunchKernelGGL((write_kernel<Digits, SCAN_ITEMS, WriteBefore<Digits>>), dim3((unsigned)nb), dim3(256), 0, stream, digits, table, (const uint32_t *)d_scan,
                               WriteBefore<Digits>{d_base});
            hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)n_tiles), dim3(256), 0, stream, src_key, src_idx, n, shift, n_tiles, (const uint32_t *)d_base, dst_key,
                               dst_idx);
            CLAIR_HIP_TRY(fail, hipGetLastError());
            src_key = dst_key;
            src_idx = dst_idx;
            to = 1 - to;
            ++*passes;
        }
        *perm = src_idx;
        return 0;
    }
};

}  // namespace clair_bsort
