// clair_bamsort_*: a BAM sorted by coordinate on the device (include/clair_amd.h; docs/sort_bam.md).  A translation unit of its own, outside
// the forward pass's sources (build.csrc_digest).  The rules are csrc/bam_sort_core.h, shared with the host twin (hostsrc/host_bam_sort.cpp);
// the front of a batch -- blocks inflated into a device-resident stream, records framed there -- is index_bam's (bam_front.h); this file
// holds the kernels behind it and the handle.
//
//   keys_kernel      a thread per record: its fields (bam_index_core.h), verdict, 64-bit key, length 4 + block_size and bucket; the first
//                    offender by a 64-bit atomicMin, the bucket's bytes by a 64-bit integer atomicAdd, the order against the record before
//                    it, the keep flag of the group being read.
//   the scan         (device_scan.h) over (kept, kept bytes) places the kept records behind the group's; copy_kernel, a wave per record,
//                    moves them.  A copy writes bytes [dst, dst + len) and no other: single bytes up to the first 4-byte boundary of the
//                    destination and behind the last, whole dwords between, each put together from the two aligned source dwords it
//                    straddles (reads may reach 3 bytes around the source record, inside its buffer's padding; never writes).  The loop is
//                    bounded by the record's length.
//   the radix sort   (radix_sort.h, shared with markdup.hip, as are the copy and the payload emit)
//                    stable, least significant digit first, 8 bits a pass over (key, uint32 index) pairs in ping-pong buffers.
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
//   the gather       the lengths len[perm[i]] scanned in int64 to destination offsets, then copy_kernel again, into the sorted buffer behind
//                    the partial payload the group before left over: every payload of 65280 bytes starts at a multiple of 65280 there,
//                    which is the 4-byte alignment deflate_bgzf_kernel (deflate_launch.h) wants of its input.
// Ordinary vector loads and stores, integer atomics only, no workgroup waits for another, every loop is bounded by a length or a count.
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#define CLAIR_BIX_FN __host__ __device__ inline
#include "bam_sort_core.h"
#include "bam_front.h"
#include "deflate_launch.h"
#include "device_buffer.h"
#include "device_scan.h"
#include "hip_status.h"
#include "radix_sort.h"

namespace clair_bsort {

// what the keys pass accumulates: the first offending record, then the counters and the order flag
enum { A_ERROR = 0, A_MAPPED, A_UNPLACED, A_UNSORTED, A_WORDS };

struct Refs {
    int n_ref;
    const int64_t *first_bucket;                 // n_ref + 1
    const int64_t *ref_len;                      // n_ref
};

// a thread per record
__global__ __launch_bounds__(256) void keys_kernel(Bytes m, const int64_t *__restrict__ starts, int64_t n_rec, Refs r, uint64_t prev_key, int64_t lo, int64_t hi,
                                                   int count_bytes, uint64_t *__restrict__ key, uint32_t *__restrict__ len, uint8_t *__restrict__ keep,
                                                   unsigned long long *__restrict__ hist, unsigned long long *__restrict__ acc) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_rec) return;
    const int64_t o = starts[k];
    const Fields f = fields(m, o, r.n_ref);
    const uint32_t size = 4u + m.le32(o);        // (the frame step accepted it: no more than INT32_MAX)
    const uint64_t mine = sort_key(f.tid, f.pos, f.flag);
    key[k] = mine;
    len[k] = size;
    keep[k] = 0;
    if (sort_verdict(f.verdict) != V_OK) {
        atomicMin(acc + A_ERROR, (unsigned long long)k << 3 | (unsigned long long)f.verdict);
        return;
    }
    uint64_t before = prev_key;
    if (k > 0) {
        const int64_t p = starts[k - 1];
        before = sort_key((int32_t)m.le32(p + 4), (int32_t)m.le32(p + 8), m.le16(p + 18));
    }
    if (mine < before) atomicOr(acc + A_UNSORTED, 1ull);
    if (f.tid < 0) atomicAdd(acc + A_UNPLACED, 1ull);
    else if (!(f.flag & 4)) atomicAdd(acc + A_MAPPED, 1ull);
    const int64_t bucket = bucket_of(f.tid, f.pos, r.n_ref, r.first_bucket, r.ref_len);
    if (count_bytes) atomicAdd(hist + bucket, (unsigned long long)size);
    keep[k] = bucket >= lo && bucket < hi;
}

// ---- compaction (Kept, KeepScan: radix_sort.h)
struct WriteKept {                               // a kept record joins the group's arrays; dst[i]: where its bytes go in the group buffer, -1: nowhere
    static constexpr int PAST_END = 0;
    const uint64_t *key;
    uint64_t *g_key;
    int64_t *g_off;
    uint32_t *g_len;
    int64_t *dst;
    int64_t g_n, g_bytes, cap;
    static __device__ inline Kept seed() { return Kept{0, 0, 0}; }
    __device__ inline void write(const KeepScan &p, int64_t i, int64_t, Kept before, Kept item) const {
        const int64_t j = g_n + before.n;
        if (!item.n || j >= cap) { dst[i] = -1; return; }
        g_key[j] = key[i];
        g_off[j] = g_bytes + before.bytes;
        g_len[j] = p.len[i];
        dst[i] = g_bytes + before.bytes;
    }
};

// the lengths in the sorted order, scanned to where each record goes
struct PermLen {
    using T = int64_t;
    const uint32_t *len;
    const uint32_t *perm;
    int64_t n;                                   // of both: a place that is none counts nothing (and copy_kernel copies nothing for it)
    static __device__ inline T identity() { return 0; }
    static __device__ inline T join(T a, T b) { return a + b; }
    static __device__ inline T up(T x, int d) { return (T)__shfl_up((long long)x, d, 64); }
    __device__ inline T item(int64_t i) const { return (int64_t)perm[i] < n ? (T)len[perm[i]] : 0; }
};
}  // namespace clair_bsort

struct clair_bamsort : clair_bix::StageHandle {
    // the file
    int n_ref = -1;
    int64_t memory = 0, n_buckets = 0;
    DeviceBuffer d_refs, d_hist, d_acc;          // first_bucket [n_ref + 1] then ref_len [n_ref]; the byte histogram; the accumulators
    // the read in progress
    bool in_pass = false, first = false, overflow = false;
    int64_t lo = 0, hi = 0;
    DeviceBuffer b_key, b_len, b_keep, b_dst, b_scan;
    // the group
    DeviceBuffer d_group, g_key, g_off, g_len;
    int64_t g_n = 0, g_bytes = 0;
    // the sort and the gather
    clair_bsort::RadixSort radix;
    DeviceBuffer d_out_off, d_len_scan;
    clair_bsort::PayloadOut out;                 // the sorted records
    // the debug entries
    DeviceBuffer t_stream, t_starts, t_perm, t_len, t_out, t_keys;
};

namespace {

using namespace clair_bsort;
using clair_bix::at_least;
using clair_bix::PAD;
using clair_scan::totals_kernel;
using clair_scan::walk_kernel;
using clair_scan::write_kernel;

constexpr int64_t GUARD = 64;                    // bytes in front of and behind the output of _debug_gather

std::string g_bsort_error;
inline HipFail bsort_fail(clair_bamsort *h) { return {h ? h->error : g_bsort_error}; }

// at least `need` bytes with the first `used` kept: grown by half, the old bytes copied over
int grow(clair_bamsort *h, DeviceBuffer &b, size_t used, size_t need) { return clair_bsort::grow(bsort_fail(h), h->stream, b, used, need); }

// the stable order of keys [n] (device), n >= 1: -> *perm (device, the handle's until the next sort), *passes run
int radix_sort(clair_bamsort *h, const uint64_t *keys, int64_t n, const uint32_t **perm, int *passes) {
    return h->radix.sort(bsort_fail(h), h->stream, keys, n, perm, passes);      // (radix_sort.h)
}

// record i of the output = record index[i] of the source (len_of[r] bytes at src + src_at[r]), one behind the other from dst on
int gather(clair_bamsort *h, const uint8_t *src, const int64_t *src_at, const uint32_t *index, const uint32_t *len_of, int64_t n, uint8_t *dst) {
    const int64_t nb = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    CLAIR_HIP_TRY(bsort_fail(h), at_least(h->d_out_off, (size_t)n * 8));
    CLAIR_HIP_TRY(bsort_fail(h), at_least(h->d_len_scan, (size_t)(nb + 1) * 8));
    int64_t *d_off = h->d_out_off.as<int64_t>(), *d_scan = h->d_len_scan.as<int64_t>();
    const PermLen lens{len_of, index, n};
    using Totals = clair_scan::SumScan<int64_t, int64_t>;
    hipLaunchKernelGGL((totals_kernel<PermLen, SCAN_ITEMS>), dim3((unsigned)nb), dim3(256), 0, h->stream, lens, n, d_scan);
    hipLaunchKernelGGL((walk_kernel<Totals, false>), dim3(1), dim3(256), 0, h->stream, Totals{d_scan}, nb, d_scan, d_scan + nb);
    hipLaunchKernelGGL((write_kernel<PermLen, SCAN_ITEMS, WriteBefore<PermLen>>), dim3((unsigned)nb), dim3(256), 0, h->stream, lens, n, (const int64_t *)d_scan,
                       WriteBefore<PermLen>{d_off});
    hipLaunchKernelGGL(copy_kernel, dim3(blocks_of(n, 4)), dim3(256), 0, h->stream, src, src_at, index, len_of, (const int64_t *)d_off, n, dst);
    CLAIR_HIP_TRY(bsort_fail(h), hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *clair_bamsort_last_error(const clair_bamsort_t *h) { return h ? h->error.c_str() : g_bsort_error.c_str(); }

int clair_bamsort_create(int device, int max_blocks, int segment_bytes, clair_bamsort_t **out) {
    if (!out) return bsort_fail(nullptr)("out is NULL");
    *out = nullptr;
    clair_bamsort *h = new clair_bamsort;
    if (h->open(bsort_fail(nullptr), device, max_blocks, segment_bytes, "the device sort runs on an MI355X only (the host one is sort_bam --backend host)")) {
        clair_bamsort_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}

void clair_bamsort_destroy(clair_bamsort_t *h) {
    if (!h) return;
    h->settle();
    for (DeviceBuffer *b : {&h->d_refs, &h->d_hist, &h->d_acc, &h->b_key, &h->b_len, &h->b_keep, &h->b_dst, &h->b_scan, &h->d_group, &h->g_key, &h->g_off, &h->g_len,
                            &h->d_out_off, &h->d_len_scan, &h->t_stream, &h->t_starts, &h->t_perm, &h->t_len, &h->t_out, &h->t_keys})
        b->reset();                              // before the stream goes, not in the destructor
    h->out.reset();
    h->radix.reset();
    h->close();
    delete h;
}

int clair_bamsort_begin(clair_bamsort_t *h, int n_ref, const int64_t *ref_len, int64_t memory) {
    if (!h) return bsort_fail(nullptr)("bamsort handle is NULL");
    if (n_ref < 0 || (n_ref > 0 && !ref_len)) return bsort_fail(h)("begin: bad arguments");
    if (memory < 1) return bsort_fail(h)("begin: memory %lld", (long long)memory);
    h->n_ref = -1;
    h->in_pass = false;
    std::vector<int64_t> refs((size_t)2 * n_ref + 1, 0);
    for (int r = 0; r < n_ref; ++r) {
        refs[(size_t)r + 1] = refs[(size_t)r] + buckets_of(ref_len[r]);
        refs[(size_t)n_ref + 1 + r] = ref_len[r];
    }
    h->n_buckets = refs[(size_t)n_ref] + 1;
    CLAIR_HIP_TRY(bsort_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(bsort_fail(h), hipStreamSynchronize(h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), h->d_refs.ensure(refs.size() * 8));
    CLAIR_HIP_TRY(bsort_fail(h), h->d_hist.ensure((size_t)h->n_buckets * 8));
    CLAIR_HIP_TRY(bsort_fail(h), h->d_acc.ensure(A_WORDS * 8));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(h->d_refs.p, refs.data(), refs.size() * 8, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemsetAsync(h->d_hist.p, 0, (size_t)h->n_buckets * 8, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipStreamSynchronize(h->stream));
    h->memory = memory;
    h->out.rewind();
    h->g_n = h->g_bytes = 0;
    h->n_ref = n_ref;
    return 0;
}

int clair_bamsort_pass(clair_bamsort_t *h, int64_t bucket_lo, int64_t bucket_hi, int first) {
    if (!h) return bsort_fail(nullptr)("bamsort handle is NULL");
    if (h->n_ref < 0) return bsort_fail(h)("pass: begin first");
    if (bucket_lo < 0 || bucket_hi < bucket_lo || bucket_hi > h->n_buckets) return bsort_fail(h)("pass: buckets [%lld, %lld) of %lld", (long long)bucket_lo, (long long)bucket_hi, (long long)h->n_buckets);
    CLAIR_HIP_TRY(bsort_fail(h), hipSetDevice(h->device));
    if (first) CLAIR_HIP_TRY(bsort_fail(h), hipMemsetAsync(h->d_hist.p, 0, (size_t)h->n_buckets * 8, h->stream));
    h->lo = bucket_lo;
    h->hi = bucket_hi;
    h->first = first != 0;
    h->overflow = false;
    h->front.rewind();
    h->g_n = h->g_bytes = 0;
    h->in_pass = true;
    return 0;
}

int clair_bamsort_batch(clair_bamsort_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                        const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state) {
    using namespace clair_bix;
    if (!h) return bsort_fail(nullptr)("bamsort handle is NULL");
    if (!state) return bsort_fail(h)("batch: NULL argument");
    if (h->n_ref < 0 || !h->in_pass) return bsort_fail(h)("batch: begin and pass first");
    if (check_batch_args(bsort_fail(h), "batch", cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    h->in_pass = false;                          // a batch that fails leaves a handle that wants a new pass
    CLAIR_HIP_TRY(bsort_fail(h), hipSetDevice(h->device));
    // 1, 2. the stream and the record starts (bam_front.h)
    Front &front = h->front;
    if (front.open_batch(bsort_fail(h), cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    const int64_t n_rec = front.fr.n_rec;
    const Bytes m{front.bytes};
    unsigned long long acc[A_WORDS] = {NO_ERROR, 0, 0, 0};
    uint64_t last_key = (uint64_t)state[SS_PREV_KEY];
    Kept kept{0, 0, 0};
    if (n_rec > 0) {
        // 3. keys, lengths, the histogram, the order, the keep flags; how much is kept
        const int64_t nb = (n_rec + SCAN_BLOCK - 1) / SCAN_BLOCK;
        CLAIR_HIP_TRY(bsort_fail(h), at_least(h->b_key, (size_t)n_rec * 8));
        CLAIR_HIP_TRY(bsort_fail(h), at_least(h->b_len, (size_t)n_rec * 4));
        CLAIR_HIP_TRY(bsort_fail(h), at_least(h->b_keep, (size_t)n_rec));
        CLAIR_HIP_TRY(bsort_fail(h), at_least(h->b_dst, (size_t)n_rec * 8));
        CLAIR_HIP_TRY(bsort_fail(h), at_least(h->b_scan, (size_t)(nb + 1) * sizeof(Kept)));
        uint64_t *b_key = h->b_key.as<uint64_t>();
        uint32_t *b_len = h->b_len.as<uint32_t>();
        uint8_t *b_keep = h->b_keep.as<uint8_t>();
        int64_t *b_dst = h->b_dst.as<int64_t>();
        Kept *b_scan = h->b_scan.as<Kept>();
        unsigned long long *d_acc = h->d_acc.as<unsigned long long>();
        const Refs refs{h->n_ref, h->d_refs.as<int64_t>(), h->d_refs.as<int64_t>() + h->n_ref + 1};
        CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(d_acc, acc, sizeof acc, hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(keys_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, h->stream, m, front.starts(), n_rec, refs, (uint64_t)state[SS_PREV_KEY], h->lo,
                           h->overflow ? h->lo : h->hi, h->first ? 1 : 0, b_key, b_len, b_keep, h->d_hist.as<unsigned long long>(), d_acc);
        const KeepScan keeps{b_keep, b_len};
        clair_scan::Stored<KeepScan> stored;
        stored.keep = b_keep;
        stored.len = b_len;
        stored.stored = b_scan;
        hipLaunchKernelGGL((totals_kernel<KeepScan, SCAN_ITEMS>), dim3((unsigned)nb), dim3(256), 0, h->stream, keeps, n_rec, b_scan);
        hipLaunchKernelGGL((walk_kernel<clair_scan::Stored<KeepScan>, false>), dim3(1), dim3(256), 0, h->stream, stored, nb, b_scan, b_scan + nb);
        CLAIR_HIP_TRY(bsort_fail(h), hipGetLastError());
        CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, h->stream));
        CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(&kept, b_scan + nb, sizeof kept, hipMemcpyDeviceToHost, h->stream));
        CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(&last_key, b_key + (n_rec - 1), 8, hipMemcpyDeviceToHost, h->stream));
        CLAIR_HIP_TRY(bsort_fail(h), hipStreamSynchronize(h->stream));
        if (acc[A_ERROR] != NO_ERROR) {
            const int64_t k = (int64_t)(acc[A_ERROR] >> 3);
            if (k >= n_rec) return bsort_fail(h)("batch: offending record %lld of %lld: the keys pass is broken", (long long)k, (long long)n_rec);
            int64_t o = 0;
            CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(&o, front.starts() + k, 8, hipMemcpyDeviceToHost, h->stream));
            CLAIR_HIP_TRY(bsort_fail(h), hipStreamSynchronize(h->stream));
            if (o < 0 || o + 4 > front.len) return bsort_fail(h)("batch: record %lld at %lld of %lld bytes: the frame pass is broken", (long long)k, (long long)o, (long long)front.len);
            const Detail d{state[SS_RECORDS_BEFORE] + k, 0, 0, 0, 0, 0, front.voffset(o), 0, (int32_t)(acc[A_ERROR] & 7)};
            char buf[400];
            describe(buf, sizeof buf, d);
            return bsort_fail(h)("%s", buf);
        }
        if ((int64_t)kept.n > n_rec || kept.bytes < 0 || kept.bytes > front.len) return bsort_fail(h)("batch: %u of %lld records kept, %lld bytes: the keep scan is broken", kept.n, (long long)n_rec, (long long)kept.bytes);
        // 4. the kept records join the group
        if (kept.n > 0 && h->g_bytes + kept.bytes > h->memory) {
            if (!h->first) return bsort_fail(h)("batch: the group outgrows the %lld bytes the histogram gave it", (long long)h->memory);
            h->overflow = true;                  // the file does not fit: what was compacted is dropped, the read goes on for the histogram
            h->g_n = h->g_bytes = 0;
            kept = Kept{0, 0, 0};
        }
        if (kept.n > 0) {
            if (h->g_n + (int64_t)kept.n > MAX_GROUP_RECORDS) return bsort_fail(h)("more than 2^31 - 1 records in one group: a smaller --memory makes smaller groups");
            const size_t have = (size_t)h->g_n, want = (size_t)(h->g_n + kept.n);
            if (grow(h, h->d_group, (size_t)h->g_bytes, (size_t)(h->g_bytes + kept.bytes + PAD)) || grow(h, h->g_key, have * 8, want * 8) ||
                grow(h, h->g_off, have * 8, want * 8) || grow(h, h->g_len, have * 4, want * 4))
                return 1;
            const WriteKept writer{b_key, h->g_key.as<uint64_t>(), h->g_off.as<int64_t>(), h->g_len.as<uint32_t>(), b_dst, h->g_n, h->g_bytes, h->g_n + (int64_t)kept.n};
            hipLaunchKernelGGL((write_kernel<KeepScan, SCAN_ITEMS, WriteKept>), dim3((unsigned)nb), dim3(256), 0, h->stream, keeps, n_rec, (const Kept *)b_scan, writer);
            hipLaunchKernelGGL(copy_kernel, dim3(blocks_of(n_rec, 4)), dim3(256), 0, h->stream, (const uint8_t *)front.bytes, front.starts(), (const uint32_t *)nullptr,
                               (const uint32_t *)b_len, (const int64_t *)b_dst, n_rec, h->d_group.as<uint8_t>());
            CLAIR_HIP_TRY(bsort_fail(h), hipGetLastError());
            h->g_n += kept.n;
            h->g_bytes += kept.bytes;
        }
    }
    if (front.close_batch(bsort_fail(h), last)) return 1;
    state[SS_N_RECORDS] = n_rec;
    state[SS_LAST_KEY] = (int64_t)last_key;
    state[SS_KEPT] = kept.n;
    state[SS_KEPT_BYTES] = kept.bytes;
    state[SS_UNSORTED] = acc[A_UNSORTED] ? 1 : 0;
    state[SS_OVERFLOW] = h->overflow ? 1 : 0;
    state[SS_MAPPED] = (int64_t)acc[A_MAPPED];
    state[SS_UNPLACED] = (int64_t)acc[A_UNPLACED];
    state[SS_CARRY] = front.carry;
    h->in_pass = true;
    return 0;
}

int clair_bamsort_histogram(clair_bamsort_t *h, int64_t *bytes, int64_t n_buckets) {
    if (!h) return bsort_fail(nullptr)("bamsort handle is NULL");
    if (!bytes || h->n_ref < 0) return bsort_fail(h)("histogram: no file begun, or bytes is NULL");
    if (n_buckets != h->n_buckets) return bsort_fail(h)("histogram: %lld buckets, the handle has %lld", (long long)n_buckets, (long long)h->n_buckets);
    CLAIR_HIP_TRY(bsort_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(bytes, h->d_hist.p, (size_t)n_buckets * 8, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipStreamSynchronize(h->stream));
    return 0;
}

int clair_bamsort_sort(clair_bamsort_t *h, int last, int64_t *info) {
    if (!h) return bsort_fail(nullptr)("bamsort handle is NULL");
    if (!info || h->n_ref < 0 || !h->in_pass) return bsort_fail(h)("sort: no read of the input is open, or info is NULL");
    h->in_pass = false;
    CLAIR_HIP_TRY(bsort_fail(h), hipSetDevice(h->device));
    const int64_t n = h->g_n;
    uint8_t *d_sorted = nullptr;                 // behind what the group before carried over
    if (h->out.begin(bsort_fail(h), h->stream, h->g_bytes, &d_sorted)) return 1;
    int passes = 0;
    if (n > 0) {
        const uint32_t *perm = nullptr;
        if (radix_sort(h, h->g_key.as<uint64_t>(), n, &perm, &passes)) return 1;
        if (gather(h, h->d_group.as<uint8_t>(), h->g_off.as<int64_t>(), perm, h->g_len.as<uint32_t>(), n, d_sorted)) return 1;
    }
    int64_t payloads = 0;
    if (h->out.cut(bsort_fail(h), h->stream, h->g_bytes, last != 0, &payloads)) return 1;
    h->g_n = h->g_bytes = 0;
    info[SI_BYTES] = h->out.total;
    info[SI_PAYLOADS] = payloads;
    info[SI_RECORDS] = n;
    info[SI_PASSES] = passes;
    return 0;
}

int clair_bamsort_emit(clair_bamsort_t *h, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) {
    if (!h) return bsort_fail(nullptr)("bamsort handle is NULL");
    CLAIR_HIP_TRY(bsort_fail(h), hipSetDevice(h->device));
    return h->out.emit(bsort_fail(h), h->stream, first, n, compressed, out, sizes);
}

static int bsort_begin(void *ctx, int n_ref, const int64_t *ref_len, int64_t memory) { return clair_bamsort_begin((clair_bamsort_t *)ctx, n_ref, ref_len, memory); }
static int bsort_pass(void *ctx, int64_t lo, int64_t hi, int first) { return clair_bamsort_pass((clair_bamsort_t *)ctx, lo, hi, first); }
static int bsort_batch(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                       const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state) {
    return clair_bamsort_batch((clair_bamsort_t *)ctx, cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry, last, state);
}
static int bsort_histogram(void *ctx, int64_t *bytes, int64_t n_buckets) { return clair_bamsort_histogram((clair_bamsort_t *)ctx, bytes, n_buckets); }
static int bsort_sort(void *ctx, int last, int64_t *info) { return clair_bamsort_sort((clair_bamsort_t *)ctx, last, info); }
static int bsort_emit(void *ctx, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) { return clair_bamsort_emit((clair_bamsort_t *)ctx, first, n, compressed, out, sizes); }
static const char *bsort_last_error(const void *ctx) { return clair_bamsort_last_error((const clair_bamsort_t *)ctx); }

int clair_bamsort_backend(clair_bamsort_t *h, clair_bamsort_backend_t *out) {
    if (!h || !out) return bsort_fail(h)("backend: NULL argument");
    *out = clair_bamsort_backend_t{h, bsort_begin, bsort_pass, bsort_batch, bsort_histogram, bsort_sort, bsort_emit, bsort_last_error};
    return 0;
}

int clair_bamsort_debug_sort(clair_bamsort_t *h, const uint64_t *keys, int64_t n, uint32_t *perm) {
    if (!h) return bsort_fail(nullptr)("bamsort handle is NULL");
    if (n < 0 || n > MAX_GROUP_RECORDS || (n > 0 && (!keys || !perm))) return bsort_fail(h)("debug_sort: bad arguments");
    if (n == 0) return 0;
    CLAIR_HIP_TRY(bsort_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(bsort_fail(h), at_least(h->t_keys, (size_t)n * 8));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(h->t_keys.p, keys, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    const uint32_t *d_perm = nullptr;
    int passes = 0;
    if (radix_sort(h, h->t_keys.as<uint64_t>(), n, &d_perm, &passes)) return 1;
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(perm, d_perm, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipStreamSynchronize(h->stream));
    return 0;
}

int clair_bamsort_debug_gather(clair_bamsort_t *h, const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, const uint32_t *perm, int64_t n, uint8_t *out,
                               int64_t out_bytes) {
    using namespace clair_bix;
    if (!h) return bsort_fail(nullptr)("bamsort handle is NULL");
    if (n < 0 || n > MAX_GROUP_RECORDS || stream_bytes < 0 || out_bytes < 0 || (n > 0 && (!stream || !starts || !perm || !out))) return bsort_fail(h)("debug_gather: bad arguments");
    if (n == 0) return out_bytes == 0 ? 0 : bsort_fail(h)("debug_gather: 0 bytes gathered, %lld expected", (long long)out_bytes);
    std::vector<uint32_t> lens((size_t)n);
    int64_t sum = 0;
    for (int64_t i = 0; i < n; ++i) {            // every source range and every place is checked here: the kernel takes them as they are
        int64_t next = 0;
        if (starts[i] < 0 || step(Bytes{stream}, starts[i], stream_bytes, &next) != STEP_NEXT) return bsort_fail(h)("debug_gather: no record at %lld", (long long)starts[i]);
        if ((int64_t)perm[i] >= n) return bsort_fail(h)("debug_gather: perm[%lld] = %u of %lld", (long long)i, perm[i], (long long)n);
        lens[(size_t)i] = (uint32_t)(next - starts[i]);
    }
    for (int64_t i = 0; i < n; ++i) sum += lens[perm[i]];
    if (sum != out_bytes) return bsort_fail(h)("debug_gather: %lld bytes gathered, %lld expected", (long long)sum, (long long)out_bytes);
    CLAIR_HIP_TRY(bsort_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(bsort_fail(h), at_least(h->t_stream, (size_t)(stream_bytes + PAD)));
    CLAIR_HIP_TRY(bsort_fail(h), at_least(h->t_starts, (size_t)n * 8));
    CLAIR_HIP_TRY(bsort_fail(h), at_least(h->t_perm, (size_t)n * 4));
    CLAIR_HIP_TRY(bsort_fail(h), at_least(h->t_len, (size_t)n * 4));
    CLAIR_HIP_TRY(bsort_fail(h), at_least(h->t_out, (size_t)(out_bytes + 2 * GUARD)));
    uint8_t *d_out = h->t_out.as<uint8_t>();
    CLAIR_HIP_TRY(bsort_fail(h), hipMemsetAsync(d_out, 0xa5, (size_t)(out_bytes + 2 * GUARD), h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemsetAsync(h->t_stream.as<uint8_t>() + stream_bytes, 0, (size_t)PAD, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(h->t_stream.p, stream, (size_t)stream_bytes, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(h->t_starts.p, starts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(h->t_perm.p, perm, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(h->t_len.p, lens.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
    if (gather(h, h->t_stream.as<uint8_t>(), h->t_starts.as<int64_t>(), h->t_perm.as<uint32_t>(), h->t_len.as<uint32_t>(), n, d_out + GUARD)) return 1;
    std::vector<uint8_t> back((size_t)(out_bytes + 2 * GUARD));
    CLAIR_HIP_TRY(bsort_fail(h), hipMemcpyAsync(back.data(), d_out, back.size(), hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(bsort_fail(h), hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < GUARD; ++i)
        if (back[(size_t)i] != 0xa5 || back[(size_t)(GUARD + out_bytes + i)] != 0xa5) return bsort_fail(h)("debug_gather: the copy wrote outside its %lld bytes", (long long)out_bytes);
    memcpy(out, back.data() + GUARD, (size_t)out_bytes);
    return 0;
}

}  // extern "C"
