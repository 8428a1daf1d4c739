// clair_markdup_*: duplicate reads flagged or removed on the device (include/clair_amd.h; docs/markdup_bam.md).  A translation unit of its
// own, outside the forward pass's sources (build.csrc_digest).  The rule is csrc/markdup_core.h, shared with the host twin
// (hostsrc/host_markdup.cpp); the front of a batch is index_bam's (bam_front.h); the radix sort, the keep scan and the copy are sort_bam's
// (radix_sort.h).  This file holds the kernels behind them and the handle.
//
//   md_summary_kernel  a thread per record: its fields, the walk over its real CIGAR (CG:B:I where the stored one is the placeholder) for the
//                      clips and the span, the FNV-1a hash of its name -> the 32-byte summary, and where its qualities lie; the first
//                      offender by a 64-bit atomicMin.  Every loop is bounded by a size fields() checked against block_size.
//   md_score_kernel    a wave per examined record: the qualities as aligned dwords (up to 3 bytes in front of and behind the array are
//                      read, inside the record and the stream's padding, and masked off), the bytes >= 15 summed in 64 bits per lane, the
//                      lanes by shuffles, lane 0 stores the clamped sum.  Integer adds: the sum does not depend on their order.
//   the resolution     over the summaries alone, every order by the stable radix sort, every verdict by a comparison with the neighbour
//                      in that order; no atomic decides anything, and each record's byte has exactly one writer.
//                        md_key_kernel     the 64-bit key of a step, read through the order so far; md_compose_kernel chains the orders
//                                          (least significant key first, as the sort's own passes are).
//                        md_mate_kernel    the order by (hash, read 1 / read 2 / neither): three binary searches give a record its group's
//                                          read 1s and read 2s; the k-th of one pairs with the k-th of the other.
//                        md_pairs_kernel   the order by (signature, score from the highest down, lower index): an entry whose signature is
//                                          its predecessor's is a duplicate pair; the entry's thread writes both records' bytes.
//                        md_frags_kernel   the order by (end, paired before fragment, score from the highest down, index): a fragment that
//                                          is not the head of its end's run is a duplicate (the head is a paired record, or a better
//                                          fragment).  It writes the byte of every record that is not paired.
//                        md_count_kernel   the counts: ballots, one integer atomicAdd a wave and counter.
//   md_patch_kernel    the second read, a thread per record: the flag's high byte at offset + 4 + 15 rewritten (an ordinary byte store; no
//                      two threads share a record), the record's length and whether it is kept.  With remove the keep scan
//                      (device_scan.h) places the kept records and copy_kernel moves them; without, the records are contiguous and go
//                      over in one copy.
// Ordinary vector loads and stores, integer atomics only for the first offender and the counts, no workgroup waits for another.
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#define CLAIR_BIX_FN __host__ __device__ inline
#include "markdup_core.h"
#include "bam_front.h"
#include "deflate_launch.h"
#include "device_buffer.h"
#include "device_scan.h"
#include "hip_status.h"
#include "radix_sort.h"

namespace clair_md {

static_assert(sizeof(Summary) == sizeof(clair_markdup_summary_t) && sizeof(Summary) == 32, "the summary is the header's");

// a thread per record.  out, qual_at, l_seq: of the batch (out already points at the batch's first summary)
static __global__ __launch_bounds__(256) void md_summary_kernel(Bytes m, const int64_t *__restrict__ starts, int64_t n_rec, int n_ref, int64_t first_index,
                                                                Summary *__restrict__ out, int64_t *__restrict__ qual_at, int32_t *__restrict__ l_seq,
                                                                unsigned long long *__restrict__ error) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_rec) return;
    const int64_t o = starts[k];
    Summary s;
    Layout y;
    const int verdict = summarize(m, o, n_ref, (uint32_t)(first_index + k), &s, &y);
    if (verdict != V_OK) atomicMin(error, (unsigned long long)k << 3 | (unsigned long long)verdict);
    out[k] = s;
    qual_at[k] = (s.bits & S_EXAMINED) ? y.qual : -1;
    l_seq[k] = y.l_seq;
}

// a wave per record, four to a workgroup
static __global__ __launch_bounds__(256) void md_score_kernel(const uint8_t *stream, const int64_t *__restrict__ qual_at, const int32_t *__restrict__ l_seq, int64_t n_rec,
                                                              Summary *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_rec) return;
    const int64_t q = qual_at[i], n = l_seq[i];
    if (q < 0 || n <= 0) return;                             // (the same for every lane of the wave)
    const uint8_t *p = stream + q;
    if (p[0] == 0xff) return;                                // absent: the score stays 0
    const uint32_t lane = threadIdx.x & 63;
    const int64_t head = (int64_t)((uintptr_t)p & 3), words = (head + n + 3) >> 2;
    const uint32_t *a = (const uint32_t *)((uintptr_t)p & ~(uintptr_t)3);
    unsigned long long sum = 0;
    for (int64_t j = lane; j < words; j += 64) {
        const uint32_t w = a[j];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int64_t at = j * 4 + b - head;
            if (at >= 0 && at < n) sum += quality_score(w >> (8 * b) & 255);
        }
    }
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) out[i].score = clamp_score(sum);
}

// ---- the resolution
enum { K_CLASS = 0, K_HASH, K_PAIR_SCORE, K_SIG_HI, K_SIG_LO, K_KIND_SCORE, K_END };

__device__ inline bool owner(const uint32_t *mate, uint32_t r) { return mate[r] != NO_MATE && r < mate[r]; }

// keys[j] = the key of step `what` of record order[j] (j itself when order is NULL)
static __global__ __launch_bounds__(256) void md_key_kernel(int what, const Summary *__restrict__ s, const uint32_t *__restrict__ mate, const uint32_t *__restrict__ order,
                                                            int64_t n, uint64_t *__restrict__ keys) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = order ? order[j] : (uint32_t)j;
    const Summary me = s[r];
    uint64_t key = 0;
    switch (what) {
    case K_CLASS: key = pair_class(me.bits); break;
    case K_HASH: key = me.hash; break;
    case K_PAIR_SCORE: key = owner(mate, r) ? (uint64_t)(uint32_t)~clamp_score((uint64_t)me.score + s[mate[r]].score) : 0; break;
    case K_SIG_HI: key = owner(mate, r) ? (me.end > s[mate[r]].end ? me.end : s[mate[r]].end) : NO_END; break;
    case K_SIG_LO: key = owner(mate, r) ? (me.end < s[mate[r]].end ? me.end : s[mate[r]].end) : NO_END; break;
    case K_KIND_SCORE: key = (me.bits & S_EXAMINED) ? (uint64_t)(mate[r] == NO_MATE ? 1 : 0) << 32 | (uint32_t)~me.score : 0; break;
    default: key = me.end; break;
    }
    keys[j] = key;
}
static __global__ __launch_bounds__(256) void md_compose_kernel(const uint32_t *__restrict__ order, const uint32_t *__restrict__ perm, int64_t n, uint32_t *__restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t p = perm[j];
    out[j] = order ? ((int64_t)p < n ? order[p] : 0) : p;
}

// the first place of the order whose (hash, class) is not below (hash, cls)
__device__ inline int64_t lower_place(const Summary *s, const uint32_t *order, int64_t n, uint64_t hash, uint32_t cls) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        const Summary x = s[order[mid]];
        if (x.hash < hash || (x.hash == hash && pair_class(x.bits) < cls)) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// order: by (hash, class), equal ones by index
static __global__ __launch_bounds__(256) void md_mate_kernel(const Summary *__restrict__ s, const uint32_t *__restrict__ order, int64_t n, uint32_t *__restrict__ mate) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = order[j];
    const Summary me = s[r];
    const uint32_t cls = pair_class(me.bits);
    uint32_t other = NO_MATE;
    if (cls < 2) {
        const int64_t first1 = lower_place(s, order, n, me.hash, 0), first2 = lower_place(s, order, n, me.hash, 1), end2 = lower_place(s, order, n, me.hash, 2);
        const int64_t at = cls == 0 ? first2 + (j - first1) : first1 + (j - first2);
        if (at >= 0 && (cls == 0 ? at < end2 : at < first2)) other = order[at];
    }
    mate[r] = other;
}
// order: by (signature, ~score), equal ones by index; the pairs' entries first
static __global__ __launch_bounds__(256) void md_pairs_kernel(const Summary *__restrict__ s, const uint32_t *__restrict__ mate, const uint32_t *__restrict__ order, int64_t n,
                                                              uint8_t *__restrict__ dup) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = order[j];
    if (!owner(mate, r)) return;
    bool same = false;
    if (j > 0) {
        const uint32_t q = order[j - 1];
        if (owner(mate, q)) {
            const uint64_t a = s[r].end, b = s[mate[r]].end, c = s[q].end, d = s[mate[q]].end;
            same = (a < b ? a : b) == (c < d ? c : d) && (a < b ? b : a) == (c < d ? d : c);
        }
    }
    dup[r] = same;
    dup[mate[r]] = same;
}
// order: by (end, paired before fragment, ~score), equal ones by index
static __global__ __launch_bounds__(256) void md_frags_kernel(const Summary *__restrict__ s, const uint32_t *__restrict__ mate, const uint32_t *__restrict__ order, int64_t n,
                                                              uint8_t *__restrict__ dup) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = order[j];
    if (mate[r] != NO_MATE) return;                          // its pair's entry wrote it
    dup[r] = (s[r].bits & S_EXAMINED) && j > 0 && s[order[j - 1]].end == s[r].end;
}
static __global__ __launch_bounds__(256) void md_count_kernel(const Summary *__restrict__ s, const uint32_t *__restrict__ mate, const uint8_t *__restrict__ dup, int64_t n,
                                                              unsigned long long *__restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    const bool seen = in && (s[i].bits & S_EXAMINED), own = in && owner(mate, (uint32_t)i), frag = seen && mate[i] == NO_MATE, d = in && dup[i];
    const bool flags[MC_WORDS] = {in, seen, own, frag, own && d, frag && d};
#pragma unroll
    for (int c = 0; c < MC_WORDS; ++c) {
        const uint64_t lanes = __ballot(flags[c]);
        if ((threadIdx.x & 63) == 0 && lanes) atomicAdd(counts + c, (unsigned long long)__popcll(lanes));
    }
}

// ---- the second read.  s, dup: of the batch's first record on
static __global__ __launch_bounds__(256) void md_patch_kernel(uint8_t *stream, const int64_t *__restrict__ starts, int64_t n_rec, const Summary *__restrict__ s,
                                                              const uint8_t *__restrict__ dup, int remove, uint32_t *__restrict__ len, uint8_t *__restrict__ keep) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_rec) return;
    const int64_t o = starts[k];
    const bool seen = (s[k].bits & S_EXAMINED) != 0, duplicate = seen && dup[k];
    if (seen) stream[o + 19] = patched(stream[o + 19], duplicate);
    len[k] = 4u + Bytes{stream}.le32(o);
    keep[k] = !(remove && duplicate);
}
struct WritePlace {                              // dst[i]: where a kept record's bytes go, -1: nowhere
    static constexpr int PAST_END = 0;
    int64_t *dst;
    int64_t base;
    static __device__ inline Kept seed() { return Kept{0, 0, 0}; }
    __device__ inline void write(const KeepScan &, int64_t i, int64_t, Kept before, Kept item) const { dst[i] = item.n ? base + before.bytes : -1; }
};

}  // namespace clair_md

struct clair_markdup : clair_bix::StageHandle {
    // the file
    int n_ref = -1;
    int64_t memory = 0, n_records = 0, marked = 0;
    bool remove = false, resolved = false;
    int64_t counts[clair_md::MC_WORDS] = {0};
    DeviceBuffer d_summaries, d_dup, d_acc;
    // the batch
    DeviceBuffer b_qual, b_lseq, b_len, b_keep, b_dst, b_scan;
    // the resolution
    clair_bsort::RadixSort radix;
    DeviceBuffer r_keys, r_order[2], r_mate;
    clair_bsort::PayloadOut out;                 // the records of the second read
    // the debug entries
    DeviceBuffer t_stream, t_starts, t_out;
};

namespace {

using namespace clair_md;
using clair_bix::at_least;
using clair_bix::PAD;
using clair_scan::totals_kernel;
using clair_scan::walk_kernel;
using clair_scan::write_kernel;

constexpr int64_t GUARD = 64;                    // bytes in front of and behind what _debug_mark's kernels may write

std::string g_md_error;
inline HipFail md_fail(clair_markdup *h) { return {h ? h->error : g_md_error}; }

// the summaries of the n_rec records at d_starts of the stream at `bytes` -> out [n_rec] (device); *error: the first offender, NO_ERROR
int summarize_records(clair_markdup *h, const uint8_t *bytes, const int64_t *d_starts, int64_t n_rec, int n_ref, int64_t first_index, Summary *out,
                      unsigned long long *error) {
    CLAIR_HIP_TRY(md_fail(h), at_least(h->b_qual, (size_t)n_rec * 8));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->b_lseq, (size_t)n_rec * 4));
    CLAIR_HIP_TRY(md_fail(h), h->d_acc.ensure(MC_WORDS * 8));
    unsigned long long *d_error = h->d_acc.as<unsigned long long>();
    *error = NO_ERROR;
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(d_error, error, 8, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(md_summary_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, h->stream, Bytes{bytes}, d_starts, n_rec, n_ref, first_index, out,
                       h->b_qual.as<int64_t>(), h->b_lseq.as<int32_t>(), d_error);
    hipLaunchKernelGGL(md_score_kernel, dim3(blocks_of(n_rec, 4)), dim3(256), 0, h->stream, bytes, (const int64_t *)h->b_qual.as<int64_t>(),
                       (const int32_t *)h->b_lseq.as<int32_t>(), n_rec, out);
    CLAIR_HIP_TRY(md_fail(h), hipGetLastError());
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(error, d_error, 8, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    return 0;
}

// one step of a least-significant-key-first sort: the records in `order` (NULL: by index) ordered stably by key `what` -> out
int sort_step(clair_markdup *h, int what, const Summary *s, int64_t n, const uint32_t *order, uint32_t *out) {
    uint64_t *keys = h->r_keys.as<uint64_t>();
    hipLaunchKernelGGL(md_key_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, h->stream, what, s, (const uint32_t *)h->r_mate.as<uint32_t>(), order, n, keys);
    CLAIR_HIP_TRY(md_fail(h), hipGetLastError());
    const uint32_t *perm = nullptr;
    int passes = 0;
    if (h->radix.sort(md_fail(h), h->stream, keys, n, &perm, &passes)) return 1;
    hipLaunchKernelGGL(md_compose_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, h->stream, order, perm, n, out);
    CLAIR_HIP_TRY(md_fail(h), hipGetLastError());
    return 0;
}

// the rule over s [n] (device), n >= 1 -> dup [n] (device), counts [MC_WORDS] (host)
int resolve(clair_markdup *h, const Summary *s, int64_t n, uint8_t *dup, int64_t *counts) {
    CLAIR_HIP_TRY(md_fail(h), at_least(h->r_keys, (size_t)n * 8));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->r_order[0], (size_t)n * 4));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->r_order[1], (size_t)n * 4));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->r_mate, (size_t)n * 4));
    CLAIR_HIP_TRY(md_fail(h), h->d_acc.ensure(MC_WORDS * 8));
    uint32_t *a = h->r_order[0].as<uint32_t>(), *b = h->r_order[1].as<uint32_t>(), *mate = h->r_mate.as<uint32_t>();
    const dim3 grid(blocks_of(n, 256)), block(256);
    // 1. mates
    if (sort_step(h, K_CLASS, s, n, nullptr, a) || sort_step(h, K_HASH, s, n, a, b)) return 1;
    hipLaunchKernelGGL(md_mate_kernel, grid, block, 0, h->stream, s, (const uint32_t *)b, n, mate);
    // 2. pairs
    if (sort_step(h, K_PAIR_SCORE, s, n, nullptr, a) || sort_step(h, K_SIG_HI, s, n, a, b) || sort_step(h, K_SIG_LO, s, n, b, a)) return 1;
    hipLaunchKernelGGL(md_pairs_kernel, grid, block, 0, h->stream, s, (const uint32_t *)mate, (const uint32_t *)a, n, dup);
    // 3. ends
    if (sort_step(h, K_KIND_SCORE, s, n, nullptr, a) || sort_step(h, K_END, s, n, a, b)) return 1;
    hipLaunchKernelGGL(md_frags_kernel, grid, block, 0, h->stream, s, (const uint32_t *)mate, (const uint32_t *)b, n, dup);
    unsigned long long *d_counts = h->d_acc.as<unsigned long long>(), got[MC_WORDS];
    CLAIR_HIP_TRY(md_fail(h), hipMemsetAsync(d_counts, 0, sizeof got, h->stream));
    hipLaunchKernelGGL(md_count_kernel, grid, block, 0, h->stream, s, (const uint32_t *)mate, (const uint8_t *)dup, n, d_counts);
    CLAIR_HIP_TRY(md_fail(h), hipGetLastError());
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(got, d_counts, sizeof got, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    for (int c = 0; c < MC_WORDS; ++c) counts[c] = (int64_t)got[c];
    return 0;
}

// the flags of the n_rec records at d_starts patched where they lie, then the records (remove: those kept) copied to out (device), which has
// room for all of them: -> *out_bytes copied, *written records.  The records are the one range [first, first + range_bytes) of the stream
int patch_and_place(clair_markdup *h, uint8_t *bytes, const int64_t *d_starts, int64_t n_rec, const Summary *s, const uint8_t *dup, bool remove, int64_t first,
                    int64_t range_bytes, uint8_t *out, int64_t *out_bytes, int64_t *written) {
    const int64_t nb = (n_rec + SCAN_BLOCK - 1) / SCAN_BLOCK;
    CLAIR_HIP_TRY(md_fail(h), at_least(h->b_len, (size_t)n_rec * 4));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->b_keep, (size_t)n_rec));
    uint32_t *b_len = h->b_len.as<uint32_t>();
    uint8_t *b_keep = h->b_keep.as<uint8_t>();
    hipLaunchKernelGGL(md_patch_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, h->stream, bytes, d_starts, n_rec, s, dup, remove ? 1 : 0, b_len, b_keep);
    CLAIR_HIP_TRY(md_fail(h), hipGetLastError());
    if (!remove) {
        CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(out, bytes + first, (size_t)range_bytes, hipMemcpyDeviceToDevice, h->stream));
        CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
        *out_bytes = range_bytes;
        *written = n_rec;
        return 0;
    }
    CLAIR_HIP_TRY(md_fail(h), at_least(h->b_dst, (size_t)n_rec * 8));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->b_scan, (size_t)(nb + 1) * sizeof(Kept)));
    int64_t *b_dst = h->b_dst.as<int64_t>();
    Kept *b_scan = h->b_scan.as<Kept>();
    const KeepScan keeps{b_keep, b_len};
    clair_scan::Stored<KeepScan> stored;
    stored.keep = b_keep;
    stored.len = b_len;
    stored.stored = b_scan;
    Kept kept{0, 0, 0};
    hipLaunchKernelGGL((totals_kernel<KeepScan, SCAN_ITEMS>), dim3((unsigned)nb), dim3(256), 0, h->stream, keeps, n_rec, b_scan);
    hipLaunchKernelGGL((walk_kernel<clair_scan::Stored<KeepScan>, false>), dim3(1), dim3(256), 0, h->stream, stored, nb, b_scan, b_scan + nb);
    CLAIR_HIP_TRY(md_fail(h), hipGetLastError());
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(&kept, b_scan + nb, sizeof kept, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    if ((int64_t)kept.n > n_rec || kept.bytes < 0 || kept.bytes > range_bytes)
        return md_fail(h)("mark: %u of %lld records kept, %lld of %lld bytes: the keep scan is broken", kept.n, (long long)n_rec, (long long)kept.bytes, (long long)range_bytes);
    hipLaunchKernelGGL((write_kernel<KeepScan, SCAN_ITEMS, WritePlace>), dim3((unsigned)nb), dim3(256), 0, h->stream, keeps, n_rec, (const Kept *)b_scan, WritePlace{b_dst, 0});
    hipLaunchKernelGGL(copy_kernel, dim3(blocks_of(n_rec, 4)), dim3(256), 0, h->stream, (const uint8_t *)bytes, d_starts, (const uint32_t *)nullptr, (const uint32_t *)b_len,
                       (const int64_t *)b_dst, n_rec, out);
    CLAIR_HIP_TRY(md_fail(h), hipGetLastError());
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    *out_bytes = kept.bytes;
    *written = kept.n;
    return 0;
}

// the first offender of a batch as index_bam words it
int report(clair_markdup *h, unsigned long long error, int64_t n_rec, int64_t before) {
    using namespace clair_bix;
    Front &front = h->front;
    const int64_t k = (int64_t)(error >> 3);
    if (k >= n_rec) return md_fail(h)("batch: offending record %lld of %lld: the summary pass is broken", (long long)k, (long long)n_rec);
    int64_t o = 0;
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(&o, front.starts() + k, 8, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    if (o < 0 || o + 4 > front.len) return md_fail(h)("batch: record %lld at %lld of %lld bytes: the frame pass is broken", (long long)k, (long long)o, (long long)front.len);
    const Detail d{before + k, 0, 0, 0, 0, 0, front.voffset(o), 0, (int32_t)(error & 7)};
    char buf[400];
    describe(buf, sizeof buf, d);
    return md_fail(h)("%s", buf);
}

}  // namespace

extern "C" {

const char *clair_markdup_last_error(const clair_markdup_t *h) { return h ? h->error.c_str() : g_md_error.c_str(); }

int clair_markdup_create(int device, int max_blocks, int segment_bytes, clair_markdup_t **out) {
    if (!out) return md_fail(nullptr)("out is NULL");
    *out = nullptr;
    clair_markdup *h = new clair_markdup;
    if (h->open(md_fail(nullptr), device, max_blocks, segment_bytes, "the device duplicate marking runs on an MI355X only (the host one is markdup_bam --backend host)")) {
        clair_markdup_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}

void clair_markdup_destroy(clair_markdup_t *h) {
    if (!h) return;
    h->settle();
    for (DeviceBuffer *b : {&h->d_summaries, &h->d_dup, &h->d_acc, &h->b_qual, &h->b_lseq, &h->b_len, &h->b_keep, &h->b_dst, &h->b_scan, &h->r_keys, &h->r_order[0],
                            &h->r_order[1], &h->r_mate, &h->t_stream, &h->t_starts, &h->t_out})
        b->reset();                              // before the stream goes, not in the destructor
    h->out.reset();
    h->radix.reset();
    h->close();
    delete h;
}

int clair_markdup_begin(clair_markdup_t *h, int n_ref, int64_t memory, int remove) {
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    if (n_ref < 0) return md_fail(h)("begin: bad arguments");
    if (memory < 1) return md_fail(h)("begin: memory %lld", (long long)memory);
    CLAIR_HIP_TRY(md_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    h->n_ref = n_ref;
    h->memory = memory;
    h->remove = remove != 0;
    h->resolved = false;
    h->n_records = h->marked = 0;
    h->out.rewind();
    h->front.rewind();
    return 0;
}

int clair_markdup_batch(clair_markdup_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                        const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state) {
    using namespace clair_bix;
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    if (!state) return md_fail(h)("batch: NULL argument");
    if (h->n_ref < 0 || h->resolved) return md_fail(h)("batch: begin first");
    if (check_batch_args(md_fail(h), "batch", cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    CLAIR_HIP_TRY(md_fail(h), hipSetDevice(h->device));
    Front &front = h->front;
    if (front.open_batch(md_fail(h), cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) { h->n_ref = -1; return 1; }
    const int64_t n_rec = front.fr.n_rec, before = h->n_records;
    const auto refuse = [&](int rc) { h->n_ref = -1; return rc; };       // a batch that fails leaves a handle that wants a new begin
    if (before + n_rec > MAX_RECORDS) return refuse(md_fail(h)("more than 2^31 - 1 records: the resolution's indices are 32 bits wide"));
    if ((before + n_rec) * (int64_t)sizeof(Summary) > h->memory) {
        char buf[200];
        describe_memory(buf, sizeof buf, before + n_rec, h->memory);
        return refuse(md_fail(h)("%s", buf));
    }
    if (n_rec > 0) {
        if (clair_bsort::grow(md_fail(h), h->stream, h->d_summaries, (size_t)before * sizeof(Summary), (size_t)(before + n_rec) * sizeof(Summary))) return refuse(1);
        unsigned long long error = NO_ERROR;
        if (summarize_records(h, front.bytes, front.starts(), n_rec, h->n_ref, before, h->d_summaries.as<Summary>() + before, &error)) return refuse(1);
        if (error != NO_ERROR) return refuse(report(h, error, n_rec, before));
    }
    if (front.close_batch(md_fail(h), last)) return refuse(1);
    h->n_records = before + n_rec;
    state[MS_TOTAL] = h->n_records;
    state[MS_N_RECORDS] = n_rec;
    state[MS_CARRY] = front.carry;
    return 0;
}

int clair_markdup_resolve(clair_markdup_t *h) {
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    if (h->n_ref < 0) return md_fail(h)("resolve: begin first");
    CLAIR_HIP_TRY(md_fail(h), hipSetDevice(h->device));
    std::fill(h->counts, h->counts + MC_WORDS, (int64_t)0);
    if (h->n_records > 0) {
        CLAIR_HIP_TRY(md_fail(h), at_least(h->d_dup, (size_t)h->n_records));
        if (resolve(h, h->d_summaries.as<Summary>(), h->n_records, h->d_dup.as<uint8_t>(), h->counts)) return 1;
    }
    h->resolved = true;
    h->marked = 0;
    h->out.rewind();
    h->front.rewind();
    return 0;
}

int clair_markdup_mark(clair_markdup_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                       const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *info) {
    using namespace clair_bix;
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    if (!info) return md_fail(h)("mark: NULL argument");
    if (h->n_ref < 0 || !h->resolved) return md_fail(h)("mark: resolve first");
    if (check_batch_args(md_fail(h), "mark", cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    CLAIR_HIP_TRY(md_fail(h), hipSetDevice(h->device));
    Front &front = h->front;
    const auto refuse = [&](int rc) { h->n_ref = -1; return rc; };
    if (front.open_batch(md_fail(h), cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return refuse(1);
    const int64_t n_rec = front.fr.n_rec;
    if (h->marked + n_rec > h->n_records)
        return refuse(md_fail(h)("the second read finds more than the %lld records of the first: the file changed", (long long)h->n_records));
    const int64_t range = n_rec > 0 ? front.fr.tail - entry : 0;
    if (range < 0 || entry + range > front.len) return refuse(md_fail(h)("mark: records [%lld, %lld) of %lld bytes: the frame pass is broken", (long long)entry, (long long)front.fr.tail, (long long)front.len));
    uint8_t *d_out = nullptr;                    // behind what the batch before carried over
    if (h->out.begin(md_fail(h), h->stream, range, &d_out)) return 1;
    int64_t bytes = 0, written = 0;
    if (n_rec > 0 && patch_and_place(h, front.bytes, front.starts(), n_rec, h->d_summaries.as<Summary>() + h->marked, h->d_dup.as<uint8_t>() + h->marked, h->remove, entry,
                                     range, d_out, &bytes, &written))
        return refuse(1);
    if (front.close_batch(md_fail(h), last)) return refuse(1);
    h->marked += n_rec;
    if (last && h->marked != h->n_records)
        return refuse(md_fail(h)("the second read finds %lld records, the first found %lld: the file changed", (long long)h->marked, (long long)h->n_records));
    int64_t payloads = 0;
    if (h->out.cut(md_fail(h), h->stream, bytes, last != 0, &payloads)) return 1;
    info[MI_BYTES] = h->out.total;
    info[MI_PAYLOADS] = payloads;
    info[MI_RECORDS] = n_rec;
    info[MI_WRITTEN] = written;
    return 0;
}

int clair_markdup_emit(clair_markdup_t *h, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) {
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    CLAIR_HIP_TRY(md_fail(h), hipSetDevice(h->device));
    return h->out.emit(md_fail(h), h->stream, first, n, compressed, out, sizes);
}

int clair_markdup_stats(clair_markdup_t *h, int64_t *counts) {
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    if (!counts || !h->resolved) return md_fail(h)("stats: resolve first");
    memcpy(counts, h->counts, sizeof h->counts);
    return 0;
}

static int md_begin(void *ctx, int n_ref, int64_t memory, int remove) { return clair_markdup_begin((clair_markdup_t *)ctx, n_ref, memory, remove); }
static int md_batch(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len, const int64_t *coffset,
                    int64_t end_coffset, int64_t entry, int last, int64_t *state) {
    return clair_markdup_batch((clair_markdup_t *)ctx, cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry, last, state);
}
static int md_resolve(void *ctx) { return clair_markdup_resolve((clair_markdup_t *)ctx); }
static int md_mark(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len, const int64_t *coffset,
                   int64_t end_coffset, int64_t entry, int last, int64_t *info) {
    return clair_markdup_mark((clair_markdup_t *)ctx, cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry, last, info);
}
static int md_emit(void *ctx, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) { return clair_markdup_emit((clair_markdup_t *)ctx, first, n, compressed, out, sizes); }
static int md_stats(void *ctx, int64_t *counts) { return clair_markdup_stats((clair_markdup_t *)ctx, counts); }
static const char *md_last_error(const void *ctx) { return clair_markdup_last_error((const clair_markdup_t *)ctx); }

int clair_markdup_backend(clair_markdup_t *h, clair_markdup_backend_t *out) {
    if (!h || !out) return md_fail(h)("backend: NULL argument");
    *out = clair_markdup_backend_t{h, md_begin, md_batch, md_resolve, md_mark, md_emit, md_stats, md_last_error};
    return 0;
}

// every start is checked here: the kernels take them as they are.  -> the stream (GUARD in front, PAD and GUARD behind, both 0xa5) and the starts on the device
static int debug_upload(clair_markdup *h, const char *who, const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, int64_t n) {
    using namespace clair_bix;
    for (int64_t i = 0; i < n; ++i) {
        int64_t next = 0;
        if (starts[i] < 0 || step(Bytes{stream}, starts[i], stream_bytes, &next) != STEP_NEXT) return md_fail(h)("%s: no record at %lld", who, (long long)starts[i]);
    }
    CLAIR_HIP_TRY(md_fail(h), at_least(h->t_stream, (size_t)(stream_bytes + PAD + 2 * GUARD)));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->t_starts, (size_t)n * 8));
    uint8_t *d = h->t_stream.as<uint8_t>();
    CLAIR_HIP_TRY(md_fail(h), hipMemsetAsync(d, 0xa5, (size_t)(stream_bytes + PAD + 2 * GUARD), h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipMemsetAsync(d + GUARD + stream_bytes, 0, (size_t)PAD, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(d + GUARD, stream, (size_t)stream_bytes, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(h->t_starts.p, starts, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
    return 0;
}

int clair_markdup_debug_summary(clair_markdup_t *h, const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, int64_t n, int n_ref,
                                clair_markdup_summary_t *out) {
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    if (n < 0 || n > MAX_RECORDS || stream_bytes < 0 || n_ref < 0 || (n > 0 && (!stream || !starts || !out))) return md_fail(h)("debug_summary: bad arguments");
    if (n == 0) return 0;
    CLAIR_HIP_TRY(md_fail(h), hipSetDevice(h->device));
    if (debug_upload(h, "debug_summary", stream, stream_bytes, starts, n)) return 1;
    CLAIR_HIP_TRY(md_fail(h), at_least(h->t_out, (size_t)n * sizeof(Summary)));
    unsigned long long error = NO_ERROR;
    if (summarize_records(h, h->t_stream.as<uint8_t>() + GUARD, h->t_starts.as<int64_t>(), n, n_ref, 0, h->t_out.as<Summary>(), &error)) return 1;
    if (error != NO_ERROR) return md_fail(h)("debug_summary: record %lld is malformed (verdict %d)", (long long)(error >> 3), (int)(error & 7));
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(out, h->t_out.p, (size_t)n * sizeof(Summary), hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    return 0;
}

int clair_markdup_debug_resolve(clair_markdup_t *h, const clair_markdup_summary_t *summaries, int64_t n, uint8_t *duplicate) {
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    if (n < 0 || n > MAX_RECORDS || (n > 0 && (!summaries || !duplicate))) return md_fail(h)("debug_resolve: bad arguments");
    if (n == 0) return 0;
    CLAIR_HIP_TRY(md_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->t_out, (size_t)n * sizeof(Summary)));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->t_stream, (size_t)n));
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(h->t_out.p, summaries, (size_t)n * sizeof(Summary), hipMemcpyHostToDevice, h->stream));
    int64_t counts[MC_WORDS];
    if (resolve(h, h->t_out.as<Summary>(), n, h->t_stream.as<uint8_t>(), counts)) return 1;
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(duplicate, h->t_stream.p, (size_t)n, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    return 0;
}

int clair_markdup_debug_mark(clair_markdup_t *h, const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, int64_t n,
                             const clair_markdup_summary_t *summaries, const uint8_t *duplicate, int remove, uint8_t *patched_stream, uint8_t *out, int64_t *out_bytes) {
    using namespace clair_bix;
    if (!h) return md_fail(nullptr)("markdup handle is NULL");
    if (n < 1 || n > MAX_RECORDS || stream_bytes < 0 || !stream || !starts || !summaries || !duplicate || !patched_stream || !out || !out_bytes)
        return md_fail(h)("debug_mark: bad arguments");
    CLAIR_HIP_TRY(md_fail(h), hipSetDevice(h->device));
    if (debug_upload(h, "debug_mark", stream, stream_bytes, starts, n)) return 1;
    int64_t range = 0;
    for (int64_t i = 0; i < n; ++i) {                        // back to back, as a batch's records are
        if (i > 0 && starts[i] != starts[0] + range) return md_fail(h)("debug_mark: record %lld does not follow record %lld", (long long)i, (long long)i - 1);
        range += 4 + (int64_t)u32(stream + starts[i]);
    }
    CLAIR_HIP_TRY(md_fail(h), at_least(h->d_summaries, (size_t)n * sizeof(Summary)));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->d_dup, (size_t)n));
    CLAIR_HIP_TRY(md_fail(h), at_least(h->t_out, (size_t)(range + 2 * GUARD)));
    h->n_ref = -1;                                           // the file's summaries are gone
    uint8_t *d_out = h->t_out.as<uint8_t>();
    CLAIR_HIP_TRY(md_fail(h), hipMemsetAsync(d_out, 0xa5, (size_t)(range + 2 * GUARD), h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(h->d_summaries.p, summaries, (size_t)n * sizeof(Summary), hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(h->d_dup.p, duplicate, (size_t)n, hipMemcpyHostToDevice, h->stream));
    int64_t bytes = 0, written = 0;
    if (patch_and_place(h, h->t_stream.as<uint8_t>() + GUARD, h->t_starts.as<int64_t>(), n, h->d_summaries.as<Summary>(), h->d_dup.as<uint8_t>(), remove != 0, starts[0],
                        range, d_out + GUARD, &bytes, &written))
        return 1;
    std::vector<uint8_t> back((size_t)(range + 2 * GUARD)), around((size_t)(stream_bytes + PAD + 2 * GUARD));
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(back.data(), d_out, back.size(), hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipMemcpyAsync(around.data(), h->t_stream.p, around.size(), hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(md_fail(h), hipStreamSynchronize(h->stream));
    for (int64_t i = 0; i < GUARD; ++i) {
        if (back[(size_t)i] != 0xa5) return md_fail(h)("debug_mark: the copy wrote in front of its output");
        if (around[(size_t)i] != 0xa5 || around[(size_t)(GUARD + stream_bytes + PAD + i)] != 0xa5) return md_fail(h)("debug_mark: the patch wrote outside the stream");
    }
    for (int64_t i = 0; i < PAD; ++i)
        if (around[(size_t)(GUARD + stream_bytes + i)] != 0) return md_fail(h)("debug_mark: the patch wrote into the stream's padding");
    for (int64_t i = GUARD + bytes; i < range + 2 * GUARD; ++i)
        if (back[(size_t)i] != 0xa5) return md_fail(h)("debug_mark: the copy wrote behind its %lld bytes", (long long)bytes);
    memcpy(patched_stream, around.data() + GUARD, (size_t)stream_bytes);
    memcpy(out, back.data() + GUARD, (size_t)bytes);
    *out_bytes = bytes;
    return 0;
}

}  // extern "C"
