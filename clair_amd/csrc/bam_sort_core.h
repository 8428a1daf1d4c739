// The rules of sort_bam (docs/sort_bam.md) that the device (csrc/bam_sort.hip) and its host twin (hostsrc/host_bam_sort.cpp) share: the
// 64-bit key a record is sorted by, the bucket of the byte histogram it is counted in, which verdicts of a record's fields stop a sort, and
// the words a batch exchanges with the file driver.  What belongs to a record -- the frame step, the size rule, the fields -- is
// csrc/bam_record_core.h and csrc/bam_index_core.h (Fields); nothing of it is restated here.  Plain C++17; CLAIR_BIX_FN is
// `__host__ __device__ inline` in the device's translation unit.
#pragma once
#include "bam_index_core.h"

namespace clair_bsort {

using namespace clair_bix;                   // Bytes, Fields, fields, V_*, Detail, describe, voffset_at

constexpr int64_t PAYLOAD = 65280;           // bytes of records per BGZF block of the output: where BgzfWriter cuts (bgzip's 0xff00)
constexpr int64_t SLOT = 65536;              // a compressed block's room
constexpr uint32_t BUCKET_SHIFT = 20;        // a bucket of the byte histogram: 2^20 positions of one reference
constexpr int64_t MAX_GROUP_RECORDS = 0x7fffffff;
constexpr int RADIX_BITS = 8, RADIX_PASSES = 8, RADIX_DIGITS = 256;
constexpr int RADIX_ITEMS = 8;               // keys per thread of a tile
constexpr int RADIX_TILE = 256 * RADIX_ITEMS;

// the int64 words a batch exchanges with the driver that carries them from batch to batch (include/clair_host.h: CLAIR_BAMSORT_STATE)
enum { SS_RECORDS_BEFORE = 0, SS_PREV_KEY, SS_N_RECORDS, SS_LAST_KEY, SS_KEPT, SS_KEPT_BYTES, SS_UNSORTED, SS_OVERFLOW, SS_MAPPED, SS_UNPLACED, SS_CARRY, SS_WORDS };
// what _sort reports
enum { SI_BYTES = 0, SI_PAYLOADS, SI_RECORDS, SI_PASSES, SI_WORDS };

// tid unsigned, so that -1 sorts last; then the position; then the forward strand before the reverse one
CLAIR_BIX_FN uint64_t sort_key(int32_t tid, int32_t pos, uint32_t flag) {
    return (uint64_t)(uint32_t)tid << 32 | (uint64_t)((uint32_t)(pos + 1) << 1) | (uint64_t)(flag >> 4 & 1);
}
// a reference of `length` bases has ceil(length / 2^20) buckets, at least one
CLAIR_BIX_FN int64_t buckets_of(int64_t length) {
    const int64_t n = (length + ((int64_t)1 << BUCKET_SHIFT) - 1) >> BUCKET_SHIFT;
    return n < 1 ? 1 : n;
}
// first_bucket [n_ref + 1]: each reference's first bucket; first_bucket[n_ref] is the one all records without a reference share
CLAIR_BIX_FN int64_t bucket_of(int32_t tid, int32_t pos, int n_ref, const int64_t *first_bucket, const int64_t *ref_len) {
    if (tid < 0 || tid >= n_ref) return first_bucket[n_ref];
    int64_t p = pos;
    if (p > ref_len[tid] - 1) p = ref_len[tid] - 1;
    if (p < 0) p = 0;
    return first_bucket[tid] + (p >> BUCKET_SHIFT);
}
// the order and the extent of the .bai are index_bam's to complain about
CLAIR_BIX_FN int sort_verdict(int verdict) { return verdict == V_TOO_FAR || verdict == V_UNSORTED ? V_OK : verdict; }

CLAIR_BIX_FN int64_t payloads_of(int64_t bytes, bool partial_too) { return partial_too ? (bytes + PAYLOAD - 1) / PAYLOAD : bytes / PAYLOAD; }

}  // namespace clair_bsort
