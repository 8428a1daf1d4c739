// The rules of index_bam (docs/index_bam.md) that the device (csrc/bam_index.hip) and its host twin (hostsrc/host_bam_index.cpp) share: the
// frame step over a stream of BAM records, the fields of a record that a .bai is made of, the order check, the virtual offset of a stream
// position and the wording of every verdict.  The frame step itself, the size rule and the CIGAR span are a record's own rules
// (csrc/bam_record_core.h).  Plain C++17 over a small memory context (Bytes); CLAIR_BIX_FN is `__host__ __device__ inline` in the device's
// translation unit.
#pragma once
#include <cstdint>
#include <cstdio>

#ifndef CLAIR_BIX_FN
#define CLAIR_BIX_FN inline
#endif
#ifndef CLAIR_REC_FN
#define CLAIR_REC_FN CLAIR_BIX_FN
#endif
#include "bam_record_core.h"

namespace clair_bix {

using namespace clair_rec;                   // Bytes, step and STEP_*, describe_bad_step, describe_cut

constexpr uint32_t SEG_MIN = 64, SEG_MAX = 8192, SEG_DEFAULT = 8192;      // bytes of a framing segment: a power of two
constexpr uint32_t MIN_RECORD = 36;                                      // 4 + block_size, block_size >= 32
constexpr int64_t POS_LIMIT = (int64_t)1 << 29;                          // the extent of the .bai binning scheme
constexpr uint32_t WINDOW_SHIFT = 14;                                    // the linear index: 16 KiB windows
constexpr uint64_t NO_OFFSET = ~0ull;                                    // a window no record touched
constexpr int STATE_WORDS = 8;

// the int64 words a batch exchanges with the caller that carries them from batch to batch (include/clair_host.h)
enum { ST_RECORDS_BEFORE = 0, ST_PREV_TID, ST_PREV_POS, ST_N_RECORDS, ST_N_RUNS, ST_LAST_TID, ST_LAST_POS, ST_CARRY };
// what clair_*bamidx_debug_frame reports
enum { FR_N_STARTS = 0, FR_TAIL, FR_BAD, FR_SENTINELS, FR_WORDS };

// the step seen from a segment that starts at `base`, as an offset from the base: >= seg, the chain leaves the segment there (a long record
// may leave it by many segments); == o, the chain stops at o (bad or past the end: absorbing)
CLAIR_BIX_FN uint32_t seg_next(const Bytes &m, int64_t base, uint32_t o, int64_t len) {
    int64_t next = 0;
    if (step(m, base + o, len, &next) != STEP_NEXT) return o;
    return (uint32_t)(next - base);
}
// rounds of pointer jumping after which every chain of a segment is resolved: a chain has at most seg / 36 + 1 links inside it
CLAIR_BIX_FN int jump_rounds(uint32_t seg) {
    int r = 0;
    while ((1u << r) < seg / MIN_RECORD + 2) ++r;
    return r;
}

// one thread, after every segment resolved exit[base + o] (seg_next followed to its end): the true chain from `entry`, segment by segment.
// seg_entry[s]: where the chain enters segment s, -1 for a segment it never stands in (a long record jumps over it, or the chain stopped
// before it).  result[0]: where the chain stops -- the tail, len when the records fill the stream --, result[1]: 1 when it stops on a bad step.
CLAIR_BIX_FN void chain_walk(const Bytes &m, int64_t len, int64_t entry, uint32_t seg, int64_t n_seg, const uint32_t *exit, int64_t *seg_entry,
                             int64_t *result) {
    int64_t e = entry;
    bool stopped = false;
    for (int64_t s = 0; s < n_seg; ++s) {
        const int64_t base = s * (int64_t)seg;
        if (stopped || e >= base + (int64_t)seg) { seg_entry[s] = -1; continue; }
        seg_entry[s] = e;
        const uint32_t v = exit[e];
        stopped = v < seg;
        e = base + (int64_t)v;
    }
    int64_t next = 0;
    result[0] = e;
    result[1] = step(m, e, len, &next) == STEP_BAD ? 1 : 0;
}
// the records of segment s on the true chain, which enters it at e (>= 0): how many; starts (unless NULL) gets them from slot `first` on
CLAIR_BIX_FN uint32_t seg_records(const Bytes &m, int64_t len, uint32_t seg, int64_t s, int64_t e, int64_t *starts, int64_t first, int64_t cap) {
    const int64_t end = (s + 1) * (int64_t)seg < len ? (s + 1) * (int64_t)seg : len;
    uint32_t c = 0;
    int64_t next = 0;
    while (e < end && c <= seg / MIN_RECORD && step(m, e, len, &next) == STEP_NEXT) {
        if (starts && first + c < cap) starts[first + c] = e;
        ++c;
        e = next;
    }
    return c;
}

// ---- a record's fields
enum { V_OK = 0, V_L_SEQ = SIZES_L_SEQ, V_FIELDS = SIZES_FIELDS, V_TID, V_POS, V_TOO_FAR, V_UNSORTED };
struct Fields {
    int32_t tid, pos;
    int64_t end;                 // bam_endpos: pos + max(reference span of the stored CIGAR, 1); span 0 for an unmapped record
    uint32_t bin, flag;
    int verdict;
};
CLAIR_BIX_FN uint32_t reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26));
    return 0;
}
// o: a record start the frame step accepted (block_size >= 32, the record inside the stream)
CLAIR_BIX_FN Fields fields(const Bytes &m, int64_t o, int n_ref) {
    Fields f;
    const uint32_t block_size = m.le32(o);
    f.tid = (int32_t)m.le32(o + 4);
    f.pos = (int32_t)m.le32(o + 8);
    const uint32_t l_read_name = m.byte(o + 12), n_cigar = m.le16(o + 16);
    f.flag = m.le16(o + 18);
    const int32_t l_seq = (int32_t)m.le32(o + 20);
    f.end = (int64_t)f.pos + 1;
    f.bin = 4680;
    f.verdict = V_OK;
    const int sizes = sizes_verdict(block_size, l_read_name, n_cigar, l_seq);
    if (sizes == SIZES_L_SEQ || sizes == SIZES_FIELDS) { f.verdict = sizes; return f; }     // (an empty read name does not trouble an index)
    if (f.tid < -1 || f.tid >= n_ref) { f.verdict = V_TID; return f; }
    if (f.pos < -1) { f.verdict = V_POS; return f; }
    const int64_t span = (f.flag & 4) ? 0 : cigar_span(m, o + 36 + l_read_name, n_cigar);
    f.end = (int64_t)f.pos + (span > 1 ? span : 1);
    if (f.tid >= 0) {
        if (f.end > POS_LIMIT) { f.verdict = V_TOO_FAR; return f; }
        f.bin = reg2bin(f.pos > 0 ? f.pos : 0, f.end);
    }
    return f;
}

// (tid, pos) as one word that orders as a coordinate-sorted BAM does: tid unsigned, so that -1 sorts last
CLAIR_BIX_FN uint64_t order_key(int32_t tid, int32_t pos) { return (uint64_t)(uint32_t)tid << 32 | ((uint32_t)pos ^ 0x80000000u); }

// ---- virtual offsets.  at[k]: where piece k of the stream starts (at[0] == 0, ascending; an empty piece shares its position with the next
// one, which wins); voff[k]: the virtual offset of its first byte.  The last entry stands at the stream's end: the block after the batch.
CLAIR_BIX_FN uint64_t voffset_at(const int64_t *at, const uint64_t *voff, int n, int64_t p) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (at[mid] <= p) lo = mid + 1; else hi = mid;
    }
    const int k = lo > 0 ? lo - 1 : 0;
    return voff[k] + (uint64_t)(p - at[k]);
}

// windows of the linear index a reference of `length` bases has room for
CLAIR_BIX_FN int64_t windows_of(int64_t length) {
    const int64_t capped = length < 1 ? 1 : length > POS_LIMIT ? POS_LIMIT : length;
    return (capped + ((int64_t)1 << WINDOW_SHIFT) - 1) >> WINDOW_SHIFT;
}

// ---- the first record of a batch that breaks a rule: index << 3 | verdict, so that the minimum is the first in file order
constexpr uint64_t NO_ERROR = ~0ull;
struct Detail {                  // what the message of a verdict names
    int64_t index;               // of the record in the file
    int32_t tid, pos, prev_tid, prev_pos;
    int64_t end;
    uint64_t voffset;
    uint32_t block_size;
    int32_t verdict;
};

// (host side only: the messages)
inline void describe(char *buf, size_t cap, const Detail &d) {
    switch (d.verdict) {
    case V_UNSORTED:
        snprintf(buf, cap, "record %lld (%d:%d, virtual offset %llu) comes after %d:%d: the BAM is not sorted by coordinate (samtools sort)",
                 (long long)d.index, d.tid, d.pos, (unsigned long long)d.voffset, d.prev_tid, d.prev_pos);
        break;
    case V_TOO_FAR:
        snprintf(buf, cap, "record %lld (%d:%d, virtual offset %llu) ends at %lld, beyond 2^29: a .bai cannot index it (a .csi could: out of scope)",
                 (long long)d.index, d.tid, d.pos, (unsigned long long)d.voffset, (long long)d.end);
        break;
    default:
        snprintf(buf, cap, "record %lld at virtual offset %llu is malformed: %s", (long long)d.index, (unsigned long long)d.voffset,
                 d.verdict == V_L_SEQ || d.verdict == V_FIELDS ? sizes_text(d.verdict) : d.verdict == V_TID ? "reference id not in the header" : "position below -1");
    }
}
}  // namespace clair_bix
