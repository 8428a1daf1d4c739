// The rules of one BAM record that every reader of records here shares: the host reader and renderer (hostsrc/host_bam.cpp), the device
// front end's decoder (csrc/frontend.hip) and index_bam on both sides (csrc/bam_index_core.h).  Little-endian fields, the frame step over a
// stream of records, the size rule of a record's fixed and variable parts, the reference span of a binary CIGAR and the aux walk to the real
// CIGAR of a record that stores the placeholder.  Plain C++17 over a small memory context: byte(at) and le32(at) at any byte offset.  Bytes
// is the context over plain pointers; the device front end's reads 32-bit values as two aligned dwords.  CLAIR_REC_FN is `__device__ inline`
// or `__host__ __device__ inline` in a device translation unit.
#pragma once
#include <climits>
#include <cstdint>
#include <cstdio>

#ifndef CLAIR_REC_FN
#define CLAIR_REC_FN inline
#endif

namespace clair_rec {

CLAIR_REC_FN uint32_t u16(const uint8_t *p) { return (uint32_t)(p[0] | p[1] << 8); }
CLAIR_REC_FN uint32_t u32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

struct Bytes {
    const uint8_t *p;
    CLAIR_REC_FN uint32_t byte(int64_t at) const { return p[at]; }
    CLAIR_REC_FN uint32_t le16(int64_t at) const { return u16(p + at); }
    CLAIR_REC_FN uint32_t le32(int64_t at) const { return u32(p + at); }
};

// ---- the frame step.  A record at o is its size word and block_size bytes; the next one starts right behind it.  No address is ever formed
// from a size word that was not checked: at an offset that is no record start the word is garbage, and that is the normal case.
enum { STEP_NEXT = 0, STEP_BAD = 1, STEP_PAST = 2 };       // BAD: no record can start here; PAST: it would not end inside the stream
CLAIR_REC_FN int step(const Bytes &m, int64_t o, int64_t len, int64_t *next) {
    if (o + 4 > len) return STEP_PAST;
    const uint32_t block_size = m.le32(o);
    if (block_size < 32 || (uint64_t)block_size + 4 > (uint64_t)INT32_MAX) return STEP_BAD;
    if (o + 4 + (int64_t)block_size > len) return STEP_PAST;
    *next = o + 4 + (int64_t)block_size;
    return STEP_NEXT;
}
// (host side only: the frame verdicts as words)
inline void describe_bad_step(char *buf, size_t cap, uint64_t voffset, uint32_t block_size) {
    if (block_size < 32) snprintf(buf, cap, "record at virtual offset %llu: block_size %u < 32", (unsigned long long)voffset, block_size);
    else snprintf(buf, cap, "record at virtual offset %llu: block_size %u", (unsigned long long)voffset, block_size);
}
inline void describe_cut(char *buf, size_t cap, uint64_t voffset) {
    snprintf(buf, cap, "the stream ends inside a record (virtual offset %llu)", (unsigned long long)voffset);
}

// ---- the size rule: the fixed part, the read name, the stored CIGAR, SEQ and QUAL lie inside block_size.  -> the first clause that fails.
// SIZES_NAME here is the empty read name; that a name ends in NUL is the renderer's to look at (the device decoder does not read it).
enum { SIZES_OK = 0, SIZES_L_SEQ = 1, SIZES_FIELDS = 2, SIZES_NAME = 3 };
CLAIR_REC_FN int sizes_verdict(uint32_t block_size, uint32_t l_read_name, uint32_t n_cigar, int32_t l_seq) {
    if (l_seq < 0) return SIZES_L_SEQ;
    if (32ull + l_read_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > (uint64_t)block_size) return SIZES_FIELDS;
    return l_read_name == 0 ? SIZES_NAME : SIZES_OK;
}
inline const char *sizes_text(int verdict) {
    return verdict == SIZES_L_SEQ ? "negative l_seq" : verdict == SIZES_FIELDS ? "fields longer than block_size" : "read name not NUL-terminated";
}

// reference span of the n operations of a binary CIGAR at `cigar` (bam_cigar2rlen): M D N = X
template <class M>
CLAIR_REC_FN int64_t cigar_span(const M &m, int64_t cigar, uint32_t n) {
    int64_t span = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t c = m.le32(cigar + 4ll * i), op = c & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += c >> 4;
    }
    return span;
}

// A record whose stored CIGAR is the <l_seq>S<ref_len>N placeholder (more than 65 535 operations) keeps the real one in CG:B:I: htslib's
// bam_tag2cigar substitutes it when it reads the record, so `samtools view` prints it.  The aux fields are [aux, end); the caller has seen
// the placeholder, n_cigar > 0, ref_id >= 0 and pos >= 0.  -> true and the real operations' offset and count; false: the stored CIGAR stands.
template <class M>
CLAIR_REC_FN bool real_cigar(const M &m, uint64_t aux, uint64_t end, uint32_t n_cigar, uint64_t *cg_off, uint32_t *cg_n) {
    while (aux + 3 <= end) {
        const uint32_t t0 = m.byte(aux), t1 = m.byte(aux + 1), type = m.byte(aux + 2);
        const bool cg = t0 == 'C' && t1 == 'G';
        const uint64_t v = aux + 3;
        uint64_t size = 0;
        switch (type) {
        case 'A': case 'c': case 'C': size = 1; break;
        case 's': case 'S': size = 2; break;
        case 'i': case 'I': case 'f': size = 4; break;
        case 'Z': case 'H': { uint64_t z = v; while (z < end && m.byte(z)) ++z; if (z >= end) return false; size = z - v + 1; break; }
        case 'B': {
            if (v + 5 > end) return false;
            const uint32_t sub = m.byte(v);
            const uint32_t count = m.le32(v + 1);
            const uint64_t each = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : (sub == 'i' || sub == 'I' || sub == 'f') ? 4 : 0;
            if (!each || (uint64_t)count * each > end - v - 5) return false;
            if (cg) {
                if (!(sub == 'I' || sub == 'i') || count < n_cigar || count >= (1u << 29)) return false;
                *cg_off = v + 5;
                *cg_n = count;
                return true;
            }
            size = 5 + (uint64_t)count * each;
            break;
        }
        default: return false;
        }
        if (cg) return false;                // a CG tag of another type: the stored CIGAR stands (bam_tag2cigar)
        aux = v + size;
    }
    return false;
}

}  // namespace clair_rec
