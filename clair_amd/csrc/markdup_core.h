// The rule of markdup_bam (docs/markdup_bam.md) that the device (csrc/markdup.hip) and its host twin (hostsrc/host_markdup.cpp) share: which
// records are examined, the end of a record (reference, unclipped 5' position, strand) from its real CIGAR, its score, the hash of its read
// name, the 32-byte summary both keep per record, the signature of a pair and the patch of the flag's high byte.  What belongs to a record --
// the frame step, the size rule, the fields, the CG:B:I walk -- is csrc/bam_record_core.h and csrc/bam_index_core.h; the block and payload
// sizes are sort_bam's (csrc/bam_sort_core.h).  Plain C++17; CLAIR_BIX_FN is `__host__ __device__ inline` in the device's translation unit.
#pragma once
#include "bam_sort_core.h"

namespace clair_md {

using namespace clair_bsort;                 // Bytes, Fields, fields, V_*, Detail, describe, PAYLOAD, SLOT, payloads_of, sort_verdict

constexpr uint32_t MIN_QUALITY = 15;         // a base quality below it adds nothing to the score
constexpr uint32_t SCORE_MAX = 0xffffffffu;
constexpr uint64_t NO_END = ~0ull;           // the end of a record that is not examined (no examined record has it: tid < 2^31 - 1)
constexpr uint32_t NO_MATE = 0xffffffffu;
constexpr int64_t MAX_RECORDS = 0x7fffffff;  // the sort's indices are 32 bits wide
constexpr uint32_t DUP_BIT_HIGH = 0x04;      // 0x400 in the flag's high byte, at the record's offset + 4 + 15

// the summary's flag bits
enum : uint32_t { S_EXAMINED = 1, S_PAIRABLE = 2, S_READ2 = 4, S_REVERSE = 8 };

struct Summary {                             // 32 bytes a record, kept for the whole file
    uint64_t end;                            // tid << 33 | (unclipped position + 2^31) << 1 | reverse strand; NO_END
    uint64_t hash;                           // of the read name; 0 when the record is not examined
    uint32_t score;
    uint32_t index;                          // of the record in the file
    uint32_t bits;                           // S_*
    uint32_t pad;
};

// the int64 words of a batch of the first read (CLAIR_MARKDUP_STATE), of _mark's info (CLAIR_MARKDUP_INFO) and the counts (CLAIR_MARKDUP_COUNTS)
enum { MS_TOTAL = 0, MS_N_RECORDS, MS_CARRY, MS_WORDS };
enum { MI_BYTES = 0, MI_PAYLOADS, MI_RECORDS, MI_WRITTEN, MI_WORDS };
enum { MC_RECORDS = 0, MC_EXAMINED, MC_PAIRS, MC_FRAGMENTS, MC_DUPLICATE_PAIRS, MC_DUPLICATE_FRAGMENTS, MC_WORDS };

// FNV-1a, 64 bit, over bytes[0 .. n), continued from h: a name may be handed over in pieces (a dword at a time)
constexpr uint64_t FNV_BASIS = 0xcbf29ce484222325ull, FNV_PRIME = 0x100000001b3ull;
CLAIR_BIX_FN uint64_t name_hash(const uint8_t *bytes, int64_t n, uint64_t h = FNV_BASIS) {
    for (int64_t i = 0; i < n; ++i) h = (h ^ bytes[i]) * FNV_PRIME;
    return h;
}

CLAIR_BIX_FN bool examined(int32_t tid, uint32_t flag) { return !(flag & 4) && tid >= 0 && !(flag & 0x900); }
CLAIR_BIX_FN uint32_t quality_score(uint32_t q) { return q >= MIN_QUALITY ? q : 0; }
CLAIR_BIX_FN uint32_t clamp_score(uint64_t sum) { return sum > SCORE_MAX ? SCORE_MAX : (uint32_t)sum; }

CLAIR_BIX_FN uint64_t end_key(int32_t tid, int64_t unclipped, bool reverse) {
    const int64_t lo = -((int64_t)1 << 31), hi = ((int64_t)1 << 31) - 1;
    const int64_t p = unclipped < lo ? lo : unclipped > hi ? hi : unclipped;
    return (uint64_t)(uint32_t)tid << 33 | (uint64_t)(uint32_t)(p - lo) << 1 | (reverse ? 1u : 0u);
}

// where the parts of a record the summary reads lie (o: a record start the frame step accepted, its sizes checked by fields())
struct Layout {
    int64_t name, cigar, qual, aux, end;
    uint32_t l_read_name, n_cigar;
    int32_t l_seq;
};
CLAIR_BIX_FN Layout layout(const Bytes &m, int64_t o) {
    Layout y;
    y.l_read_name = m.byte(o + 12);
    y.n_cigar = m.le16(o + 16);
    y.l_seq = (int32_t)m.le32(o + 20);
    y.name = o + 36;
    y.cigar = y.name + y.l_read_name;
    y.qual = y.cigar + 4ll * y.n_cigar + ((int64_t)y.l_seq + 1) / 2;
    y.aux = y.qual + y.l_seq;
    y.end = o + 4 + (int64_t)m.le32(o);
    return y;
}

// the clips and the span of the n operations at `cigar`: lead and trail are the lengths of the longest run of S and H operations at the
// front and at the back (a CIGAR of clips alone: both are all of it)
struct Clips { int64_t lead, trail, span; };
CLAIR_BIX_FN Clips clips(const Bytes &m, int64_t cigar, uint32_t n) {
    Clips c{0, 0, 0};
    bool front = true;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t v = m.le32(cigar + 4ll * i), op = v & 15, len = v >> 4;
        if (op == 4 || op == 5) {
            if (front) c.lead += len;
            c.trail += len;
        } else {
            front = false;
            c.trail = 0;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) c.span += len;
        }
    }
    return c;
}

// everything of a record's summary but its score: -> the verdict of its fields (sort_verdict: what stops the tool); *y its layout
CLAIR_BIX_FN int summarize(const Bytes &m, int64_t o, int n_ref, uint32_t index, Summary *s, Layout *y) {
    *s = Summary{NO_END, 0, 0, index, 0, 0};
    const Fields f = fields(m, o, n_ref);
    *y = layout(m, o);
    const int verdict = sort_verdict(f.verdict);
    if (verdict != V_OK || !examined(f.tid, f.flag)) return verdict;
    int64_t cigar = y->cigar;
    uint32_t n_ops = y->n_cigar;
    if (n_ops > 0 && f.pos >= 0) {
        const uint32_t c0 = m.le32(cigar);
        if ((c0 & 15) == 4 && (c0 >> 4) == (uint32_t)y->l_seq) {             // the placeholder: the real CIGAR is in CG:B:I
            uint64_t cg = (uint64_t)cigar;
            real_cigar(m, (uint64_t)y->aux, (uint64_t)y->end, n_ops, &cg, &n_ops);
            cigar = (int64_t)cg;
        }
    }
    const Clips c = clips(m, cigar, n_ops);
    const bool reverse = (f.flag & 16) != 0;
    s->end = end_key(f.tid, reverse ? (int64_t)f.pos + c.span - 1 + c.trail : (int64_t)f.pos - c.lead, reverse);
    s->hash = name_hash(m.p + y->name, y->l_read_name > 0 ? (int64_t)y->l_read_name - 1 : 0);
    s->bits = S_EXAMINED | (reverse ? S_REVERSE : 0);
    const uint32_t number = f.flag & 0xc0;
    if ((f.flag & 1) && !(f.flag & 8) && (number == 0x40 || number == 0x80)) s->bits |= S_PAIRABLE | (number == 0x80 ? S_READ2 : 0);
    return verdict;
}

// the score, a byte at a time (the host twin; the device sums a wave per record): an absent quality array starts with 0xff
CLAIR_BIX_FN uint32_t score_of(const Bytes &m, int64_t qual, int32_t l_seq) {
    if (l_seq <= 0 || m.byte(qual) == 0xff) return 0;
    uint64_t sum = 0;
    for (int32_t i = 0; i < l_seq; ++i) sum += quality_score(m.byte(qual + i));
    return clamp_score(sum);
}

// the key the pairing sorts by behind the hash: read 1, read 2, not pairable
CLAIR_BIX_FN uint32_t pair_class(uint32_t bits) { return !(bits & S_PAIRABLE) ? 2u : (bits & S_READ2) ? 1u : 0u; }

CLAIR_BIX_FN uint8_t patched(uint8_t high, bool duplicate) { return (uint8_t)((high & ~DUP_BIT_HIGH) | (duplicate ? DUP_BIT_HIGH : 0)); }

// (host side only: the wording of the capacity verdict)
inline void describe_memory(char *buf, size_t cap, int64_t records, int64_t memory) {
    snprintf(buf, cap, "the summaries of %lld records need %lld bytes, more than --memory %lld", (long long)records, (long long)(records * (int64_t)sizeof(Summary)),
             (long long)memory);
}

}  // namespace clair_md
