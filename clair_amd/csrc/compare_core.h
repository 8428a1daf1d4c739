// The rule of compare_vcf (docs/compare_vcf.md), as the code both sides run: the device kernels of csrc/compare.hip and the sequential host
// twin (hostsrc/host_compare.cpp).  Everything here works on the text where it lies -- a record holds offsets into its side's text, and
// nothing is copied -- and in integers only.  The one pass that copies is left alignment (the end of this file): a left-aligned allele is in
// general no substring of the text, so after it a side's offsets index an allele arena instead, which the join receives as its `text`.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CLAIR_CMP_HD __host__ __device__ inline
#else
#define CLAIR_CMP_HD inline
#endif

// one allele of one row: REF and ALT as offsets into the side's text, after trimming
struct clair_compare_record {
    int32_t ctg, pos;               // contig id (the table of _set_contigs), 1-based position after trimming
    uint32_t ref_off, alt_off;      // where the trimmed alleles start in the text
    uint16_t ref_len, alt_len;
    uint16_t qual_bin;              // min(integer part of QUAL, 1023); 0 for "."
    uint8_t copies, type;           // 1 or 2; CLAIR_CMP_SNP ..
    uint32_t line;                  // 1-based line of the row in the text
    uint32_t pad;
};
static_assert(sizeof(clair_compare_record) == 32, "record layout");

enum { CLAIR_CMP_SNP = 0, CLAIR_CMP_INS = 1, CLAIR_CMP_DEL = 2, CLAIR_CMP_MNP = 3, CLAIR_CMP_TYPES = 4 };
enum { CLAIR_CMP_TP = 0, CLAIR_CMP_GT = 1, CLAIR_CMP_FP = 2, CLAIR_CMP_FN = 3, CLAIR_CMP_DUP = 4, CLAIR_CMP_OUTSIDE = 5, CLAIR_CMP_OUTCOMES = 6,
       CLAIR_CMP_PENDING = 255 };   // PENDING: inside, no duplicate, not joined yet; never leaves the library
enum { CLAIR_CMP_CALLS = 0, CLAIR_CMP_TRUTH = 1 };
enum { CLAIR_CMP_QUAL_BINS = 1024, CLAIR_CMP_KINDS = 3 };      // kinds of the QUAL histogram: tp, gt, fp (= the outcome numbers)
// the counter block of _counts (docs/compare_vcf.md has the table)
enum {
    CLAIR_CMP_AT_COUNTS = 0,                                                                      // [side][type][outcome]
    CLAIR_CMP_AT_HIST = 2 * CLAIR_CMP_TYPES * CLAIR_CMP_OUTCOMES,                                 // [type][kind][1024]
    CLAIR_CMP_AT_AT_LEAST = CLAIR_CMP_AT_HIST + CLAIR_CMP_TYPES * CLAIR_CMP_KINDS * CLAIR_CMP_QUAL_BINS,   // [type][kind][1024]
    CLAIR_CMP_AT_DROPS = CLAIR_CMP_AT_AT_LEAST + CLAIR_CMP_TYPES * CLAIR_CMP_KINDS * CLAIR_CMP_QUAL_BINS,  // [side][symbolic, unknown_contig, too_long]
    CLAIR_CMP_COUNTS = CLAIR_CMP_AT_DROPS + 2 * 3
};
// what a line is: skipped, a data row, or the first thing wrong with it
enum { CLAIR_CMP_ROW_SKIP = 0, CLAIR_CMP_ROW_DATA = 1, CLAIR_CMP_BAD_COLUMNS = 2, CLAIR_CMP_BAD_POS = 3, CLAIR_CMP_BAD_QUAL = 4, CLAIR_CMP_BAD_FORMAT = 5,
       CLAIR_CMP_BAD_GT = 6, CLAIR_CMP_BAD_ALLELE = 7 };
// what became of a record slot of a row: none, kept, or dropped and counted
enum { CLAIR_CMP_SLOT_NONE = 0, CLAIR_CMP_SLOT_KEPT = 1, CLAIR_CMP_SLOT_SYMBOLIC = 2, CLAIR_CMP_SLOT_CONTIG = 3, CLAIR_CMP_SLOT_LONG = 4 };
enum { CLAIR_CMP_STATS = 8 };      // _parse: lines, rows, records, symbolic, unknown_contig, too_long, sorted, 0
// _left_align: its stats[8], and what the pass makes of a record
enum { CLAIR_CMP_LA_EXAMINED = 0, CLAIR_CMP_LA_SHIFTED = 1, CLAIR_CMP_LA_REF_MISMATCH = 2, CLAIR_CMP_LA_AT_CONTIG_START = 3, CLAIR_CMP_LA_NO_SEQUENCE = 4,
       CLAIR_CMP_LA_SORTED = 5, CLAIR_CMP_LA_ARENA = 6 };
enum { CLAIR_CMP_LA_UNTOUCHED = 0, CLAIR_CMP_LA_IS_NO_SEQUENCE = 1, CLAIR_CMP_LA_IS_REF_MISMATCH = 2, CLAIR_CMP_LA_COMPLEX = 3, CLAIR_CMP_LA_CANDIDATE = 4 };
#define CLAIR_CMP_MAX_POS 2000000000

CLAIR_CMP_HD const char *clair_compare_row_error(int code) {
    switch (code) {
    case CLAIR_CMP_BAD_COLUMNS: return "fewer than 10 tab-separated columns";
    case CLAIR_CMP_BAD_POS: return "POS is not [0-9]+ (at most 2000000000)";
    case CLAIR_CMP_BAD_QUAL: return "QUAL is neither . nor [0-9]+(.[0-9]*)?";
    case CLAIR_CMP_BAD_FORMAT: return "FORMAT has no GT";
    case CLAIR_CMP_BAD_GT: return "GT is not one or two allele indices of this row separated by / or |";
    case CLAIR_CMP_BAD_ALLELE: return "empty REF or ALT allele";
    }
    return "";
}

struct clair_compare_contigs {
    const uint8_t *names;      // the names one after the other; name k = names[off[k] .. off[k + 1])
    const int64_t *off;        // [n + 1]
    int32_t n;
};
// sorted, merged intervals of all contigs: those of contig k are [first[k], first[k + 1]); first == NULL: no bed file, everything is inside
struct clair_compare_regions {
    const int64_t *first, *starts, *ends;
};
// the two record slots of a row
struct clair_compare_row {
    clair_compare_record rec[2];
    uint8_t slot[2];           // CLAIR_CMP_SLOT_*
};

CLAIR_CMP_HD uint8_t clair_compare_upper(uint8_t c) { return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c; }
CLAIR_CMP_HD bool clair_compare_digit(uint8_t c) { return c >= '0' && c <= '9'; }
CLAIR_CMP_HD int64_t clair_compare_key(const clair_compare_record &r) { return (int64_t)(((uint64_t)(uint32_t)r.ctg << 32) | (uint32_t)r.pos); }

// QUAL in t[b, e) -> its bin; false: not a QUAL
CLAIR_CMP_HD bool clair_compare_qual_bin(const uint8_t *t, int64_t b, int64_t e, int *bin) {
    if (e - b == 1 && t[b] == '.') { *bin = 0; return true; }
    int64_t i = b;
    int v = 0;
    for (; i < e && clair_compare_digit(t[i]); ++i) { v = v * 10 + (t[i] - '0'); if (v > CLAIR_CMP_QUAL_BINS - 1) v = CLAIR_CMP_QUAL_BINS - 1; }
    if (i == b) return false;
    if (i < e) {
        if (t[i] != '.') return false;
        for (++i; i < e && clair_compare_digit(t[i]); ++i) {}
        if (i < e) return false;
    }
    *bin = v;
    return true;
}

// one allele index of a GT at t[*i ..e): "." counts as 0; saturates far above any ALT count
CLAIR_CMP_HD bool clair_compare_gt_index(const uint8_t *t, int64_t *i, int64_t e, int *idx) {
    if (*i < e && t[*i] == '.') { *idx = 0; ++*i; return true; }
    const int64_t b = *i;
    int v = 0;
    for (; *i < e && clair_compare_digit(t[*i]); ++*i) { v = v * 10 + (t[*i] - '0'); if (v > (1 << 20)) v = 1 << 20; }
    *idx = v;
    return *i > b;
}

CLAIR_CMP_HD bool clair_compare_symbolic(const uint8_t *t, int64_t b, int64_t e) {
    if (e - b == 1 && (t[b] == '*' || t[b] == '.')) return true;
    for (int64_t i = b; i < e; ++i) if (t[i] == '<' || t[i] == '[' || t[i] == ']') return true;
    return false;
}

CLAIR_CMP_HD int clair_compare_type(int ref_len, int alt_len) {
    return ref_len < alt_len ? CLAIR_CMP_INS : ref_len > alt_len ? CLAIR_CMP_DEL : ref_len == 1 ? CLAIR_CMP_SNP : CLAIR_CMP_MNP;
}

// the contig named t[b, e): its id, or -1
CLAIR_CMP_HD int clair_compare_contig(const clair_compare_contigs &c, const uint8_t *t, int64_t b, int64_t e) {
    for (int k = 0; k < c.n; ++k) {
        const int64_t at = c.off[k], len = c.off[k + 1] - at;
        if (len != e - b) continue;
        int64_t i = 0;
        while (i < len && c.names[at + i] == t[b + i]) ++i;
        if (i == len) return k;
    }
    return -1;
}

// suffix first, then prefix, while both alleles keep a base; the alleles compare upper-cased
CLAIR_CMP_HD void clair_compare_trim(const uint8_t *t, int64_t *ref, int64_t *ref_len, int64_t *alt, int64_t *alt_len, int64_t *pos) {
    while (*ref_len > 1 && *alt_len > 1 && clair_compare_upper(t[*ref + *ref_len - 1]) == clair_compare_upper(t[*alt + *alt_len - 1])) { --*ref_len; --*alt_len; }
    while (*ref_len > 1 && *alt_len > 1 && clair_compare_upper(t[*ref]) == clair_compare_upper(t[*alt])) { ++*ref; ++*alt; --*ref_len; --*alt_len; ++*pos; }
}

// The line t[b, e) (no line feed), 1-based `line` of its text -> CLAIR_CMP_ROW_SKIP, _DATA with both slots of *out set, or CLAIR_CMP_BAD_*.
CLAIR_CMP_HD int clair_compare_parse_line(const uint8_t *t, int64_t b, int64_t e, uint32_t line, const clair_compare_contigs &contigs, clair_compare_row *out) {
    out->slot[0] = out->slot[1] = CLAIR_CMP_SLOT_NONE;
    if (e > b && t[e - 1] == '\r') --e;
    if (e == b || t[b] == '#') return CLAIR_CMP_ROW_SKIP;
    int64_t col[11];               // column k = t[col[k], col[k + 1] - 1)
    int n_col = 1;
    col[0] = b;
    for (int64_t i = b; i < e && n_col < 10; ++i) if (t[i] == '\t') col[n_col++] = i + 1;
    if (n_col < 10) return CLAIR_CMP_BAD_COLUMNS;
    {
        int64_t i = col[9];
        while (i < e && t[i] != '\t') ++i;
        col[10] = i + 1;           // the first sample ends at the next tab or at the end of the line
    }
    // POS
    int64_t pos = 0;
    if (col[2] - 1 == col[1]) return CLAIR_CMP_BAD_POS;
    for (int64_t i = col[1]; i < col[2] - 1; ++i) {
        if (!clair_compare_digit(t[i])) return CLAIR_CMP_BAD_POS;
        pos = pos * 10 + (t[i] - '0');
        if (pos > CLAIR_CMP_MAX_POS) return CLAIR_CMP_BAD_POS;
    }
    int qual_bin = 0;
    if (!clair_compare_qual_bin(t, col[5], col[6] - 1, &qual_bin)) return CLAIR_CMP_BAD_QUAL;
    // the index of GT among the subfields of FORMAT
    int gt_at = -1;
    {
        int k = 0;
        int64_t s = col[8];
        for (int64_t i = col[8]; i <= col[9] - 1; ++i) {
            if (i == col[9] - 1 || t[i] == ':') {
                if (i - s == 2 && t[s] == 'G' && t[s + 1] == 'T') { gt_at = k; break; }
                ++k;
                s = i + 1;
            }
        }
    }
    if (gt_at < 0) return CLAIR_CMP_BAD_FORMAT;
    // that subfield of the first sample
    int64_t gb = col[9], ge = col[10] - 1;
    {
        int k = 0;
        int64_t s = col[9];
        bool found = false;
        for (int64_t i = col[9]; i <= col[10] - 1; ++i) {
            if (i == col[10] - 1 || t[i] == ':') {
                if (k == gt_at) { gb = s; ge = i; found = true; break; }
                ++k;
                s = i + 1;
            }
        }
        if (!found) return CLAIR_CMP_BAD_GT;
    }
    int idx[2] = {0, 0}, n_idx = 1;
    {
        int64_t i = gb;
        if (!clair_compare_gt_index(t, &i, ge, &idx[0])) return CLAIR_CMP_BAD_GT;
        if (i < ge) {
            if (t[i] != '/' && t[i] != '|') return CLAIR_CMP_BAD_GT;
            ++i;
            if (!clair_compare_gt_index(t, &i, ge, &idx[1]) || i != ge) return CLAIR_CMP_BAD_GT;
            n_idx = 2;
        }
    }
    int n_alt = 1;
    for (int64_t i = col[4]; i < col[5] - 1; ++i) n_alt += t[i] == ',';
    if (idx[0] > n_alt || idx[1] > n_alt) return CLAIR_CMP_BAD_GT;
    if (col[4] - 1 == col[3]) return CLAIR_CMP_BAD_ALLELE;
    // one record per distinct non-zero index, in the order of the GT
    int want[2], copies[2], n_want = 0;
    if (idx[0] != 0) { want[n_want] = idx[0]; copies[n_want++] = 1 + (n_idx == 2 && idx[1] == idx[0]); }
    if (n_idx == 2 && idx[1] != 0 && idx[1] != idx[0]) { want[n_want] = idx[1]; copies[n_want++] = 1; }
    int ctg = -2;                  // looked up once, and only for a row that has a record
    for (int w = 0; w < n_want; ++w) {
        int64_t ab = col[4], ae = col[4];
        for (int k = 1;; ++k) {    // ALT number want[w]
            ae = ab;
            while (ae < col[5] - 1 && t[ae] != ',') ++ae;
            if (k == want[w]) break;
            ab = ae + 1;
        }
        if (ae == ab) return CLAIR_CMP_BAD_ALLELE;
        if (clair_compare_symbolic(t, ab, ae)) { out->slot[w] = CLAIR_CMP_SLOT_SYMBOLIC; continue; }
        if (ctg == -2) ctg = clair_compare_contig(contigs, t, col[0], col[1] - 1);
        if (ctg < 0) { out->slot[w] = CLAIR_CMP_SLOT_CONTIG; continue; }
        int64_t ref = col[3], ref_len = col[4] - 1 - col[3], alt = ab, alt_len = ae - ab, p = pos;
        if (ref_len > 65535 || alt_len > 65535) { out->slot[w] = CLAIR_CMP_SLOT_LONG; continue; }
        clair_compare_trim(t, &ref, &ref_len, &alt, &alt_len, &p);
        clair_compare_record &r = out->rec[w];
        r.ctg = ctg; r.pos = (int32_t)p;
        r.ref_off = (uint32_t)ref; r.alt_off = (uint32_t)alt;
        r.ref_len = (uint16_t)ref_len; r.alt_len = (uint16_t)alt_len;
        r.qual_bin = (uint16_t)qual_bin;
        r.copies = (uint8_t)copies[w]; r.type = (uint8_t)clair_compare_type((int)ref_len, (int)alt_len);
        r.line = line; r.pad = 0;
        out->slot[w] = CLAIR_CMP_SLOT_KEPT;
    }
    return CLAIR_CMP_ROW_DATA;
}

// same REF and ALT, upper-cased (a and b may lie in two texts)
CLAIR_CMP_HD bool clair_compare_same_alleles(const uint8_t *ta, const clair_compare_record &a, const uint8_t *tb, const clair_compare_record &b) {
    if (a.ref_len != b.ref_len || a.alt_len != b.alt_len) return false;
    for (uint32_t i = 0; i < a.ref_len; ++i) if (clair_compare_upper(ta[a.ref_off + i]) != clair_compare_upper(tb[b.ref_off + i])) return false;
    for (uint32_t i = 0; i < a.alt_len; ++i) if (clair_compare_upper(ta[a.alt_off + i]) != clair_compare_upper(tb[b.alt_off + i])) return false;
    return true;
}

// start < pos <= end for one interval of the contig (BED is 0-based and half-open, pos 1-based)
CLAIR_CMP_HD bool clair_compare_inside(const clair_compare_regions &g, int32_t ctg, int64_t pos) {
    if (!g.first) return true;
    int64_t lo = g.first[ctg], hi = g.first[ctg + 1];
    const int64_t base = lo;
    while (lo < hi) {              // -> the number of intervals that start before pos
        const int64_t mid = lo + (hi - lo) / 2;
        if (g.starts[mid] < pos) lo = mid + 1; else hi = mid;
    }
    return lo > base && pos <= g.ends[lo - 1];
}

// record i of a side in (contig, pos, file) order: DUP when a record before it has its contig, pos, REF and ALT, else OUTSIDE or PENDING
CLAIR_CMP_HD uint8_t clair_compare_classify(const clair_compare_record *r, const uint8_t *text, int64_t i, const clair_compare_regions &g) {
    const clair_compare_record me = r[i];
    const int64_t key = clair_compare_key(me);
    for (int64_t j = i - 1; j >= 0 && clair_compare_key(r[j]) == key; --j)
        if (clair_compare_same_alleles(text, r[j], text, me)) return CLAIR_CMP_DUP;
    return clair_compare_inside(g, me.ctg, me.pos) ? CLAIR_CMP_PENDING : CLAIR_CMP_OUTSIDE;
}

// the truth record a call matches: the first one with its contig, pos, REF and ALT (the one that is no duplicate), or -1
CLAIR_CMP_HD int64_t clair_compare_find(const clair_compare_record *truth, int64_t n_truth, const uint8_t *truth_text, const clair_compare_record &call,
                                        const uint8_t *call_text) {
    const int64_t key = clair_compare_key(call);
    int64_t lo = 0, hi = n_truth;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (clair_compare_key(truth[mid]) < key) lo = mid + 1; else hi = mid;
    }
    for (; lo < n_truth && clair_compare_key(truth[lo]) == key; ++lo)
        if (clair_compare_same_alleles(truth_text, truth[lo], call_text, call)) return lo;
    return -1;
}

// -- left alignment (docs/compare_vcf.md, "Left alignment"): per record, after the trimming and before order, duplicates, regions and join ------
// the sequences of the contig table one after the other: contig k = seq[off[k] .. off[k + 1]), an empty range = no sequence loaded
struct clair_compare_reference {
    const uint8_t *seq;
    const int64_t *off;        // [n + 1]
};
// an indel whose shorter allele is one byte b, at text[b_off], and whose longer one is W of len + 1 bytes, at text[w_off]: the len event bytes X
// start at text[x_off], and the anchor, the base before the event, is at the 1-based position a of the contig (0: before its first base).
// With V = G[1 .. a] ++ X the event may move left while V[a + len - j] == V[a - j].
struct clair_compare_event {
    int64_t a;
    uint32_t x_off, len, w_off, b_off;
};

// What the pass makes of a record.  Not an indel: not examined.  Then the first that applies: no sequence for its contig; REF differs from the
// reference at pos, or lies outside the contig; the closed form does not apply (the literal loop of the docs leaves such a record as it is);
// otherwise a candidate for the run search, with *ev set.
CLAIR_CMP_HD int clair_compare_la_case(const clair_compare_reference &g, const uint8_t *t, const clair_compare_record &r, clair_compare_event *ev) {
    const uint32_t ref_len = r.ref_len, alt_len = r.alt_len, ref_off = r.ref_off, alt_off = r.alt_off;
    const int64_t pos = r.pos;
    if (ref_len == alt_len) return CLAIR_CMP_LA_UNTOUCHED;
    const int64_t at = g.off[r.ctg], len = g.off[r.ctg + 1] - at;
    if (len == 0) return CLAIR_CMP_LA_IS_NO_SEQUENCE;
    if (pos < 1 || pos - 1 + ref_len > len) return CLAIR_CMP_LA_IS_REF_MISMATCH;
    for (uint32_t i = 0; i < ref_len; ++i)
        if (clair_compare_upper(t[ref_off + i]) != clair_compare_upper(g.seq[at + pos - 1 + i])) return CLAIR_CMP_LA_IS_REF_MISMATCH;
    const bool ins = ref_len < alt_len;
    if ((ins ? ref_len : alt_len) != 1) return CLAIR_CMP_LA_COMPLEX;
    const uint32_t w = ins ? alt_off : ref_off, n = (ins ? alt_len : ref_len) - 1u, b_off = ins ? ref_off : alt_off;
    const uint8_t b = clair_compare_upper(t[b_off]);
    const bool at_end = clair_compare_upper(t[w + n]) == b;      // W ends in b: X = W[0 .. n - 1] behind the anchor at pos - 1; else W begins with b
    if (!at_end && clair_compare_upper(t[w]) != b) return CLAIR_CMP_LA_COMPLEX;
    ev->a = pos - (at_end ? 1 : 0);
    ev->x_off = w + (at_end ? 0u : 1u);
    ev->len = n;
    ev->w_off = w;
    ev->b_off = b_off;
    return CLAIR_CMP_LA_CANDIDATE;
}

// V[i], upper-cased, for 1 <= i <= a + len; contig = where the record's own contig starts in the reference, so no other contig is ever read
CLAIR_CMP_HD uint8_t clair_compare_la_v(const uint8_t *contig, const uint8_t *t, const clair_compare_event &ev, int64_t i) {
    return clair_compare_upper(i <= ev.a ? contig[i - 1] : t[ev.x_off + (i - ev.a - 1)]);
}

// does the event stop after j steps to the left: the contig's start is reached, or the bytes differ
CLAIR_CMP_HD bool clair_compare_la_stops(const uint8_t *contig, const uint8_t *t, const clair_compare_event &ev, int64_t j) {
    return ev.a - j < 1 || clair_compare_la_v(contig, t, ev, ev.a + ev.len - j) != clair_compare_la_v(contig, t, ev, ev.a - j);
}

// The alleles of a candidate that stopped after `steps`.  a - steps < 1 is at_contig_start: it keeps its own bytes.  Otherwise the anchor
// G[a - steps] is the shorter allele and the first byte of the longer one, and the event bytes behind it are V[a - steps + 1 ..].
CLAIR_CMP_HD uint8_t clair_compare_la_long_byte(const uint8_t *contig, const uint8_t *t, const clair_compare_event &ev, int64_t steps, uint32_t k) {
    return ev.a - steps < 1 ? clair_compare_upper(t[ev.w_off + k]) : clair_compare_la_v(contig, t, ev, ev.a - steps + k);
}
CLAIR_CMP_HD uint8_t clair_compare_la_short_byte(const uint8_t *contig, const uint8_t *t, const clair_compare_event &ev, int64_t steps) {
    return ev.a - steps < 1 ? clair_compare_upper(t[ev.b_off]) : clair_compare_la_v(contig, t, ev, ev.a - steps);
}

// a record the pass leaves as it is: its alleles go upper-cased to its slot of the arena, REF first, ALT behind it
CLAIR_CMP_HD void clair_compare_la_copy(const uint8_t *t, const clair_compare_record &r, uint32_t slot, uint8_t *arena) {
    const uint32_t ref_len = r.ref_len, alt_len = r.alt_len, ref_off = r.ref_off, alt_off = r.alt_off;
    for (uint32_t i = 0; i < ref_len; ++i) arena[slot + i] = clair_compare_upper(t[ref_off + i]);
    for (uint32_t i = 0; i < alt_len; ++i) arena[slot + ref_len + i] = clair_compare_upper(t[alt_off + i]);
}
