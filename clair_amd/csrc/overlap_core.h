// The rule of the overlap filter, one pair of VCF rows at a time: shared by the device path (csrc/overlap.hip: clair_overlap_keep) and the
// host twin (hostsrc/host_overlap.cpp: clair_host_overlap_keep).  docs/overlap_variant.md derives it from the reference's
// clair/post_processing/overlap_variant.py; nothing else in the native code restates it.
//
// A row is reduced to a span (clair_amd/overlap_variant.py parses the text and renders the rows that stay):
//   ctg    the contig as an id (equal ids <=> equal names)
//   pos    POS
//   qual   int(float(QUAL))
//   del    len(REF) - min(len(ALT1), len(ALT2) if there is one else 1024): the longest deletion, <= 0 when there is none (:29-33)
//   flags  CLAIR_OVERLAP_SNP: len(REF) == len(ALT1), or there is an ALT2 and len(REF) == len(ALT2) (:36-45)
// The reference's insertion intervals are computed and never used (:128-152); they are not here.
#ifndef CLAIR_OVERLAP_CORE_H
#define CLAIR_OVERLAP_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CLAIR_OV_HD __host__ __device__
#else
#define CLAIR_OV_HD
#endif

struct clair_overlap_span {     // 24 bytes, little endian: clair_amd/overlap_variant.py SPAN_DTYPE
    int64_t pos;
    int32_t ctg;
    int32_t qual;
    int32_t del;
    uint32_t flags;
};
#define CLAIR_OVERLAP_SNP 1u

// the row has something a deletion before it can cover: a "SNP" interval or a deletion interval of its own
CLAIR_OV_HD inline bool clair_overlap_body(const clair_overlap_span &v) { return (v.flags & CLAIR_OVERLAP_SNP) != 0 || v.del > 0; }

// the last position a's deletion covers, in 64 bits (POS near 2^31 does not wrap); meaningful where a.del > 0
CLAIR_OV_HD inline int64_t clair_overlap_reach(const clair_overlap_span &a) { return a.pos + (int64_t)a.del; }

// is_two_variants_overlap (:122-152): the row at the lower position is the one whose deletion counts (equal positions: L's)
CLAIR_OV_HD inline bool clair_overlap(const clair_overlap_span &L, const clair_overlap_span &v) {
    if (L.ctg != v.ctg) return false;
    const clair_overlap_span &a = L.pos <= v.pos ? L : v, &b = L.pos <= v.pos ? v : L;
    return a.del > 0 && clair_overlap_body(b) && b.pos <= clair_overlap_reach(a);
}

// variant_to_output_for (:228-234) for a pair that overlaps: the later row takes the place of the last kept one unless that one's QUAL is higher
CLAIR_OV_HD inline bool clair_overlap_replaces(const clair_overlap_span &L, const clair_overlap_span &v) { return !(L.qual > v.qual); }

// filter_variants_with (:237-267) over rows [from, to), the first of which is kept whatever came before it: keep[i] = 1 for the rows
// that stay.  L is the last row kept; a row that replaces it clears its byte.
CLAIR_OV_HD inline void clair_overlap_walk(const clair_overlap_span *s, int64_t from, int64_t to, uint8_t *keep) {
    if (from >= to) return;
    int64_t last = from;
    clair_overlap_span L = s[from];
    keep[from] = 1;
    for (int64_t i = from + 1; i < to; ++i) {
        const clair_overlap_span v = s[i];
        if (!clair_overlap(L, v)) {
            keep[i] = 1;
        } else if (clair_overlap_replaces(L, v)) {
            keep[last] = 0;
            keep[i] = 1;
        } else {
            keep[i] = 0;
            continue;
        }
        last = i;
        L = v;
    }
}

#endif /* CLAIR_OVERLAP_CORE_H */
