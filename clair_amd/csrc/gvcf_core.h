// The reference-confidence rule of the gVCF stage (docs/gvcf.md), shared by the device (csrc/gvcf.hip, part of frontend.hip's translation
// unit) and the host twin (hostsrc/host_gvcf.cpp): the includer defines CLAIR_GVCF_FN (`__device__ __host__ inline` / `static inline`), as
// bam_record_core.h has its includers define CLAIR_REC_FN.  Integers only: the three costs come in as fixed-point numbers (1/1024 phred)
// that Python worked out once from --gvcf_error_rate, so no floating point decides a byte of the output on either side.
//
// Per 0-based position the candidate search's seven tallies t[0..6] = A C G T I D N (what fe_candidate_flags_kernel reads):
//   DP = A + C + G + T + N            the candidate filter's depth
//   R  = max(0, t[r] - I - D)         r: the search's index of the reference base (none: R = 0); a read that opens an indel right after the
//                                     position is evidence against the reference where a VCF anchors that indel
//   A  = DP - R
//   S00 = R c_match + A c_err, S01 = DP c_half, S11 = R c_err + A c_match, m = min;  PLg = (Sg - m + 512) >> 10
//   GQ = min(99, PL01, PL11) when S00 == m, else 0 (blocks are written 0/0 whatever the counts say: GQ 0 is "no confidence")
// With 21-bit counters DP < 2^24 and costs < 2^17: every sum fits 64 bits with room to spare, every PL 32.
#pragma once
#include <stdint.h>

#ifndef CLAIR_GVCF_TYPES
#define CLAIR_GVCF_TYPES
typedef struct clair_gvcf_block {
    int64_t start, end;
    uint32_t min_dp, dp;
    int32_t gq;
    int32_t pl[3];
} clair_gvcf_block_t;
#endif

static_assert(sizeof(clair_gvcf_block_t) == 40, "block record layout");

#define CLAIR_GVCF_MAX_COST ((1 << 17) - 1)
#define CLAIR_GVCF_GQ_VALUES 100

struct clair_gvcf_costs { int32_t c_match, c_err, c_half; };
struct clair_gvcf_bands { uint8_t of[CLAIR_GVCF_GQ_VALUES]; };      // band of a GQ value 0 .. 99
struct clair_gvcf_site { uint32_t dp; int32_t gq; int32_t pl[3]; };

// the search's index of a reference base (BASES.evc of frontend.hip: IUPAC codes through IUPAC_base_to_ACGT_base_dict): 0 .. 3, or -1 for N and for
// what is no key
CLAIR_GVCF_FN int clair_gvcf_ref_index(uint8_t c) {
    if (c >= 'a' && c <= 'z') c = (uint8_t)(c - 32);
    switch (c) {
    case 'A': case 'R': case 'W': case 'M': case 'D': case 'H': case 'V': return 0;
    case 'C': case 'Y': case 'S': case 'B': return 1;
    case 'G': case 'K': return 2;
    case 'T': case 'U': return 3;
    default: return -1;
    }
}

CLAIR_GVCF_FN clair_gvcf_site clair_gvcf_rule(const uint32_t t[7], int r, const clair_gvcf_costs &c) {
    const int64_t dp = (int64_t)t[0] + t[1] + t[2] + t[3] + t[6];
    int64_t ref = 0;
    if (r >= 0) {
        ref = (int64_t)t[r] - (int64_t)t[4] - (int64_t)t[5];
        if (ref < 0) ref = 0;
    }
    const int64_t alt = dp - ref;
    const int64_t s00 = ref * c.c_match + alt * c.c_err, s01 = dp * c.c_half, s11 = ref * c.c_err + alt * c.c_match;
    int64_t m = s00 < s01 ? s00 : s01;
    if (s11 < m) m = s11;
    clair_gvcf_site out;
    out.dp = (uint32_t)dp;
    out.pl[0] = (int32_t)((s00 - m + 512) >> 10);
    out.pl[1] = (int32_t)((s01 - m + 512) >> 10);
    out.pl[2] = (int32_t)((s11 - m + 512) >> 10);
    int32_t gq = out.pl[1] < out.pl[2] ? out.pl[1] : out.pl[2];
    if (gq > 99) gq = 99;
    out.gq = s00 == m ? gq : 0;
    return out;
}

// is 0-based position p in the allowed set (sorted, disjoint, half-open)?  *first: p opens its interval.  Bisection, as the candidate kernel
// finds bed intervals.
CLAIR_GVCF_FN bool clair_gvcf_allowed(const int64_t *iv_start, const int64_t *iv_end, int64_t n_iv, int64_t p, bool *first) {
    int64_t a = 0, b = n_iv;                                // first interval starting after p
    while (a < b) { const int64_t mid = (a + b) >> 1; if (iv_start[mid] <= p) a = mid + 1; else b = mid; }
    if (a == 0 || !(p < iv_end[a - 1])) return false;
    *first = iv_start[a - 1] == p;
    return true;
}

// The running value of the segmentation: what the positions since the last block head (inclusive) amount to.  heads counts the block heads
// of the whole range, so that the value in front of a block's last position also says which record it is.
struct clair_gvcf_run {
    uint32_t heads, start;      // start: offset of the head from the first table position
    uint32_t min_dp;
    int32_t gq;
    uint64_t sum_dp;
    int32_t pl[3];
    uint32_t pad;
};

CLAIR_GVCF_FN clair_gvcf_run clair_gvcf_run_identity() { return clair_gvcf_run{0u, 0xffffffffu, 0xffffffffu, INT32_MAX, 0ull, {INT32_MAX, INT32_MAX, INT32_MAX}, 0u}; }

CLAIR_GVCF_FN clair_gvcf_run clair_gvcf_run_of(const clair_gvcf_site &s, bool head, uint32_t at) {
    return clair_gvcf_run{head ? 1u : 0u, head ? at : 0xffffffffu, s.dp, s.gq, (uint64_t)s.dp, {s.pl[0], s.pl[1], s.pl[2]}, 0u};
}

// a: the earlier range.  Associative: the segmented form of (min, sum), a head in b cutting off what a carries.
CLAIR_GVCF_FN clair_gvcf_run clair_gvcf_run_join(const clair_gvcf_run &a, const clair_gvcf_run &b) {
    clair_gvcf_run o = b;
    o.heads = a.heads + b.heads;
    if (b.heads) return o;
    o.start = a.start;
    o.min_dp = a.min_dp < b.min_dp ? a.min_dp : b.min_dp;
    o.gq = a.gq < b.gq ? a.gq : b.gq;
    o.sum_dp = a.sum_dp + b.sum_dp;
    for (int g = 0; g < 3; ++g) o.pl[g] = a.pl[g] < b.pl[g] ? a.pl[g] : b.pl[g];
    return o;
}

// the record of the block whose positions (head .. last, `last` an offset like start) amount to v
CLAIR_GVCF_FN clair_gvcf_block_t clair_gvcf_block_of(const clair_gvcf_run &v, int64_t lo, uint32_t last) {
    clair_gvcf_block_t b;
    b.start = lo + (int64_t)v.start;
    b.end = lo + (int64_t)last + 1;
    b.min_dp = v.min_dp;
    b.dp = (uint32_t)(v.sum_dp / (uint64_t)(b.end - b.start));
    b.gq = v.gq;
    for (int g = 0; g < 3; ++g) b.pl[g] = v.pl[g];
    return b;
}

// ---- arguments both backends check the same way, in the same words (host code) --------------------------------------------------------
#include <stdio.h>
// 0: fine; otherwise `msg` says what is wrong with the costs, the band table or the allowed intervals over tables [lo, lo + n)
static inline int clair_gvcf_check_arguments(int c_match, int c_err, int c_half, const uint8_t *band_of_gq, const int64_t *iv_start, const int64_t *iv_end, int64_t n_iv,
                                             int64_t lo, int64_t n, char *msg, size_t cap) {
    const int cost[3] = {c_match, c_err, c_half};
    const char *name[3] = {"c_match", "c_err", "c_half"};
    for (int k = 0; k < 3; ++k)
        if (cost[k] < 1 || cost[k] > CLAIR_GVCF_MAX_COST) { snprintf(msg, cap, "gvcf: cost %s = %d is outside 1 .. %d", name[k], cost[k], CLAIR_GVCF_MAX_COST); return 1; }
    if (!band_of_gq) { snprintf(msg, cap, "gvcf: band table missing"); return 1; }
    for (int g = 1; g < CLAIR_GVCF_GQ_VALUES; ++g)
        if (band_of_gq[g] < band_of_gq[g - 1]) { snprintf(msg, cap, "gvcf: band table decreases at GQ %d", g); return 1; }
    if (n_iv < 0 || (n_iv > 0 && (!iv_start || !iv_end))) { snprintf(msg, cap, "gvcf: allowed intervals missing"); return 1; }
    for (int64_t i = 0; i < n_iv; ++i) {
        if (iv_end[i] <= iv_start[i]) { snprintf(msg, cap, "gvcf: allowed interval %lld [%lld, %lld) is empty", (long long)i, (long long)iv_start[i], (long long)iv_end[i]); return 1; }
        if (i > 0 && iv_start[i] < iv_end[i - 1]) {
            snprintf(msg, cap, "gvcf: allowed interval %lld [%lld, %lld) starts before interval %lld ends (%lld): the list is sorted and disjoint", (long long)i,
                     (long long)iv_start[i], (long long)iv_end[i], (long long)(i - 1), (long long)iv_end[i - 1]);
            return 1;
        }
        if (iv_start[i] < lo || iv_end[i] > lo + n) {
            snprintf(msg, cap, "gvcf: allowed interval %lld [%lld, %lld) lies outside the tables [%lld, %lld)", (long long)i, (long long)iv_start[i], (long long)iv_end[i],
                     (long long)lo, (long long)(lo + n));
            return 1;
        }
    }
    return 0;
}
