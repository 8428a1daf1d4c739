// The rules of the training-set builder, one position / one window at a time: shared by the device path (csrc/train_set.hip:
// clair_frontend_sample_candidates, clair_frontend_pair) and the host twin (hostsrc/host_train_set.cpp: clair_host_train_set_*).
// docs/train_set.md derives them from the reference's dataPrepScripts/ExtractVariantCandidates.py (--gen4Training),
// dataPrepScripts/PairWithNonVariants.py and clair/utils.py (get_training_array); nothing else in the native code restates them.
//
// Draws are counter based: a draw is a function of (seed, contig, stage, position) and of nothing else, so a run is reproducible and
// two runs over differently down-sampled alignments with one seed sample the same sites wherever the depth allows.
#ifndef CLAIR_TRAIN_SET_CORE_H
#define CLAIR_TRAIN_SET_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CLAIR_TS_HD __host__ __device__
#else
#define CLAIR_TS_HD
#endif

// ---- draws -------------------------------------------------------------------------------------------------------------------------
// the finaliser of splitmix64 (also the dropout masks' hash, csrc/train_kernels.hip.h)
CLAIR_TS_HD inline uint64_t clair_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// 64-bit FNV-1a over the bytes of the contig name (host side: the kernels take the key)
inline uint64_t clair_ts_fnv1a64(const char *s, int64_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (int64_t i = 0; i < n; ++i) { h ^= (uint8_t)s[i]; h *= 0x100000001B3ull; }
    return h;
}

#define CLAIR_TS_STAGE_SAMPLE 1   /* which sites are sampled */
#define CLAIR_TS_STAGE_PAIR 2     /* which usable non-variant windows are kept */
CLAIR_TS_HD inline uint64_t clair_ts_key(uint64_t seed, uint64_t ctg_hash, uint64_t stage) {
    return clair_mix64(clair_mix64(seed) ^ clair_mix64(ctg_hash ^ stage));
}
// 53 bits for the 1-based position `pos`; u = draw * 2^-53 is uniform on [0, 1)
CLAIR_TS_HD inline uint64_t clair_ts_draw(uint64_t key, int64_t pos) { return clair_mix64(key + (uint64_t)pos) >> 11; }
CLAIR_TS_HD inline double clair_ts_u(uint64_t draw) { return (double)draw * 0x1p-53; }

// ---- membership in the bed intervals of the contig: sorted, merged, 0-based half-open; n_bed < 0: no bed file, everything is inside -----
CLAIR_TS_HD inline bool clair_ts_in_bed(const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed, int64_t p) {
    if (n_bed < 0) return true;
    int64_t a = 0, b = n_bed;                                      // first interval starting after p
    while (a < b) { const int64_t mid = (a + b) >> 1; if (bed_start[mid] <= p) a = mid + 1; else b = mid; }
    return a > 0 && p < bed_end[a - 1];
}

// ---- class of a 1-based position against the sorted truth positions (duplicates allowed) ------------------------------------------------
// The closed form of non_variants_map_near_variants_from (ExtractVariantCandidates.py:59-101): a position 15 or 16 away from a truth
// position enters the map unless one within 14 of it takes it out again, i.e. its NEAREST truth position is 15 or 16 away.
#define CLAIR_TS_OUTSIDE 0
#define CLAIR_TS_NEAR 1
#define CLAIR_TS_TRUTH 2
// first index whose truth position is >= pos
CLAIR_TS_HD inline int64_t clair_ts_lower_bound(const int64_t *truth, int64_t n_truth, int64_t pos) {
    int64_t a = 0, b = n_truth;
    while (a < b) { const int64_t mid = (a + b) >> 1; if (truth[mid] < pos) a = mid + 1; else b = mid; }
    return a;
}
CLAIR_TS_HD inline int clair_ts_class(const int64_t *truth, int64_t n_truth, int64_t pos) {
    const int64_t i = clair_ts_lower_bound(truth, n_truth, pos);
    if (i < n_truth && truth[i] == pos) return CLAIR_TS_TRUTH;
    int64_t d = INT64_MAX;
    if (i < n_truth) d = truth[i] - pos;
    if (i > 0 && pos - truth[i - 1] < d) d = pos - truth[i - 1];
    return (d == 15 || d == 16) ? CLAIR_TS_NEAR : CLAIR_TS_OUTSIDE;
}

// random.uniform(0, 1) <= p (:336-341); truth positions are never sampled (they come in through the truth list)
CLAIR_TS_HD inline bool clair_ts_sampled(int cls, uint64_t draw, double p_near, double p_outside) {
    return cls != CLAIR_TS_TRUTH && clair_ts_u(draw) <= (cls == CLAIR_TS_NEAR ? p_near : p_outside);
}

// ---- pairing (PairWithNonVariants.py:17-90) ---------------------------------------------------------------------------------------
// a non-variant window is usable when its 1-based position, AS IT STANDS, lies in the 0-based bed intervals (:43) and no truth row has it (:46)
CLAIR_TS_HD inline bool clair_ts_usable(const int64_t *truth, int64_t n_truth, const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed, int64_t pos) {
    return clair_ts_class(truth, n_truth, pos) != CLAIR_TS_TRUTH && clair_ts_in_bed(bed_start, bed_end, n_bed, pos);
}
// r = min(1, v * amp / c) (:32, :53-54); with no usable window nothing is drawn and r is reported as 1
CLAIR_TS_HD inline double clair_ts_ratio(int64_t v, double amp, int64_t c) {
    if (c == 0) return 1.0;
    const double r = ((double)v * amp) / (double)c;
    return r <= 1.0 ? r : 1.0;
}
// random() < r (:81)
CLAIR_TS_HD inline bool clair_ts_paired(uint64_t draw, double r) { return clair_ts_u(draw) < r; }

// ---- data-set membership and labels (clair/utils.py:133-220, get_training_array) ---------------------------------------------------------
// IUPAC_base_to_ACGT_base_dict over an upper-cased base as an index into ACGT; -1: not a key
CLAIR_TS_HD inline int clair_ts_acgt(uint8_t base) {
    if (base >= 'a' && base <= 'z') base -= 32;
    switch (base) {
    case 'A': case 'R': case 'W': case 'M': case 'D': case 'H': case 'V': case 'N': return 0;
    case 'C': case 'Y': case 'S': case 'B': return 1;
    case 'G': case 'K': return 2;
    case 'T': case 'U': return 3;
    default: return -1;
    }
}
// the window is part of the data set: position (as it stands) inside the bed (:145), upper-cased centre base in ACGTU (:147-149)
CLAIR_TS_HD inline bool clair_ts_in_set(const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed, int64_t pos, uint8_t centre) {
    if (centre >= 'a' && centre <= 'z') centre -= 32;
    const bool basic = centre == 'A' || centre == 'C' || centre == 'G' || centre == 'T' || centre == 'U';
    return basic && clair_ts_in_bed(bed_start, bed_end, n_bed, pos);
}
// the four true indices of a window: the LAST truth row of its position (:125-126; truth_labels [n_truth][4], computed on the host by
// task.labels_from_vcf_columns), else homozygous reference of the centre base (:168-170: gt21 of base+base, genotype 0/0, both lengths 0)
CLAIR_TS_HD inline void clair_ts_label(const int64_t *truth, const uint8_t *truth_labels, int64_t n_truth, int64_t pos, uint8_t centre, uint8_t *out) {
    int64_t a = 0, b = n_truth;                                    // first index whose truth position is > pos
    while (a < b) { const int64_t mid = (a + b) >> 1; if (truth[mid] <= pos) a = mid + 1; else b = mid; }
    if (a > 0 && truth[a - 1] == pos) {
        for (int k = 0; k < 4; ++k) out[k] = truth_labels[(a - 1) * 4 + k];
        return;
    }
    const uint8_t homo[4] = {0, 4, 7, 9};                          // AA CC GG TT in the 21 genotype labels (task/gt21.py:3-50)
    const int base = clair_ts_acgt(centre);
    out[0] = homo[base < 0 ? 0 : base];
    out[1] = 0;
    out[2] = 16;
    out[3] = 16;
}

#endif /* CLAIR_TRAIN_SET_CORE_H */
