// Host-side helpers of the Clair hot path (include/clair_host.h): the training-set builder's three steps over arrays -- class and draw
// over a position list, pairing over window centres, the label join -- the twin of the device's (clair_amd/csrc/train_set.hip).  Plain
// C++17, no HIP.  The rules themselves are csrc/train_set_core.h, the code the kernels run; here they are applied in one sequential loop each.
#include "../../include/clair_host.h"
#include "../csrc/train_set_core.h"

#include <string.h>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

namespace {

bool bad_list(const int64_t *p, int64_t n) { return n < 0 || (n > 0 && !p); }
bool bad_bed(const int64_t *s, const int64_t *e, int64_t n) { return n > 0 && (!s || !e); }
bool unsorted(const int64_t *p, int64_t n) {
    for (int64_t i = 1; i < n; ++i) if (p[i] < p[i - 1]) return true;
    return false;
}

}  // namespace

extern "C" {

int clair_host_train_set_key(const char *ctg_name, int64_t seed, int stage, int64_t *key) {
    if (!ctg_name || !key || (stage != CLAIR_TS_STAGE_SAMPLE && stage != CLAIR_TS_STAGE_PAIR)) return clair_host_fail("train set key: bad arguments");
    *key = (int64_t)clair_ts_key((uint64_t)seed, clair_ts_fnv1a64(ctg_name, (int64_t)strlen(ctg_name)), (uint64_t)stage);
    return 0;
}

int clair_host_train_set_sample(const int64_t *positions, int64_t n, const int64_t *truth, int64_t n_truth, double p_near, double p_outside, int64_t key,
                                uint8_t *cls, uint64_t *draws, uint8_t *sampled, int64_t *n_near, int64_t *n_outside) {
    if (bad_list(positions, n) || bad_list(truth, n_truth)) return clair_host_fail("train set sample: bad arguments");
    if (unsorted(truth, n_truth)) return clair_host_fail("train set sample: truth positions not ascending");
    int64_t near = 0, outside = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int c = clair_ts_class(truth, n_truth, positions[i]);
        const uint64_t d = clair_ts_draw((uint64_t)key, positions[i]);
        const bool s = clair_ts_sampled(c, d, p_near, p_outside);
        if (cls) cls[i] = (uint8_t)c;
        if (draws) draws[i] = d;
        if (sampled) sampled[i] = s ? 1 : 0;
        if (s) ++(c == CLAIR_TS_NEAR ? near : outside);
    }
    if (n_near) *n_near = near;
    if (n_outside) *n_outside = outside;
    return 0;
}

int clair_host_train_set_pair_count(const int64_t *centres, int64_t n, const int64_t *truth, int64_t n_truth, const int64_t *bed_start, const int64_t *bed_end,
                                    int64_t n_bed, int64_t *v, int64_t *c) {
    if (bad_list(centres, n) || bad_list(truth, n_truth) || bad_bed(bed_start, bed_end, n_bed) || !v || !c) return clair_host_fail("train set pair: bad arguments");
    if (unsorted(truth, n_truth)) return clair_host_fail("train set pair: truth positions not ascending");
    int64_t nv = 0, nc = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (clair_ts_class(truth, n_truth, centres[i]) == CLAIR_TS_TRUTH) ++nv;
        else if (clair_ts_usable(truth, n_truth, bed_start, bed_end, n_bed, centres[i])) ++nc;
    }
    *v = nv;
    *c = nc;
    return 0;
}

int clair_host_train_set_ratio(int64_t v, double amp, int64_t c, double *r) {
    if (!r || v < 0 || c < 0) return clair_host_fail("train set ratio: bad arguments");
    *r = clair_ts_ratio(v, amp, c);
    return 0;
}

int clair_host_train_set_pair_keep(const int64_t *centres, int64_t n, const int64_t *truth, int64_t n_truth, const int64_t *bed_start, const int64_t *bed_end,
                                   int64_t n_bed, double r, int64_t key, int64_t *kept, int64_t *n_kept_var, int64_t *n_kept_non) {
    if (bad_list(centres, n) || bad_list(truth, n_truth) || bad_bed(bed_start, bed_end, n_bed) || (n > 0 && !kept) || !n_kept_var || !n_kept_non)
        return clair_host_fail("train set pair: bad arguments");
    if (unsorted(truth, n_truth)) return clair_host_fail("train set pair: truth positions not ascending");
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i)                                  // the variant windows first, in input order (PairWithNonVariants.py:61-68) ...
        if (clair_ts_class(truth, n_truth, centres[i]) == CLAIR_TS_TRUTH) kept[at++] = i;
    *n_kept_var = at;
    for (int64_t i = 0; i < n; ++i)                                  // ... then the usable non-variant windows that draw below r (:69-84)
        if (clair_ts_usable(truth, n_truth, bed_start, bed_end, n_bed, centres[i]) && clair_ts_paired(clair_ts_draw((uint64_t)key, centres[i]), r)) kept[at++] = i;
    *n_kept_non = at - *n_kept_var;
    return 0;
}

int clair_host_train_set_labels(const int64_t *centres, const uint8_t *centre_base, int64_t n, const int64_t *truth, const uint8_t *truth_labels, int64_t n_truth,
                                const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed, uint8_t *labels, uint8_t *in_set) {
    if (bad_list(centres, n) || (n > 0 && (!centre_base || !labels || !in_set)) || bad_list(truth, n_truth) || (n_truth > 0 && !truth_labels) ||
        bad_bed(bed_start, bed_end, n_bed))
        return clair_host_fail("train set labels: bad arguments");
    if (unsorted(truth, n_truth)) return clair_host_fail("train set labels: truth positions not ascending");
    for (int64_t i = 0; i < n; ++i) {
        clair_ts_label(truth, truth_labels, n_truth, centres[i], centre_base[i], labels + i * 4);
        in_set[i] = clair_ts_in_set(bed_start, bed_end, n_bed, centres[i], centre_base[i]) ? 1 : 0;
    }
    return 0;
}

}  // extern "C"
