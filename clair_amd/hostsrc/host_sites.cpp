// Host-side helpers of the Clair hot path (include/clair_host.h): the site table of ensemble calling across BAMs, the twin of the device's
// (clair_amd/csrc/sites.hip.h).  Plain C++17, no HIP.  Same semantics step for step -- a sorted index searched per position, new sites
// numbered in first-seen order, sums in run order in double, the site's own count as divisor -- and the same rule header
// (csrc/ensemble_core.h), so that both give the same bits; what it is measured against in tests is the text filter it restates
// (clair_amd/ensemble.py, clair/post_processing/ensemble.py:10-75).
#include "../../include/clair_host.h"
#include "../csrc/ensemble_core.h"

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

namespace {
constexpr int OUT = 90, X = 1056, SEQ = 33, MAX_ROWS = 64;
}

struct clair_host_sites {
    std::vector<int64_t> key;
    std::vector<int> count;
    std::vector<double> acc;            // [rows][90]
    std::vector<float> x;               // [rows][1056]
    std::vector<uint8_t> centre, seq;   // [rows][2], [rows][33]
    std::vector<std::pair<int64_t, int64_t>> index;   // (key, row) sorted by key
    std::vector<int64_t> row_of;        // of the current source
    bool has_source = false, finished = false;
    std::vector<int64_t> out_row;
};

extern "C" {

int clair_host_sites_create(clair_host_sites_t **out) {
    if (!out) return clair_host_fail("site table: out is NULL");
    *out = new clair_host_sites();
    return 0;
}

void clair_host_sites_destroy(clair_host_sites_t *t) { delete t; }

int clair_host_sites_begin_source(clair_host_sites_t *t, const int64_t *positions, int64_t n, int64_t *n_new) {
    if (!t) return clair_host_fail("site table: the table is NULL");
    if (t->finished) return clair_host_fail("site table: the table has been finished: it takes no more rows");
    if (n < 0 || (n > 0 && !positions)) return clair_host_fail("site table: bad arguments");
    for (int64_t i = 1; i < n; ++i)
        if (positions[i] <= positions[i - 1])
            return clair_host_fail("site table: positions are not strictly ascending (%lld after %lld at %lld)", (long long)positions[i], (long long)positions[i - 1], (long long)i);
    const size_t old = t->key.size();
    t->row_of.assign((size_t)n, 0);
    std::vector<std::pair<int64_t, int64_t>> fresh;
    for (int64_t i = 0; i < n; ++i) {
        auto at = std::lower_bound(t->index.begin(), t->index.end(), std::make_pair(positions[i], (int64_t)-1));
        if (at != t->index.end() && at->first == positions[i]) { t->row_of[(size_t)i] = at->second; continue; }
        const int64_t row = (int64_t)(old + fresh.size());
        t->row_of[(size_t)i] = row;
        fresh.emplace_back(positions[i], row);
    }
    const size_t rows = old + fresh.size();
    for (const auto &f : fresh) t->key.push_back(f.first);
    t->count.resize(rows, 0);
    t->acc.resize(rows * OUT, 0.0);
    t->x.resize(rows * X, 0.f);
    t->centre.resize(rows * 2, 0);
    t->seq.resize(rows * SEQ, 0);
    std::vector<std::pair<int64_t, int64_t>> merged(rows);
    std::merge(t->index.begin(), t->index.end(), fresh.begin(), fresh.end(), merged.begin());
    t->index.swap(merged);
    t->has_source = true;
    if (n_new) *n_new = (int64_t)fresh.size();
    return 0;
}

int clair_host_sites_add_rows(clair_host_sites_t *t, int64_t first, const float *probs, int64_t n, const float *x, const uint8_t *centre, const uint8_t *seq) {
    if (!t) return clair_host_fail("site table: the table is NULL");
    if (t->finished) return clair_host_fail("site table: the table has been finished: it takes no more rows");
    if (!probs) return clair_host_fail("site table: NULL input pointer");
    if (!t->has_source) return clair_host_fail("site table: no source begun: call clair_host_sites_begin_source first");
    const int64_t src_n = (int64_t)t->row_of.size();
    if (first < 0 || n < 1 || first > src_n - n)
        return clair_host_fail("site table: rows [%lld, %lld) lie outside the current source of %lld", (long long)first, (long long)(first + n), (long long)src_n);
    for (int64_t i = 0; i < n; ++i)
        if (t->count[(size_t)t->row_of[(size_t)(first + i)]] >= MAX_ROWS) return clair_host_fail("site table: a site was given more than %d rows", MAX_ROWS);
    for (int64_t i = 0; i < n; ++i) {
        const size_t row = (size_t)t->row_of[(size_t)(first + i)];
        if (t->count[row] == 0) {     // nobody has written this site yet: window, centre and seq are this run's
            if (x) memcpy(&t->x[row * X], x + (size_t)i * X, X * sizeof(float));
            if (centre) memcpy(&t->centre[row * 2], centre + (size_t)i * 2, 2); else memset(&t->centre[row * 2], 0, 2);
            if (seq) memcpy(&t->seq[row * SEQ], seq + (size_t)i * SEQ, SEQ); else memset(&t->seq[row * SEQ], 0, SEQ);
        }
        double *a = &t->acc[row * OUT];
        for (int j = 0; j < OUT; ++j) a[j] = a[j] + clair_ens_reread(probs[(size_t)i * OUT + j]);
        t->count[row] += 1;
    }
    return 0;
}

int clair_host_sites_finish(clair_host_sites_t *t, int min_count, int order, int64_t *n_out) {
    if (!t) return clair_host_fail("site table: the table is NULL");
    if (order != 0 && order != 1) return clair_host_fail("site table: order %d is neither chain (0) nor position (1)", order);
    const int need = std::max(min_count, 1);     // a row begun but never fed is no site
    t->out_row.clear();
    for (size_t i = 0; i < t->key.size(); ++i) {
        const int64_t row = order == 1 ? t->index[i].second : (int64_t)i;
        if (t->count[(size_t)row] >= need) t->out_row.push_back(row);
    }
    t->finished = true;
    if (n_out) *n_out = (int64_t)t->out_row.size();
    return 0;
}

static int check_out(clair_host_sites_t *t, int64_t first, int64_t n) {
    if (!t) return clair_host_fail("site table: the table is NULL");
    if (!t->finished) return clair_host_fail("site table: call clair_host_sites_finish first");
    const int64_t n_out = (int64_t)t->out_row.size();
    if (first < 0 || n < 0 || first > n_out - n)
        return clair_host_fail("site table: rows [%lld, %lld) lie outside the output list of %lld", (long long)first, (long long)(first + n), (long long)n_out);
    return 0;
}

int clair_host_sites_info(clair_host_sites_t *t, int64_t first, int64_t n, int64_t *positions, int32_t *counts, uint8_t *seq) {
    if (check_out(t, first, n)) return 1;
    for (int64_t i = 0; i < n; ++i) {
        const size_t row = (size_t)t->out_row[(size_t)(first + i)];
        if (positions) positions[i] = t->key[row];
        if (counts) counts[i] = t->count[row];
        if (seq) memcpy(seq + (size_t)i * SEQ, &t->seq[row * SEQ], SEQ);
    }
    return 0;
}

int clair_host_sites_rows(clair_host_sites_t *t, int64_t first, int64_t n, float *out) {
    if (check_out(t, first, n)) return 1;
    if (n > 0 && !out) return clair_host_fail("site table: out is NULL");
    for (int64_t i = 0; i < n; ++i) {
        const size_t row = (size_t)t->out_row[(size_t)(first + i)];
        for (int j = 0; j < OUT; ++j) out[(size_t)i * OUT + j] = clair_ens_finish(t->acc[row * OUT + j], t->count[row]);
    }
    return 0;
}

int clair_host_sites_windows(clair_host_sites_t *t, int64_t first, int64_t n, float *x) {
    if (check_out(t, first, n)) return 1;
    if (n > 0 && !x) return clair_host_fail("site table: x is NULL");
    for (int64_t i = 0; i < n; ++i) {
        const size_t row = (size_t)t->out_row[(size_t)(first + i)];
        if (x) memcpy(x + (size_t)i * X, &t->x[row * X], X * sizeof(float));
    }
    return 0;
}

}  // extern "C"
