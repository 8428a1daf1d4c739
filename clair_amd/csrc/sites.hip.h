// Ensemble across BAMs on the device: the site table.  Different BAMs yield different candidate sites, so the rows several (BAM, model)
// runs gave the same position have to be found before they can be averaged: what clair/post_processing/ensemble.py:10-75 does with a
// dict keyed by the text of (ctg, pos), over 3 KB of text per candidate and run.  Here the table lives in HBM, per site row:
//
//     key     int64           position within the contig
//     count   int32           the (BAM, model) runs that produced the site so far
//     acc     double [90]     the sum of their re-read probabilities (ensemble_core.h), in run order
//     x       float [1056]    the window of the FIRST run that had the site, as decode_kernel reads it from a slot
//     centre  2 bytes, seq 33 bytes: of that same run
//
// and an index of (key, row) sorted by key, double-buffered.  Rows are numbered in first-seen order, which is the order the text chain prints.
//
// BEGIN A SOURCE (once per BAM, all its positions, strictly ascending): sites_search_kernel looks every position up in the index (binary
// search) and flags those not found; sites_scan_kernel ranks the flags; sites_assign_kernel gives new site `rank` the row n_sites + rank,
// writes row_of[] for the whole source and merges the new keys into the other index buffer by rank -- a new key lands at its lower bound
// among the old keys plus its rank, an old key at its own place plus the new keys below it.  Row numbers therefore depend on the
// source alone, not on which lane runs which of its batches.
// ACCUMULATE (behind each forward pass of a batch of the source, on the slot's lane): sites_adopt_kernel copies window, centre and seq into
// the rows nobody has written yet (count == 0), sites_accumulate_kernel adds the re-read values into acc[row_of[first + i]], two values per
// thread as ensemble_kernel does, and bumps the count.  Sites are distinct within a source, batches are disjoint and sources follow one
// another: no atomics, and the order of every sum is the order of the runs.
// FINISH: flag count >= N in row order (chain) or in index order (position), scan, compact: the output list, the averaged float32 rows
// (clair_ens_finish with the site's own count as divisor) and the keys, counts and seqs in output order.
// DECODE: sites_gather_kernel puts windows, centre bytes and averaged rows of a range of the output list where a slot's decode_kernel and
// result copy read them.
//
// Shape.  Everything here is element-wise or a scan over at most a few million sites next to forward passes of 1.9 GFLOP per 1 024
// candidates: plain vector loads and stores, one workgroup for the scan (block_scan.hip.h, 256 items a step).
// Twin: clair_host_sites_* (hostsrc/host_sites.cpp), the same rule header compiled by the host compiler.
#pragma once
#include "common.hip.h"
#include "block_scan.hip.h"
#include "ensemble_core.h"

namespace clair {

constexpr int SITE_SEQ = 33;              // bytes of a reference window
constexpr int SITE_X = T_POS * F_IN;      // floats of a window
constexpr int SITE_MAX_ROWS = 64;         // CLAIR_SITES_MAX_ROWS: 8 BAMs x 8 checkpoints

static_assert(OUT_FLOATS % 2 == 0 && SITE_X % 4 == 0, "the site kernels take probabilities in pairs and windows in quads");

__device__ __forceinline__ int64_t sites_lower_bound(const int64_t *keys, int64_t n, int64_t key) {   // how many of keys[0 .. n) are < key
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// position i of the source: its lower bound in the index, whether it is new, and its row when it is not
__global__ __launch_bounds__(256) void sites_search_kernel(const int64_t *pos, int64_t n, const int64_t *idx_key, const int64_t *idx_row, int64_t n_sites,
                                                            int64_t *lb, uint32_t *is_new, int64_t *row_of) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t at = sites_lower_bound(idx_key, n_sites, pos[i]);
    const bool found = at < n_sites && idx_key[at] == pos[i];
    lb[i] = at;
    is_new[i] = found ? 0u : 1u;
    if (found) row_of[i] = idx_row[at];
}

// one workgroup walks n flags 256 at a time: before[i] = the flags set below i, before[n] = all of them
__global__ __launch_bounds__(256) void sites_scan_kernel(const uint32_t *flag, int64_t n, uint32_t *before) {
    uint32_t carry = 0, total;
    for (int64_t at = 0; at < n; at += 256) {
        const int64_t i = at + threadIdx.x;
        const uint32_t x = i < n ? flag[i] : 0u;
        const uint32_t ex = block_exclusive_scan(x, &total);
        if (i < n) before[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) before[n] = carry;
}

// threads [0, n): the new sites of the source take their rows and their places in the new index; threads [n, n + n_sites): the old index
// entries move up by the new keys below them
__global__ __launch_bounds__(256) void sites_assign_kernel(const int64_t *pos, int64_t n, const int64_t *lb, const uint32_t *is_new, const uint32_t *before,
                                                            const int64_t *idx_key, const int64_t *idx_row, int64_t n_sites, int64_t *new_key, int64_t *new_row,
                                                            int64_t *row_of, int64_t *key, int *count) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        if (!is_new[i]) return;
        const int64_t row = n_sites + before[i], at = lb[i] + before[i];
        row_of[i] = row;
        key[row] = pos[i];
        count[row] = 0;
        new_key[at] = pos[i];
        new_row[at] = row;
    } else if (i - n < n_sites) {
        const int64_t k = i - n;
        const int64_t at = k + before[sites_lower_bound(pos, n, idx_key[k])];
        new_key[at] = idx_key[k];
        new_row[at] = idx_row[k];
    }
}

struct SiteRows {           // the per-row arrays of the table
    int64_t *key;
    int *count;
    double *acc;            // [rows][90]
    float *x;               // [rows][1056]
    unsigned char *centre;  // [rows][2]
    unsigned char *seq;     // [rows][33]
};

// window, centre and seq of batch row r into its site row, where no run has written that row yet.  64 threads per batch row.
__global__ __launch_bounds__(256) void sites_adopt_kernel(SiteRows t, const int64_t *row_of, int n, const float *x, const unsigned char *centre,
                                                           const unsigned char *seq) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n) return;
    const int64_t row = row_of[r];
    if (t.count[row] != 0) return;
    if (x) {
        const f32x4 *src = (const f32x4 *)(x + (size_t)r * SITE_X);
        f32x4 *dst = (f32x4 *)(t.x + (size_t)row * SITE_X);
        for (int i = lane; i < SITE_X / 4; i += 64) dst[i] = src[i];
    }
    if (centre && lane < 2) t.centre[row * 2 + lane] = centre[r * 2 + lane];
    if (seq && lane < SITE_SEQ) t.seq[row * SITE_SEQ + lane] = seq[r * SITE_SEQ + lane];
}

// acc[row_of[r]] += reread(rows[r]), two values per thread; the thread that owns a row's first pair bumps its count.  A 65th run of a
// site raises *overflow instead (the table is refused from then on).
__global__ __launch_bounds__(256) void sites_accumulate_kernel(SiteRows t, const int64_t *row_of, int n_pairs, const float *rows, int *overflow) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pairs) return;
    constexpr int PAIRS = OUT_FLOATS / 2;
    const int r = i / PAIRS, j = i - r * PAIRS;
    const int64_t row = row_of[r];
    const float2 v = ((const float2 *)rows)[i];
    double2 *acc = (double2 *)(t.acc + (size_t)row * OUT_FLOATS) + j;
    double2 a = *acc;
    a.x = a.x + clair_ens_reread(v.x);
    a.y = a.y + clair_ens_reread(v.y);
    *acc = a;
    if (j == 0) {
        const int c = t.count[row];
        if (c >= SITE_MAX_ROWS) *overflow = 1; else t.count[row] = c + 1;
    }
}

// finish, step 1: entry i of the walk (row i for chain order, row idx_row[i] for position order) is kept when its count reaches min_count
__global__ __launch_bounds__(256) void sites_keep_kernel(const int *count, const int64_t *idx_row, int64_t n_sites, int min_count, uint32_t *keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sites) return;
    const int64_t row = idx_row ? idx_row[i] : i;
    keep[i] = count[row] >= min_count ? 1u : 0u;
}

// finish, step 2 (after the scan): the output list and the keys, counts and seqs in output order
__global__ __launch_bounds__(256) void sites_compact_kernel(SiteRows t, const int64_t *idx_row, int64_t n_sites, const uint32_t *keep, const uint32_t *before,
                                                             int64_t *out_row, int64_t *out_key, int *out_count, unsigned char *out_seq) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_sites || !keep[i]) return;
    const int64_t row = idx_row ? idx_row[i] : i, o = before[i];
    out_row[o] = row;
    out_key[o] = t.key[row];
    out_count[o] = t.count[row];
    for (int k = 0; k < SITE_SEQ; ++k) out_seq[o * SITE_SEQ + k] = t.seq[row * SITE_SEQ + k];
}

// finish, step 3: the averaged rows, float32 [n_out][90]
__global__ __launch_bounds__(256) void sites_average_kernel(SiteRows t, const int64_t *out_row, int64_t n_values, float *avg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_values) return;
    const int64_t o = i / OUT_FLOATS;
    const int j = (int)(i - o * OUT_FLOATS);
    const int64_t row = out_row[o];
    avg[i] = clair_ens_finish(t.acc[(size_t)row * OUT_FLOATS + j], t.count[row]);
}

// entries [first, first + n) of the output list -> a slot: windows, centre bytes, averaged rows.  64 threads per entry.
__global__ __launch_bounds__(256) void sites_gather_kernel(SiteRows t, const int64_t *out_row, const float *avg, int64_t first, int n, float *x, unsigned char *centre,
                                                            float *rows) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= n) return;
    const int64_t row = out_row[first + r];
    if (x) {
        const f32x4 *src = (const f32x4 *)(t.x + (size_t)row * SITE_X);
        f32x4 *dst = (f32x4 *)(x + (size_t)r * SITE_X);
        for (int i = lane; i < SITE_X / 4; i += 64) dst[i] = src[i];
    }
    if (centre && lane < 2) centre[r * 2 + lane] = t.centre[row * 2 + lane];
    if (rows) {
        const float *src = avg + (size_t)(first + r) * OUT_FLOATS;
        for (int i = lane; i < OUT_FLOATS; i += 64) rows[(size_t)r * OUT_FLOATS + i] = src[i];
    }
}

}  // namespace clair
