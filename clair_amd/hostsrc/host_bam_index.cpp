// index_bam on the CPU (include/clair_host.h: clair_host_bamidx_*; docs/index_bam.md).  Three things:
//   - the host twin of csrc/bam_index.hip: the same batch interface and the rules of csrc/bam_index_core.h as sequential loops.  Blocks are
//     inflated by zlib on a few threads (hostsrc/bgzf_file.h); records are framed by the plain walk, or by the restatement of the segmented
//     framing the device runs (hostsrc/bam_frame.h, shared with host_bam_sort.cpp);
//   - the file driver both backends run under: the input as a job and its batches of max_blocks blocks (hostsrc/bam_job.h), the runs joined
//     across batches;
//   - the result the Python side writes the .bai from (clair_amd/index_bam.py).
// Plain C++17 + zlib, no HIP.
#include "../../include/clair_host.h"
#include "../csrc/bam_index_core.h"
#include "bam_frame.h"
#include "bam_job.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

using namespace clair_bix;
using namespace clair_bgzf;
using namespace clair_frame;

}  // namespace

struct clair_host_bamidx {
    clair_frame::HostFront front;                // the batch: the stream, the record starts, the carry
    int n_ref = -1;
    std::vector<int64_t> first_window;           // n_ref + 1
    std::vector<uint64_t> linear;
    int64_t counts[3] = {0, 0, 0};
    std::vector<clair_bamidx_run_t> runs;
};

struct clair_host_bamidx_result {
    int64_t counts[3] = {0, 0, 0};
    std::vector<int64_t> first_window;
    std::vector<uint64_t> linear;
    std::vector<clair_bamidx_run_t> runs;
};

extern "C" {

int clair_host_bamidx_create(int threads, int max_blocks, int segment_bytes, clair_host_bamidx_t **out) {
    if (!out) return clair_host_fail("out is NULL");
    *out = nullptr;
    clair_host_bamidx *h = new clair_host_bamidx;
    if (h->front.configure(threads, max_blocks, segment_bytes)) { delete h; return 1; }
    *out = h;
    return 0;
}

void clair_host_bamidx_destroy(clair_host_bamidx_t *h) { delete h; }

int clair_host_bamidx_begin(clair_host_bamidx_t *h, int n_ref, const int64_t *ref_len) {
    if (!h || n_ref < 0 || (n_ref > 0 && !ref_len)) return clair_host_fail("bamidx begin: bad arguments");
    h->first_window.assign((size_t)n_ref + 1, 0);
    for (int r = 0; r < n_ref; ++r) h->first_window[(size_t)r + 1] = h->first_window[(size_t)r] + windows_of(ref_len[r]);
    h->linear.assign((size_t)h->first_window[(size_t)n_ref], NO_OFFSET);
    h->n_ref = n_ref;
    h->counts[0] = h->counts[1] = h->counts[2] = 0;
    h->front.rewind();
    return 0;
}

int clair_host_bamidx_batch(clair_host_bamidx_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                            const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state,
                            const clair_bamidx_run_t **runs) {
    if (!h || !state || !runs) return clair_host_fail("bamidx batch: NULL argument");
    if (h->n_ref < 0) return clair_host_fail("bamidx batch: begin first");
    // 1, 2. the stream and the record starts (bam_frame.h)
    HostFront &front = h->front;
    if (front.open_batch("bamidx batch", cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    const Bytes m{front.stream.data()};
    const int64_t n_rec = (int64_t)front.starts.size(), tail = front.tail;
    const auto voffset = [&](int64_t p) { return front.voffset(p); };
    // 3 - 5. fields, runs, the linear index
    h->runs.clear();
    int32_t prev_tid = (int32_t)state[ST_PREV_TID], prev_pos = (int32_t)state[ST_PREV_POS];
    for (int64_t k = 0; k < n_rec; ++k) {
        const int64_t o = front.starts[(size_t)k];
        Fields f = fields(m, o, h->n_ref);
        if (f.verdict == V_OK && order_key(f.tid, f.pos) < order_key(prev_tid, prev_pos)) f.verdict = V_UNSORTED;
        if (f.verdict != V_OK) {
            const Detail d{state[ST_RECORDS_BEFORE] + k, f.tid, f.pos, prev_tid, prev_pos, f.end, voffset(o), m.le32(o), f.verdict};
            char buf[400];
            describe(buf, sizeof buf, d);
            return clair_host_fail("%s", buf);
        }
        const uint64_t beg = voffset(o), end = voffset(k + 1 < n_rec ? front.starts[(size_t)k + 1] : tail);
        h->counts[0] += 1;
        if (f.tid < 0) h->counts[2] += 1;
        else if (!(f.flag & 4)) h->counts[1] += 1;
        if (f.tid >= 0) {
            const int64_t n_win = h->first_window[(size_t)f.tid + 1] - h->first_window[(size_t)f.tid];
            for (int64_t w = (f.pos > 0 ? f.pos : 0) >> WINDOW_SHIFT; w <= (f.end - 1) >> WINDOW_SHIFT && w < n_win; ++w) {
                uint64_t &slot = h->linear[(size_t)(h->first_window[(size_t)f.tid] + w)];
                slot = std::min(slot, beg);
            }
        }
        if (h->runs.empty() || k == 0 || h->runs.back().tid != f.tid || h->runs.back().bin != f.bin) h->runs.push_back(clair_bamidx_run_t{f.tid, f.bin, beg, end});
        else h->runs.back().end = end;
        prev_tid = f.tid;
        prev_pos = f.pos;
    }
    if (front.close_batch(last)) return 1;
    state[ST_N_RECORDS] = n_rec;
    state[ST_N_RUNS] = (int64_t)h->runs.size();
    state[ST_LAST_TID] = prev_tid;
    state[ST_LAST_POS] = prev_pos;
    state[ST_CARRY] = (int64_t)front.carry.size();
    *runs = h->runs.data();
    return 0;
}

int clair_host_bamidx_finish(clair_host_bamidx_t *h, uint64_t *linear, int64_t n_windows, int64_t *counts) {
    if (!h || !counts || h->n_ref < 0) return clair_host_fail("bamidx finish: bad arguments");
    if (n_windows != (int64_t)h->linear.size() || (n_windows > 0 && !linear)) return clair_host_fail("bamidx finish: %lld windows, the handle has %zu", (long long)n_windows, h->linear.size());
    if (n_windows) memcpy(linear, h->linear.data(), (size_t)n_windows * 8);
    for (int i = 0; i < 3; ++i) counts[i] = h->counts[i];
    return 0;
}

static int twin_begin(void *ctx, int n_ref, const int64_t *ref_len) { return clair_host_bamidx_begin((clair_host_bamidx_t *)ctx, n_ref, ref_len); }
static int twin_batch(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                      const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state, const clair_bamidx_run_t **runs) {
    return clair_host_bamidx_batch((clair_host_bamidx_t *)ctx, cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry, last, state, runs);
}
static int twin_finish(void *ctx, uint64_t *linear, int64_t n_windows, int64_t *counts) { return clair_host_bamidx_finish((clair_host_bamidx_t *)ctx, linear, n_windows, counts); }
static const char *twin_last_error(const void *) { return clair_host_last_error(); }

int clair_host_bamidx_backend(clair_host_bamidx_t *h, clair_bamidx_backend_t *out) {
    if (!h || !out) return clair_host_fail("bamidx backend: NULL argument");
    *out = clair_bamidx_backend_t{h, twin_begin, twin_batch, twin_finish, twin_last_error};
    return 0;
}

int clair_host_bamidx_debug_frame(const uint8_t *stream, int64_t n, int64_t entry, int segment_bytes, int64_t *starts, int64_t cap, int64_t *result) {
    if (n < 0 || (n > 0 && !stream) || entry < 0 || entry > n || cap < 0 || (cap > 0 && !starts) || !result) return clair_host_fail("debug_frame: bad arguments");
    if (segment_bytes != 0 && !good_segment(segment_bytes)) return clair_host_fail("segment_bytes %d: a power of two in %u .. %u, or 0", segment_bytes, SEG_MIN, SEG_MAX);
    std::vector<int64_t> found;
    int64_t tail = 0;
    bool bad = false;
    if (segment_bytes) frame_segmented(Bytes{stream}, n, entry, (uint32_t)segment_bytes, found, &tail, &bad);
    else frame_walk(Bytes{stream}, n, entry, found, &tail, &bad);
    if ((int64_t)found.size() > cap) return clair_host_fail("debug_frame: %zu records, room for %lld", found.size(), (long long)cap);
    std::copy(found.begin(), found.end(), starts);
    result[FR_N_STARTS] = (int64_t)found.size();
    result[FR_TAIL] = tail;
    result[FR_BAD] = bad ? 1 : 0;
    result[FR_SENTINELS] = 1;
    return 0;
}

// ---- the file driver
int clair_host_bamidx_build(const char *path, const clair_bamidx_backend_t *be, int max_blocks, clair_host_bamidx_result_t **out) {
    if (!out) return clair_host_fail("out is NULL");
    *out = nullptr;
    if (!path || !be || !be->begin || !be->batch || !be->finish || !be->last_error) return clair_host_fail("bamidx build: NULL argument");
    if (check_max_blocks(max_blocks)) return 1;
    clair_job::Job job;
    if (clair_job::open_job(path, "(SAM text, CRAM and plain gzip have no .bai)", &job)) return 1;
    const int32_t n_ref = (int32_t)job.header.lengths.size();
    const std::vector<int64_t> &ref_len = job.header.lengths;
    if (be->begin(be->ctx, n_ref, ref_len.data())) return clair_host_fail("%s: %s", path, be->last_error(be->ctx));
    clair_host_bamidx_result *res = new clair_host_bamidx_result;
    struct Guard { clair_host_bamidx_result *r; ~Guard() { delete r; } } guard{res};
    int64_t state[STATE_WORDS] = {0, 0, INT32_MIN, 0, 0, 0, INT32_MIN, 0};
    clair_job::Batches in(&job, max_blocks);
    while (!in.last) {
        if (in.next()) return 1;
        const clair_bamidx_run_t *runs = nullptr;
        if (in.through(be->batch, be->ctx, state, &runs)) return clair_host_fail("%s: %s", path, be->last_error(be->ctx));
        for (int64_t k = 0; k < state[ST_N_RUNS]; ++k) {
            const clair_bamidx_run_t &r = runs[k];
            if (r.tid < 0) continue;
            if (k == 0 && !res->runs.empty() && res->runs.back().tid == r.tid && res->runs.back().bin == r.bin && res->runs.back().end == r.beg) res->runs.back().end = r.end;
            else res->runs.push_back(r);
        }
        state[ST_RECORDS_BEFORE] += state[ST_N_RECORDS];
        state[ST_PREV_TID] = state[ST_LAST_TID];
        state[ST_PREV_POS] = state[ST_LAST_POS];
    }
    res->first_window.assign((size_t)n_ref + 1, 0);
    for (int r = 0; r < n_ref; ++r) res->first_window[(size_t)r + 1] = res->first_window[(size_t)r] + windows_of(ref_len[(size_t)r]);
    res->linear.assign((size_t)res->first_window[(size_t)n_ref], NO_OFFSET);
    if (be->finish(be->ctx, res->linear.data(), (int64_t)res->linear.size(), res->counts)) return clair_host_fail("%s: %s", path, be->last_error(be->ctx));
    guard.r = nullptr;
    *out = res;
    return 0;
}

int clair_host_bamidx_result_info(const clair_host_bamidx_result_t *r, int64_t *info) {
    if (!r || !info) return clair_host_fail("NULL argument");
    info[0] = (int64_t)r->first_window.size() - 1;
    info[1] = r->counts[0];
    info[2] = r->counts[1];
    info[3] = r->counts[2];
    info[4] = (int64_t)r->runs.size();
    info[5] = (int64_t)r->linear.size();
    return 0;
}

int clair_host_bamidx_result_copy(const clair_host_bamidx_result_t *r, clair_bamidx_run_t *runs, uint64_t *linear, int64_t *first_window) {
    if (!r) return clair_host_fail("NULL argument");
    if (runs && !r->runs.empty()) memcpy(runs, r->runs.data(), r->runs.size() * sizeof(clair_bamidx_run_t));
    if (linear && !r->linear.empty()) memcpy(linear, r->linear.data(), r->linear.size() * 8);
    if (first_window) memcpy(first_window, r->first_window.data(), r->first_window.size() * 8);
    return 0;
}

void clair_host_bamidx_result_free(clair_host_bamidx_result_t *r) { delete r; }

}  // extern "C"
