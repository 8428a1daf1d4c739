// sort_bam on the CPU (include/clair_host.h: clair_host_bamsort_*; docs/sort_bam.md).  Two things:
//   - the host twin of csrc/bam_sort.hip: the same calls and the rules of csrc/bam_sort_core.h as sequential loops.  Blocks are inflated by
//     zlib on a few threads (hostsrc/bgzf_file.h), records framed as host_bam_index.cpp frames them (hostsrc/bam_frame.h), kept records
//     compacted into the group buffer, the group ordered by std::stable_sort over (key, index), gathered, cut every 65280 bytes and
//     compressed by the host twin of the device compressor (host_deflate.cpp);
//   - the file driver both backends run under (the job, its batches and the output's writer are hostsrc/bam_job.h): the first read with the
//     byte histogram, the groups of buckets when the file does not fit, one more read per group, the blocks appended to the output, the EOF
//     marker.
// Plain C++17 + zlib, no HIP.
#include "../../include/clair_host.h"
#include "../csrc/bam_sort_core.h"
#include "bam_frame.h"
#include "bam_job.h"

#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

namespace {

using namespace clair_bsort;
using namespace clair_bgzf;
using namespace clair_frame;
}  // namespace

struct clair_host_bamsort {
    clair_frame::HostFront front;                // the batch: the stream, the record starts, the carry
    // the file
    int n_ref = -1;
    int64_t memory = 0;
    std::vector<int64_t> ref_len, first_bucket;  // n_ref; n_ref + 1
    std::vector<int64_t> hist;
    // the read in progress
    int64_t lo = 0, hi = 0;
    bool first = false, overflow = false;
    // the group
    std::vector<uint8_t> group;
    std::vector<uint64_t> keys;
    std::vector<int64_t> off;                    // of each kept record in the group buffer, one more for its end
    clair_job::OutStream out;                    // the sorted records
};

extern "C" {

int clair_host_bamsort_create(int threads, int max_blocks, int segment_bytes, clair_host_bamsort_t **out) {
    if (!out) return clair_host_fail("out is NULL");
    *out = nullptr;
    clair_host_bamsort *h = new clair_host_bamsort;
    if (h->front.configure(threads, max_blocks, segment_bytes)) { delete h; return 1; }
    *out = h;
    return 0;
}

void clair_host_bamsort_destroy(clair_host_bamsort_t *h) { delete h; }

int clair_host_bamsort_begin(clair_host_bamsort_t *h, int n_ref, const int64_t *ref_len, int64_t memory) {
    if (!h || n_ref < 0 || (n_ref > 0 && !ref_len)) return clair_host_fail("bamsort begin: bad arguments");
    if (memory < 1) return clair_host_fail("bamsort begin: memory %lld", (long long)memory);
    h->ref_len.assign(ref_len, ref_len + n_ref);
    h->first_bucket.assign((size_t)n_ref + 1, 0);
    for (int r = 0; r < n_ref; ++r) h->first_bucket[(size_t)r + 1] = h->first_bucket[(size_t)r] + buckets_of(ref_len[r]);
    h->hist.assign((size_t)h->first_bucket[(size_t)n_ref] + 1, 0);
    h->memory = memory;
    h->n_ref = n_ref;
    h->out.rewind();
    h->lo = h->hi = 0;
    return 0;
}

int clair_host_bamsort_pass(clair_host_bamsort_t *h, int64_t bucket_lo, int64_t bucket_hi, int first) {
    if (!h || h->n_ref < 0) return clair_host_fail("bamsort pass: begin first");
    if (bucket_lo < 0 || bucket_hi < bucket_lo || bucket_hi > (int64_t)h->hist.size()) return clair_host_fail("bamsort pass: buckets [%lld, %lld) of %zu", (long long)bucket_lo, (long long)bucket_hi, h->hist.size());
    h->lo = bucket_lo;
    h->hi = bucket_hi;
    h->first = first != 0;
    h->overflow = false;
    h->front.rewind();
    h->group.clear();
    h->keys.clear();
    h->off.assign(1, 0);
    if (h->first) std::fill(h->hist.begin(), h->hist.end(), 0);
    return 0;
}

int clair_host_bamsort_batch(clair_host_bamsort_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                             const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state) {
    if (!h || !state) return clair_host_fail("bamsort batch: NULL argument");
    if (h->n_ref < 0 || h->off.empty()) return clair_host_fail("bamsort batch: begin and pass first");
    // 1, 2. the stream and the record starts (bam_frame.h)
    HostFront &front = h->front;
    if (front.open_batch("bamsort batch", cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    const Bytes m{front.stream.data()};
    const int64_t n_rec = (int64_t)front.starts.size();
    const auto voffset = [&](int64_t p) { return front.voffset(p); };
    // 3. keys, the histogram, the order, the records of this group
    uint64_t prev = (uint64_t)state[SS_PREV_KEY];
    int64_t kept = 0, kept_bytes = 0, mapped = 0, unplaced = 0, unsorted = 0;
    for (int64_t k = 0; k < n_rec; ++k) {
        const int64_t o = front.starts[(size_t)k];
        const Fields f = fields(m, o, h->n_ref);
        if (sort_verdict(f.verdict) != V_OK) {
            const Detail d{state[SS_RECORDS_BEFORE] + k, f.tid, f.pos, 0, 0, f.end, voffset(o), m.le32(o), f.verdict};
            char buf[400];
            describe(buf, sizeof buf, d);
            return clair_host_fail("%s", buf);
        }
        const uint64_t key = sort_key(f.tid, f.pos, f.flag);
        const int64_t size = 4 + (int64_t)m.le32(o), bucket = bucket_of(f.tid, f.pos, h->n_ref, h->first_bucket.data(), h->ref_len.data());
        if (key < prev) unsorted = 1;
        prev = key;
        if (f.tid < 0) ++unplaced;
        else if (!(f.flag & 4)) ++mapped;
        if (h->first) h->hist[(size_t)bucket] += size;
        if (bucket < h->lo || bucket >= h->hi || h->overflow) continue;
        if ((int64_t)h->group.size() + size > h->memory) {
            if (!h->first) return clair_host_fail("bamsort batch: the group outgrows the %lld bytes the histogram gave it", (long long)h->memory);
            h->overflow = true;                  // the file does not fit: what was compacted is dropped, the read goes on for the histogram
            h->group.clear();
            h->keys.clear();
            h->off.assign(1, 0);
            continue;
        }
        if ((int64_t)h->keys.size() >= MAX_GROUP_RECORDS) return clair_host_fail("more than 2^31 - 1 records in one group: a smaller --memory makes smaller groups");
        h->group.insert(h->group.end(), front.stream.begin() + (ptrdiff_t)o, front.stream.begin() + (ptrdiff_t)(o + size));
        h->keys.push_back(key);
        h->off.push_back((int64_t)h->group.size());
        ++kept;
        kept_bytes += size;
    }
    if (front.close_batch(last)) return 1;
    state[SS_N_RECORDS] = n_rec;
    state[SS_LAST_KEY] = (int64_t)prev;
    state[SS_KEPT] = h->overflow ? 0 : kept;
    state[SS_KEPT_BYTES] = h->overflow ? 0 : kept_bytes;
    state[SS_UNSORTED] = unsorted;
    state[SS_OVERFLOW] = h->overflow ? 1 : 0;
    state[SS_MAPPED] = mapped;
    state[SS_UNPLACED] = unplaced;
    state[SS_CARRY] = (int64_t)front.carry.size();
    return 0;
}

int clair_host_bamsort_histogram(clair_host_bamsort_t *h, int64_t *bytes, int64_t n_buckets) {
    if (!h || !bytes || h->n_ref < 0) return clair_host_fail("bamsort histogram: bad arguments");
    if (n_buckets != (int64_t)h->hist.size()) return clair_host_fail("bamsort histogram: %lld buckets, the handle has %zu", (long long)n_buckets, h->hist.size());
    memcpy(bytes, h->hist.data(), h->hist.size() * 8);
    return 0;
}

int clair_host_bamsort_sort(clair_host_bamsort_t *h, int last, int64_t *info) {
    if (!h || !info || h->n_ref < 0 || h->off.empty()) return clair_host_fail("bamsort sort: bad arguments");
    const size_t n = h->keys.size();
    std::vector<uint32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return h->keys[a] < h->keys[b]; });
    std::vector<uint8_t> &sorted = h->out.bytes;
    h->out.begin();
    sorted.reserve(sorted.size() + h->group.size());
    for (size_t i = 0; i < n; ++i) sorted.insert(sorted.end(), h->group.begin() + (ptrdiff_t)h->off[perm[i]], h->group.begin() + (ptrdiff_t)h->off[(size_t)perm[i] + 1]);
    const int64_t payloads = h->out.cut(last != 0);
    h->group.clear();
    h->keys.clear();
    h->off.clear();                              // a new pass before the next batch
    info[SI_BYTES] = h->out.total;
    info[SI_PAYLOADS] = payloads;
    info[SI_RECORDS] = (int64_t)n;
    info[SI_PASSES] = 0;
    return 0;
}

int clair_host_bamsort_emit(clair_host_bamsort_t *h, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) {
    if (!h) return clair_host_fail("bamsort emit: bad arguments");
    return clair_job::emit_payloads(h->out.bytes.data(), h->out.total, h->front.threads, first, n, compressed, out, sizes, "bamsort");
}

static int twin_begin(void *ctx, int n_ref, const int64_t *ref_len, int64_t memory) { return clair_host_bamsort_begin((clair_host_bamsort_t *)ctx, n_ref, ref_len, memory); }
static int twin_pass(void *ctx, int64_t lo, int64_t hi, int first) { return clair_host_bamsort_pass((clair_host_bamsort_t *)ctx, lo, hi, first); }
static int twin_batch(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                      const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state) {
    return clair_host_bamsort_batch((clair_host_bamsort_t *)ctx, cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry, last, state);
}
static int twin_histogram(void *ctx, int64_t *bytes, int64_t n_buckets) { return clair_host_bamsort_histogram((clair_host_bamsort_t *)ctx, bytes, n_buckets); }
static int twin_sort(void *ctx, int last, int64_t *info) { return clair_host_bamsort_sort((clair_host_bamsort_t *)ctx, last, info); }
static int twin_emit(void *ctx, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) { return clair_host_bamsort_emit((clair_host_bamsort_t *)ctx, first, n, compressed, out, sizes); }
static const char *twin_last_error(const void *) { return clair_host_last_error(); }

int clair_host_bamsort_backend(clair_host_bamsort_t *h, clair_bamsort_backend_t *out) {
    if (!h || !out) return clair_host_fail("bamsort backend: NULL argument");
    *out = clair_bamsort_backend_t{h, twin_begin, twin_pass, twin_batch, twin_histogram, twin_sort, twin_emit, twin_last_error};
    return 0;
}

int clair_host_bamsort_debug_sort(const uint64_t *keys, int64_t n, uint32_t *perm) {
    if (n < 0 || n > MAX_GROUP_RECORDS || (n > 0 && (!keys || !perm))) return clair_host_fail("debug_sort: bad arguments");
    std::iota(perm, perm + n, 0u);
    std::stable_sort(perm, perm + n, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    return 0;
}

int clair_host_bamsort_debug_gather(const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, const uint32_t *perm, int64_t n, uint8_t *out, int64_t out_bytes) {
    if (n < 0 || stream_bytes < 0 || out_bytes < 0 || (n > 0 && (!stream || !starts || !perm || !out))) return clair_host_fail("debug_gather: bad arguments");
    int64_t at = 0;
    for (int64_t i = 0; i < n; ++i) {
        if ((int64_t)perm[i] >= n) return clair_host_fail("debug_gather: perm[%lld] = %u of %lld", (long long)i, perm[i], (long long)n);
        const int64_t o = starts[perm[i]];
        int64_t next = 0;
        if (o < 0 || step(Bytes{stream}, o, stream_bytes, &next) != STEP_NEXT) return clair_host_fail("debug_gather: no record at %lld", (long long)o);
        if (at + (next - o) > out_bytes) return clair_host_fail("debug_gather: the records need more than %lld bytes", (long long)out_bytes);
        memcpy(out + at, stream + o, (size_t)(next - o));
        at += next - o;
    }
    if (at != out_bytes) return clair_host_fail("debug_gather: %lld bytes gathered, %lld expected", (long long)at, (long long)out_bytes);
    return 0;
}

// ---- the file driver
// deflate: 0 the backend's own compressor, 1 zlib, 2 the host twin of the device compressor on `threads` threads.
// stats [CLAIR_BAMSORT_STATS] = records, mapped, unplaced, groups, input reads, already sorted, bytes appended to out_path
int clair_host_bamsort_run(clair_host_bam_job_t *job, const clair_bamsort_backend_t *be, const char *out_path, int deflate, int64_t memory, int max_blocks,
                           int threads, int64_t *stats) {
    if (!job || !be || !out_path || !stats || !be->begin || !be->pass || !be->batch || !be->histogram || !be->sort || !be->emit || !be->last_error)
        return clair_host_fail("bamsort run: NULL argument");
    if (check_max_blocks(max_blocks)) return 1;
    if (deflate < 0 || deflate > 2 || threads < 1 || threads > 16 || memory < 1) return clair_host_fail("bamsort run: bad arguments");
    const char *path = job->path.c_str();
    const auto failed = [&] { return clair_host_fail("%s: %s", path, be->last_error(be->ctx)); };
    const int n_ref = (int)job->header.lengths.size();
    const std::vector<int64_t> &ref_len = job->header.lengths;
    std::vector<int64_t> first_bucket((size_t)n_ref + 1, 0);
    for (int r = 0; r < n_ref; ++r) first_bucket[(size_t)r + 1] = first_bucket[(size_t)r] + buckets_of(ref_len[(size_t)r]);
    const int64_t n_buckets = first_bucket[(size_t)n_ref] + 1;
    if (be->begin(be->ctx, n_ref, ref_len.data(), memory)) return failed();

    int64_t records = 0, mapped = 0, unplaced = 0;
    bool sorted = true, overflow = false;
    // one read of the input, every batch through the backend
    const auto read_all = [&](bool first) -> int {
        clair_job::Batches in(job, max_blocks);
        int64_t state[SS_WORDS] = {0};
        while (!in.last) {
            if (in.next()) return 1;
            if (in.through(be->batch, be->ctx, state)) return failed();
            if (first) {
                records += state[SS_N_RECORDS];
                mapped += state[SS_MAPPED];
                unplaced += state[SS_UNPLACED];
                sorted = sorted && !state[SS_UNSORTED];
                overflow = overflow || state[SS_OVERFLOW];
            } else if (state[SS_OVERFLOW]) {
                return clair_host_fail("%s: a group outgrew --memory on its second read: the file changed", path);
            }
            state[SS_RECORDS_BEFORE] += state[SS_N_RECORDS];
            state[SS_PREV_KEY] = state[SS_LAST_KEY];
        }
        return 0;
    };

    clair_job::Writer out;
    if (out.open(path, out_path, deflate, threads)) return 1;
    // the sorted group goes out: whole payloads, and with `final` the partial one behind them
    const auto write_group = [&](bool final) -> int {
        int64_t info[SI_WORDS] = {0};
        if (be->sort(be->ctx, final ? 1 : 0, info)) return failed();
        return out.payloads(info[SI_PAYLOADS], be->emit, be->ctx, failed);
    };

    int64_t groups = 1, reads = 1;
    if (be->pass(be->ctx, 0, n_buckets, 1)) return failed();
    if (read_all(true)) return 1;
    if (!overflow) {
        if (write_group(true)) return 1;
    } else {
        std::vector<int64_t> hist((size_t)n_buckets, 0);
        if (be->histogram(be->ctx, hist.data(), n_buckets)) return failed();
        std::vector<std::pair<int64_t, int64_t>> ranges;      // consecutive buckets, greedily, up to `memory` bytes
        for (int64_t b = 0; b < n_buckets;) {
            if (hist[(size_t)b] > memory) {
                int r = 0;
                while (r < n_ref && first_bucket[(size_t)r + 1] <= b) ++r;
                if (r >= n_ref)
                    return clair_host_fail("%s: the reads without a reference hold %lld bytes, more than --memory %lld: a sort cannot split them", path,
                                           (long long)hist[(size_t)b], (long long)memory);
                const int64_t from = (b - first_bucket[(size_t)r]) << BUCKET_SHIFT;
                const bool last_of_ref = b + 1 == first_bucket[(size_t)r + 1];
                const int64_t to = last_of_ref ? std::max(ref_len[(size_t)r], from + 1) : from + ((int64_t)1 << BUCKET_SHIFT);
                return clair_host_fail("%s: the reads of %s:%lld-%lld hold %lld bytes, more than --memory %lld: a sort cannot split them", path,
                                       job->header.names[(size_t)r].c_str(), (long long)from + 1, (long long)to, (long long)hist[(size_t)b], (long long)memory);
            }
            int64_t e = b, sum = 0;
            while (e < n_buckets && sum + hist[(size_t)e] <= memory) sum += hist[(size_t)e++];
            ranges.emplace_back(b, e);
            b = e;
        }
        groups = (int64_t)ranges.size();
        for (size_t g = 0; g < ranges.size(); ++g) {
            if (be->pass(be->ctx, ranges[g].first, ranges[g].second, 0)) return failed();
            if (read_all(false)) return 1;
            ++reads;
            if (write_group(g + 1 == ranges.size())) return 1;
        }
    }
    if (out.finish()) return 1;
    stats[0] = records;
    stats[1] = mapped;
    stats[2] = unplaced;
    stats[3] = groups;
    stats[4] = reads;
    stats[5] = sorted ? 1 : 0;
    stats[6] = out.written;
    return 0;
}

}  // extern "C"
