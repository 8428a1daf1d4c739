// markdup_bam on the CPU (include/clair_host.h: clair_host_markdup_*; docs/markdup_bam.md).  Two things:
//   - the host twin of csrc/markdup.hip: the same calls and the rule of csrc/markdup_core.h as sequential loops.  Blocks are inflated by zlib
//     on a few threads (hostsrc/bgzf_file.h), records framed as host_bam_index.cpp frames them (hostsrc/bam_frame.h), every record
//     summarised, the rule resolved by std::stable_sort over the summaries, the flag bytes patched in the second read's stream, the records
//     cut every 65280 bytes and compressed by the host twin of the device compressor (host_deflate.cpp);
//   - the file driver both backends run under (hostsrc/bam_job.h): the first read, the resolution, the second read, the blocks appended
//     to the output, the EOF marker.
// Plain C++17 + zlib, no HIP.
#include "../../include/clair_host.h"
#include "../csrc/markdup_core.h"
#include "bam_frame.h"
#include "bam_job.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>

namespace {

using namespace clair_md;
using namespace clair_bgzf;
using namespace clair_frame;

static_assert(sizeof(Summary) == sizeof(clair_markdup_summary_t) && sizeof(Summary) == 32, "the summary is the header's");

// the rule over summaries [n] -> duplicate [n], counts [MC_WORDS].  The input index of a record is its place in `s`.
void resolve(const Summary *s, int64_t n, uint8_t *dup, int64_t *counts) {
    std::fill(dup, dup + n, (uint8_t)0);
    std::fill(counts, counts + MC_WORDS, (int64_t)0);
    counts[MC_RECORDS] = n;
    // 1. mates: per name hash the read 1s and the read 2s in input order, the k-th with the k-th
    std::vector<uint32_t> mate((size_t)n, NO_MATE), order;
    for (int64_t i = 0; i < n; ++i) if (s[i].bits & S_PAIRABLE) order.push_back((uint32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return std::make_tuple(s[a].hash, pair_class(s[a].bits)) < std::make_tuple(s[b].hash, pair_class(s[b].bits));
    });
    for (size_t a = 0; a < order.size();) {
        size_t e = a, first2 = a;
        while (e < order.size() && s[order[e]].hash == s[order[a]].hash) ++e;
        while (first2 < e && pair_class(s[order[first2]].bits) == 0) ++first2;
        for (size_t k = 0; a + k < first2 && first2 + k < e; ++k) {
            mate[order[a + k]] = order[first2 + k];
            mate[order[first2 + k]] = order[a + k];
        }
        a = e;
    }
    // 2. pairs: an entry per pair at its lower index; by signature, then the score from the highest down, then the index
    const auto signature = [&](uint32_t i) {
        const uint64_t a = s[i].end, b = s[mate[i]].end;
        return std::make_pair(std::min(a, b), std::max(a, b));
    };
    const auto pair_score = [&](uint32_t i) { return clamp_score((uint64_t)s[i].score + s[mate[i]].score); };
    std::vector<uint32_t> owners;
    for (int64_t i = 0; i < n; ++i) if (mate[(size_t)i] != NO_MATE && (uint32_t)i < mate[(size_t)i]) owners.push_back((uint32_t)i);
    std::stable_sort(owners.begin(), owners.end(), [&](uint32_t a, uint32_t b) {
        return std::make_tuple(signature(a), ~pair_score(a)) < std::make_tuple(signature(b), ~pair_score(b));
    });
    for (size_t k = 0; k < owners.size(); ++k)
        if (k > 0 && signature(owners[k - 1]) == signature(owners[k])) {
            dup[owners[k]] = dup[mate[owners[k]]] = 1;
            ++counts[MC_DUPLICATE_PAIRS];
        }
    counts[MC_PAIRS] = (int64_t)owners.size();
    // 3. ends: per end the paired records first, then the fragments from the highest score down; a fragment survives at the head only
    std::vector<uint32_t> ends;
    for (int64_t i = 0; i < n; ++i) if (s[i].bits & S_EXAMINED) ends.push_back((uint32_t)i);
    counts[MC_EXAMINED] = (int64_t)ends.size();
    const auto kind = [&](uint32_t i) { return mate[i] == NO_MATE ? 1 : 0; };
    std::stable_sort(ends.begin(), ends.end(), [&](uint32_t a, uint32_t b) {
        return std::make_tuple(s[a].end, kind(a), ~s[a].score) < std::make_tuple(s[b].end, kind(b), ~s[b].score);
    });
    for (size_t k = 0; k < ends.size(); ++k) {
        if (!kind(ends[k])) continue;
        ++counts[MC_FRAGMENTS];
        if (k > 0 && s[ends[k - 1]].end == s[ends[k]].end) { dup[ends[k]] = 1; ++counts[MC_DUPLICATE_FRAGMENTS]; }
    }
}

}  // namespace

struct clair_host_markdup {
    clair_frame::HostFront front;                // the batch: the stream, the record starts, the carry
    // the file
    int n_ref = -1;
    int64_t memory = 0;
    bool remove = false, resolved = false;
    std::vector<Summary> summaries;
    std::vector<uint8_t> dup;
    int64_t counts[MC_WORDS] = {0};
    int64_t marked = 0;
    clair_job::OutStream out;                    // the records of the second read
};

extern "C" {

int clair_host_markdup_create(int threads, int max_blocks, int segment_bytes, clair_host_markdup_t **out) {
    if (!out) return clair_host_fail("out is NULL");
    *out = nullptr;
    clair_host_markdup *h = new clair_host_markdup;
    if (h->front.configure(threads, max_blocks, segment_bytes)) { delete h; return 1; }
    *out = h;
    return 0;
}

void clair_host_markdup_destroy(clair_host_markdup_t *h) { delete h; }

int clair_host_markdup_begin(clair_host_markdup_t *h, int n_ref, int64_t memory, int remove) {
    if (!h || n_ref < 0) return clair_host_fail("markdup begin: bad arguments");
    if (memory < 1) return clair_host_fail("markdup begin: memory %lld", (long long)memory);
    h->n_ref = n_ref;
    h->memory = memory;
    h->remove = remove != 0;
    h->resolved = false;
    h->summaries.clear();
    h->dup.clear();
    h->front.rewind();
    h->out.rewind();
    h->marked = 0;
    return 0;
}

int clair_host_markdup_batch(clair_host_markdup_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                             const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state) {
    if (!h || !state) return clair_host_fail("markdup batch: NULL argument");
    if (h->n_ref < 0 || h->resolved) return clair_host_fail("markdup batch: begin first");
    HostFront &front = h->front;
    if (front.open_batch("markdup batch", cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    const Bytes m{front.stream.data()};
    const int64_t n_rec = (int64_t)front.starts.size(), before = (int64_t)h->summaries.size();
    if (before + n_rec > MAX_RECORDS) return clair_host_fail("more than 2^31 - 1 records: the resolution's indices are 32 bits wide");
    if ((before + n_rec) * (int64_t)sizeof(Summary) > h->memory) {
        char buf[200];
        describe_memory(buf, sizeof buf, before + n_rec, h->memory);
        return clair_host_fail("%s", buf);
    }
    for (int64_t k = 0; k < n_rec; ++k) {
        const int64_t o = front.starts[(size_t)k];
        Summary s;
        Layout y;
        const int verdict = summarize(m, o, h->n_ref, (uint32_t)(before + k), &s, &y);
        if (verdict != V_OK) {
            const Detail d{before + k, 0, 0, 0, 0, 0, front.voffset(o), m.le32(o), verdict};
            char buf[400];
            describe(buf, sizeof buf, d);
            return clair_host_fail("%s", buf);
        }
        if (s.bits & S_EXAMINED) s.score = score_of(m, y.qual, y.l_seq);
        h->summaries.push_back(s);
    }
    if (front.close_batch(last)) return 1;
    state[MS_TOTAL] = before + n_rec;
    state[MS_N_RECORDS] = n_rec;
    state[MS_CARRY] = (int64_t)front.carry.size();
    return 0;
}

int clair_host_markdup_resolve(clair_host_markdup_t *h) {
    if (!h || h->n_ref < 0) return clair_host_fail("markdup resolve: begin first");
    h->dup.resize(h->summaries.size());
    resolve(h->summaries.data(), (int64_t)h->summaries.size(), h->dup.data(), h->counts);
    h->resolved = true;
    h->front.rewind();
    h->out.rewind();
    h->marked = 0;
    return 0;
}

int clair_host_markdup_mark(clair_host_markdup_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                            const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *info) {
    if (!h || !info) return clair_host_fail("markdup mark: NULL argument");
    if (h->n_ref < 0 || !h->resolved) return clair_host_fail("markdup mark: resolve first");
    HostFront &front = h->front;
    if (front.open_batch("markdup mark", cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    const Bytes m{front.stream.data()};
    const int64_t n_rec = (int64_t)front.starts.size();
    if (h->marked + n_rec > (int64_t)h->summaries.size())
        return clair_host_fail("the second read finds more than the %zu records of the first: the file changed", h->summaries.size());
    std::vector<uint8_t> &out = h->out.bytes;
    h->out.begin();
    int64_t written = 0;
    for (int64_t k = 0; k < n_rec; ++k) {
        const int64_t o = front.starts[(size_t)k], size = 4 + (int64_t)m.le32(o);
        const size_t g = (size_t)(h->marked + k);
        const bool seen = (h->summaries[g].bits & S_EXAMINED) != 0, duplicate = seen && h->dup[g];
        if (seen) front.stream[(size_t)o + 19] = patched(front.stream[(size_t)o + 19], duplicate);
        if (h->remove && duplicate) continue;
        if (h->remove) out.insert(out.end(), front.stream.begin() + (ptrdiff_t)o, front.stream.begin() + (ptrdiff_t)(o + size));
        ++written;
    }
    if (!h->remove && n_rec > 0) out.insert(out.end(), front.stream.begin() + (ptrdiff_t)front.starts[0], front.stream.begin() + (ptrdiff_t)front.tail);
    if (front.close_batch(last)) return 1;
    h->marked += n_rec;
    if (last && h->marked != (int64_t)h->summaries.size())
        return clair_host_fail("the second read finds %lld records, the first found %zu: the file changed", (long long)h->marked, h->summaries.size());
    info[MI_PAYLOADS] = h->out.cut(last != 0);
    info[MI_BYTES] = h->out.total;
    info[MI_RECORDS] = n_rec;
    info[MI_WRITTEN] = written;
    return 0;
}

int clair_host_markdup_emit(clair_host_markdup_t *h, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) {
    if (!h) return clair_host_fail("markdup emit: bad arguments");
    return clair_job::emit_payloads(h->out.bytes.data(), h->out.total, h->front.threads, first, n, compressed, out, sizes, "markdup");
}

int clair_host_markdup_stats(clair_host_markdup_t *h, int64_t *counts) {
    if (!h || !counts || !h->resolved) return clair_host_fail("markdup stats: resolve first");
    memcpy(counts, h->counts, sizeof h->counts);
    return 0;
}

static int twin_begin(void *ctx, int n_ref, int64_t memory, int remove) { return clair_host_markdup_begin((clair_host_markdup_t *)ctx, n_ref, memory, remove); }
static int twin_batch(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                      const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state) {
    return clair_host_markdup_batch((clair_host_markdup_t *)ctx, cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry, last, state);
}
static int twin_resolve(void *ctx) { return clair_host_markdup_resolve((clair_host_markdup_t *)ctx); }
static int twin_mark(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                     const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *info) {
    return clair_host_markdup_mark((clair_host_markdup_t *)ctx, cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry, last, info);
}
static int twin_emit(void *ctx, int64_t first, int n, int compressed, uint8_t *out, int32_t *sizes) { return clair_host_markdup_emit((clair_host_markdup_t *)ctx, first, n, compressed, out, sizes); }
static int twin_stats(void *ctx, int64_t *counts) { return clair_host_markdup_stats((clair_host_markdup_t *)ctx, counts); }
static const char *twin_last_error(const void *) { return clair_host_last_error(); }

int clair_host_markdup_backend(clair_host_markdup_t *h, clair_markdup_backend_t *out) {
    if (!h || !out) return clair_host_fail("markdup backend: NULL argument");
    *out = clair_markdup_backend_t{h, twin_begin, twin_batch, twin_resolve, twin_mark, twin_emit, twin_stats, twin_last_error};
    return 0;
}

int clair_host_markdup_debug_summary(const uint8_t *stream, int64_t stream_bytes, const int64_t *starts, int64_t n, int n_ref, clair_markdup_summary_t *out) {
    if (n < 0 || n > MAX_RECORDS || stream_bytes < 0 || n_ref < 0 || (n > 0 && (!stream || !starts || !out))) return clair_host_fail("debug_summary: bad arguments");
    const Bytes m{stream};
    for (int64_t i = 0; i < n; ++i) {
        int64_t next = 0;
        if (starts[i] < 0 || step(m, starts[i], stream_bytes, &next) != STEP_NEXT) return clair_host_fail("debug_summary: no record at %lld", (long long)starts[i]);
        Summary s;
        Layout y;
        const int verdict = summarize(m, starts[i], n_ref, (uint32_t)i, &s, &y);
        if (verdict != V_OK) return clair_host_fail("debug_summary: record %lld is malformed (verdict %d)", (long long)i, verdict);
        if (s.bits & S_EXAMINED) s.score = score_of(m, y.qual, y.l_seq);
        memcpy(out + i, &s, sizeof s);
    }
    return 0;
}

int clair_host_markdup_debug_resolve(const clair_markdup_summary_t *summaries, int64_t n, uint8_t *duplicate) {
    if (n < 0 || n > MAX_RECORDS || (n > 0 && (!summaries || !duplicate))) return clair_host_fail("debug_resolve: bad arguments");
    int64_t counts[MC_WORDS];
    if (n > 0) resolve((const Summary *)summaries, n, duplicate, counts);
    return 0;
}

// ---- the file driver
int clair_host_markdup_run(clair_host_bam_job_t *job, const clair_markdup_backend_t *be, const char *out_path, int deflate, int64_t memory, int max_blocks,
                           int threads, int remove, int64_t *stats) {
    if (!job || !be || !out_path || !stats || !be->begin || !be->batch || !be->resolve || !be->mark || !be->emit || !be->stats || !be->last_error)
        return clair_host_fail("markdup run: NULL argument");
    if (check_max_blocks(max_blocks)) return 1;
    if (deflate < 0 || deflate > 2 || threads < 1 || threads > 16 || memory < 1) return clair_host_fail("markdup run: bad arguments");
    const char *path = job->path.c_str();
    const auto failed = [&] { return clair_host_fail("%s: %s", path, be->last_error(be->ctx)); };
    if (be->begin(be->ctx, (int)job->header.lengths.size(), memory, remove)) return failed();
    {   // the first read: every record summarised
        clair_job::Batches in(job, max_blocks);
        int64_t state[MS_WORDS] = {0};
        while (!in.last) {
            if (in.next()) return 1;
            if (in.through(be->batch, be->ctx, state)) return failed();
        }
    }
    if (be->resolve(be->ctx)) return failed();
    int64_t counts[MC_WORDS] = {0};
    if (be->stats(be->ctx, counts)) return failed();

    clair_job::Writer out;
    if (out.open(path, out_path, deflate, threads)) return 1;
    int64_t records_out = 0;
    {   // the second read: the flags patched, the records out
        clair_job::Batches in(job, max_blocks);
        while (!in.last) {
            if (in.next()) return 1;
            int64_t info[MI_WORDS] = {0};
            if (in.through(be->mark, be->ctx, info)) return failed();
            records_out += info[MI_WRITTEN];
            if (out.payloads(info[MI_PAYLOADS], be->emit, be->ctx, failed)) return 1;
        }
    }
    if (out.finish()) return 1;
    for (int i = 0; i < MC_WORDS; ++i) stats[i] = counts[i];
    stats[MC_WORDS] = 2 * counts[MC_DUPLICATE_PAIRS] + counts[MC_DUPLICATE_FRAGMENTS];
    stats[MC_WORDS + 1] = records_out;
    stats[MC_WORDS + 2] = out.written;
    return 0;
}

}  // extern "C"
