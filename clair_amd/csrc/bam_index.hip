// clair_bamidx_*: the .bai of a coordinate-sorted BAM built on the device (include/clair_amd.h; docs/index_bam.md).  A translation unit of its
// own, outside the forward pass's sources (build.csrc_digest).  The rules are csrc/bam_index_core.h, shared with the host twin
// (hostsrc/host_bam_index.cpp); this file holds the kernels and the handle.  The front of a batch -- the stream and the record starts, steps 1 and
// 2 below -- is declared in bam_front.h and defined here; sort_bam (bam_sort.hip) runs on it too.
//
// A batch: the BGZF blocks are inflated (inflate_bgzf_kernel of inflate.hip, a wave per block) behind the bytes the batch before carried
// over, into one device buffer that never goes back to the host.  Records are then framed where they lie:
//   exits_kernel   a workgroup per segment of the stream: in LDS the jump table next[o] of every byte offset of the segment (o + 4 +
//                  block_size when that is a step a record could take, o itself when not: absorbing), resolved by pointer jumping to
//                  exit[o], where the chain from o leaves the segment.  A record is at least 36 bytes, so jump_rounds(segment) rounds do;
//   chain_kernel   one thread: the true chain, a table look-up per segment, from the batch's entry; segments a long record jumps over hold
//                  no record start;
//   count_kernel   a thread per segment walks its records from its true entry; the device-wide scan (device_scan.h); emit_kernel writes
//                  the record offsets.
// fields_kernel (a thread per record) computes tid, pos, end, bin and the virtual offset, checks the record and the order against the
// record before it, counts, and lowers the linear index with a 64-bit integer atomicMin; flag_kernel marks where (tid, bin) changes and the
// scan compacts the runs, which are all that goes back.  Ordinary vector loads and stores, integer atomics only, no workgroup waits for
// another, every loop is bounded by the stream's length.
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <vector>

#define CLAIR_BIX_FN __host__ __device__ inline
#include "bam_index_core.h"
#include "bam_front.h"
#include "device_buffer.h"
#include "device_scan.h"
#include "hip_status.h"
#include "inflate_core.h"
#include "inflate_launch.h"

namespace clair_bix {

constexpr int ITEMS = 4;                         // of the scans: 1024 items per workgroup
constexpr int64_t SCAN_BLOCK = 256 * ITEMS;
constexpr int PER_THREAD = SEG_MAX / 256;        // offsets of a segment a thread of exits_kernel owns, at most

using Counts = clair_scan::SumScan<uint32_t, uint32_t>;
using Flags = clair_scan::FlagScan<false>;

// grid: one workgroup of 256 per segment; dynamic LDS: seg words (32 KiB at the largest segment: several segments per CU).  Thread t owns
// offsets t, t + 256, ...: the table is written and read with consecutive words by consecutive lanes; the gathers e[e[o]] land where the data
// sends them.  A round: every lane reads, a barrier, every lane writes, a barrier.
__global__ __launch_bounds__(256) void exits_kernel(Bytes m, int64_t len, uint32_t seg, int rounds, uint32_t *__restrict__ exit_g) {
    extern __shared__ uint32_t e[];
    const int64_t base = (int64_t)blockIdx.x * seg;
    for (uint32_t o = threadIdx.x; o < seg; o += 256) e[o] = seg_next(m, base, o, len);
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
        uint32_t now[PER_THREAD];
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
            const uint32_t o = threadIdx.x + 256u * (uint32_t)i;
            now[i] = 0;
            if (o < seg) { const uint32_t v = e[o]; now[i] = v < seg ? e[v] : v; }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < PER_THREAD; ++i) {
            const uint32_t o = threadIdx.x + 256u * (uint32_t)i;
            if (o < seg) e[o] = now[i];
        }
        __syncthreads();
    }
    for (uint32_t o = threadIdx.x; o < seg; o += 256) exit_g[base + o] = e[o];
}

__global__ void chain_kernel(Bytes m, int64_t len, int64_t entry, uint32_t seg, int64_t n_seg, const uint32_t *exit_g, int64_t *seg_entry, int64_t *result) {
    if (blockIdx.x == 0 && threadIdx.x == 0) chain_walk(m, len, entry, seg, n_seg, exit_g, seg_entry, result);
}

__global__ __launch_bounds__(64) void count_kernel(Bytes m, int64_t len, uint32_t seg, int64_t n_seg, const int64_t *__restrict__ seg_entry, uint32_t *__restrict__ count) {
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t e = seg_entry[s];
    count[s] = e < 0 ? 0u : seg_records(m, len, seg, s, e, nullptr, 0, 0);
}

struct WriteFirst {                              // first[s]: the records before segment s
    static constexpr int PAST_END = 0;
    uint32_t *first;
    static __device__ inline uint32_t seed() { return 0; }
    __device__ inline void write(const Counts &, int64_t i, int64_t, uint32_t before, uint32_t) const { first[i] = before; }
};

__global__ __launch_bounds__(64) void emit_kernel(Bytes m, int64_t len, uint32_t seg, int64_t n_seg, const int64_t *__restrict__ seg_entry,
                                                  const uint32_t *__restrict__ first, int64_t *__restrict__ starts, int64_t cap) {
    const int64_t s = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seg) return;
    const int64_t e = seg_entry[s];
    if (e >= 0) (void)seg_records(m, len, seg, s, e, starts, (int64_t)first[s], cap);
}

// what the fields pass accumulates: the first offending record, then the three counters
enum { A_ERROR = 0, A_RECORDS, A_MAPPED, A_UNPLACED, A_WORDS };

struct Table {                                   // the pieces of the stream (voffset_at) and the references
    const int64_t *at;
    const uint64_t *voff;
    int n_tab;
    int n_ref;
    const int64_t *first_window;                 // n_ref + 1
};

// a thread per record
__global__ __launch_bounds__(256) void fields_kernel(Bytes m, const int64_t *__restrict__ starts, int64_t n_rec, int64_t tail, Table t, uint64_t prev_key,
                                                     int32_t *__restrict__ tid, uint32_t *__restrict__ bin, uint64_t *__restrict__ beg,
                                                     unsigned long long *__restrict__ linear, unsigned long long *__restrict__ acc) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_rec) return;
    const int64_t o = starts[k];
    Fields f = fields(m, o, t.n_ref);
    const uint64_t before = k > 0 ? order_key((int32_t)m.le32(starts[k - 1] + 4), (int32_t)m.le32(starts[k - 1] + 8)) : prev_key;
    if (f.verdict == V_OK && order_key(f.tid, f.pos) < before) f.verdict = V_UNSORTED;
    const uint64_t v = voffset_at(t.at, t.voff, t.n_tab, o);
    tid[k] = f.tid;
    bin[k] = f.bin;
    beg[k] = v;
    if (k == n_rec - 1) beg[n_rec] = voffset_at(t.at, t.voff, t.n_tab, tail);      // where the last record ends
    if (f.verdict != V_OK) {
        atomicMin(acc + A_ERROR, (unsigned long long)k << 3 | (unsigned long long)f.verdict);
        return;
    }
    atomicAdd(acc + A_RECORDS, 1ull);
    if (f.tid < 0) { atomicAdd(acc + A_UNPLACED, 1ull); return; }
    if (!(f.flag & 4)) atomicAdd(acc + A_MAPPED, 1ull);
    const int64_t w0 = t.first_window[f.tid], n_win = t.first_window[f.tid + 1] - w0;
    for (int64_t w = (f.pos > 0 ? f.pos : 0) >> WINDOW_SHIFT; w <= (f.end - 1) >> WINDOW_SHIFT && w < n_win; ++w)
        atomicMin(linear + w0 + w, (unsigned long long)v);
}

__global__ __launch_bounds__(256) void flag_kernel(const int32_t *__restrict__ tid, const uint32_t *__restrict__ bin, int64_t n_rec, uint8_t *__restrict__ opens) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n_rec) opens[k] = k == 0 || tid[k] != tid[k - 1] || bin[k] != bin[k - 1];
}

struct WriteRuns {                               // record i opens run `before`, or closes the run it is in when the next record opens one
    static constexpr int PAST_END = 0;
    const int32_t *tid;
    const uint32_t *bin;
    const uint64_t *beg;                         // n + 1
    const uint8_t *opens;
    clair_bamidx_run_t *runs;
    static __device__ inline uint32_t seed() { return 0; }
    __device__ inline void write(const Flags &, int64_t i, int64_t n, uint32_t before, uint32_t is_open) const {
        const uint32_t run = before + is_open - 1;
        if (is_open) { runs[run].tid = tid[i]; runs[run].bin = bin[i]; runs[run].beg = beg[i]; }
        if (i + 1 == n || opens[i + 1]) runs[run].end = beg[i + 1];
    }
};

// one thread: what the message about record k names
__global__ void detail_kernel(Bytes m, const int64_t *starts, int64_t k, Table t, int32_t prev_tid, int32_t prev_pos, Detail *out) {
    if (blockIdx.x || threadIdx.x) return;
    const int64_t o = starts[k];
    const Fields f = fields(m, o, t.n_ref);
    Detail d;
    d.index = k;
    d.tid = f.tid;
    d.pos = f.pos;
    d.prev_tid = k > 0 ? (int32_t)m.le32(starts[k - 1] + 4) : prev_tid;
    d.prev_pos = k > 0 ? (int32_t)m.le32(starts[k - 1] + 8) : prev_pos;
    d.end = f.end;
    d.voffset = voffset_at(t.at, t.voff, t.n_tab, o);
    d.block_size = m.le32(o);
    d.verdict = f.verdict;
    *out = d;
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace clair_bix

struct clair_bamidx : clair_bix::StageHandle {
    // the file
    int n_ref = -1;
    std::vector<int64_t> first_window;
    DeviceBuffer d_first_window, d_linear, d_acc;
    // a batch
    DeviceBuffer d_tid, d_bin, d_beg, d_opens, d_run_scan, d_runs, d_detail;
    std::vector<clair_bamidx_run_t> runs;
};

// ---- the batch front (bam_front.h): shared with bam_sort.hip
namespace clair_bix {

hipError_t at_least(DeviceBuffer &b, size_t n) {
    if (b.p && b.bytes >= n) return hipSuccess;
    return b.ensure(n + n / 2 + 256);
}

void Front::reset() {
    for (DeviceBuffer *b : {&d_stream[0], &d_stream[1], &d_cdata, &d_meta, &d_exit, &d_seg_entry, &d_count, &d_first, &d_scan, &d_starts, &d_result}) b->reset();
}

int Front::frame(const HipFail &fail, const uint8_t *stream_bytes, int64_t stream_len, int64_t entry, Framed *out) {
    using clair_scan::totals_kernel; using clair_scan::walk_kernel; using clair_scan::write_kernel;
    *out = Framed();
    out->tail = entry;
    if (stream_len == 0) return 0;
    const int64_t n_seg = (stream_len + seg - 1) / seg, nb = (n_seg + SCAN_BLOCK - 1) / SCAN_BLOCK, cap = stream_len / MIN_RECORD + 1;
    CLAIR_HIP_TRY(fail, at_least(d_exit, (size_t)(n_seg * seg) * 4));
    CLAIR_HIP_TRY(fail, at_least(d_seg_entry, (size_t)n_seg * 8));
    CLAIR_HIP_TRY(fail, at_least(d_count, (size_t)n_seg * 4));
    CLAIR_HIP_TRY(fail, at_least(d_first, (size_t)n_seg * 4));
    CLAIR_HIP_TRY(fail, at_least(d_scan, (size_t)(nb + 1) * 4));
    CLAIR_HIP_TRY(fail, at_least(d_starts, (size_t)(cap + PAD) * 8));
    CLAIR_HIP_TRY(fail, d_result.ensure(2 * 8));
    const Bytes m{stream_bytes};
    uint32_t *exit_d = d_exit.as<uint32_t>(), *count_d = d_count.as<uint32_t>(), *first_d = d_first.as<uint32_t>(), *scan_d = d_scan.as<uint32_t>();
    int64_t *seg_entry_d = d_seg_entry.as<int64_t>(), *starts_d = d_starts.as<int64_t>(), *result_d = d_result.as<int64_t>();
    hipLaunchKernelGGL(exits_kernel, dim3((unsigned)n_seg), dim3(256), seg * 4, stream, m, stream_len, seg, jump_rounds(seg), exit_d);
    hipLaunchKernelGGL(chain_kernel, dim3(1), dim3(64), 0, stream, m, stream_len, entry, seg, n_seg, (const uint32_t *)exit_d, seg_entry_d, result_d);
    hipLaunchKernelGGL(count_kernel, dim3(blocks_of(n_seg, 64)), dim3(64), 0, stream, m, stream_len, seg, n_seg, (const int64_t *)seg_entry_d, count_d);
    const Counts counts{count_d};
    hipLaunchKernelGGL((totals_kernel<Counts, ITEMS>), dim3((unsigned)nb), dim3(256), 0, stream, counts, n_seg, scan_d);
    hipLaunchKernelGGL((walk_kernel<Counts, false>), dim3(1), dim3(256), 0, stream, Counts{scan_d}, nb, scan_d, scan_d + nb);
    hipLaunchKernelGGL((write_kernel<Counts, ITEMS, WriteFirst>), dim3((unsigned)nb), dim3(256), 0, stream, counts, n_seg, (const uint32_t *)scan_d, WriteFirst{first_d});
    hipLaunchKernelGGL(emit_kernel, dim3(blocks_of(n_seg, 64)), dim3(64), 0, stream, m, stream_len, seg, n_seg, (const int64_t *)seg_entry_d, (const uint32_t *)first_d,
                       starts_d, cap);
    CLAIR_HIP_TRY(fail, hipGetLastError());
    uint32_t n_rec = 0;
    int64_t result[2] = {0, 0};
    CLAIR_HIP_TRY(fail, hipMemcpyAsync(&n_rec, scan_d + nb, 4, hipMemcpyDeviceToHost, stream));
    CLAIR_HIP_TRY(fail, hipMemcpyAsync(result, result_d, sizeof result, hipMemcpyDeviceToHost, stream));
    CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
    if ((int64_t)n_rec > cap || result[0] < entry || result[0] > stream_len) return fail("framing: %u records, tail %lld in %lld bytes: the frame pass is broken", n_rec, (long long)result[0], (long long)stream_len);
    out->n_rec = n_rec;
    out->tail = result[0];
    out->bad = result[1] != 0;
    return 0;
}

int Front::open_batch(const HipFail &fail, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                      const int64_t *coffset, int64_t end_coffset, int64_t entry) {
    if (clair_inf::check_blocks(fail, n, max_blocks, cbytes, in_at, csize, out_len)) return 1;
    len = carry;
    for (int i = 0; i < n; ++i) {
        if (coffset[i] < 0) return fail("block %d: negative offset", i);
        len += out_len[i];
    }
    if (entry > len) return fail("batch: entry %lld beyond the %lld bytes of the batch", (long long)entry, (long long)len);
    // 1. the stream: the carried bytes to the front of the other buffer, the blocks inflated behind them
    to = 1 - cur;
    CLAIR_HIP_TRY(fail, at_least(d_stream[to], (size_t)(len + PAD)));
    bytes = d_stream[to].as<uint8_t>();
    if (carry) CLAIR_HIP_TRY(fail, hipMemcpyAsync(bytes, d_stream[cur].as<uint8_t>() + carry_at, (size_t)carry, hipMemcpyDeviceToDevice, stream));
    // meta, one copy: the table (at, voff: n_tab entries each), then the blocks' arrays (inflate_launch.h)
    n_tab = n + 1 + (carry ? 1 : 0);
    const size_t N = (size_t)n, T = (size_t)n_tab;
    meta.assign(T * 16 + N * clair_inf::META_PER_BLOCK, 0);
    int64_t *at = (int64_t *)meta.data();
    uint64_t *voff = (uint64_t *)(at + T);
    m_at = at;
    m_voff = voff;
    const clair_inf::BlockMeta mb = clair_inf::carve_meta(voff + T, N);
    {
        int k = 0;
        int64_t pos = carry;
        if (carry) { at[k] = 0; voff[k++] = carry_voff; }
        for (int i = 0; i < n; ++i) {
            at[k] = pos;
            voff[k++] = (uint64_t)coffset[i] << 16;
            mb.in_at[i] = in_at[i];
            mb.out_at[i] = pos;
            mb.csize[i] = csize[i];
            mb.out_len[i] = out_len[i];
            pos += out_len[i];
        }
        at[k] = len;
        voff[k] = (uint64_t)end_coffset << 16;
    }
    CLAIR_HIP_TRY(fail, at_least(d_meta, meta.size()));
    CLAIR_HIP_TRY(fail, hipMemcpyAsync(d_meta.p, meta.data(), meta.size(), hipMemcpyHostToDevice, stream));
    d_at = d_meta.as<int64_t>();
    d_voff = (const uint64_t *)(d_at + T);
    const clair_inf::BlockMeta db = clair_inf::carve_meta(d_meta.as<int64_t>() + 2 * T, N);
    std::vector<int32_t> status(N, 0);
    if (n > 0) {
        // (the inflate kernel reads whole 16-byte pieces around each deflate stream)
        if (!d_cdata.p || d_cdata.bytes < (size_t)cbytes + 32) {
            CLAIR_HIP_TRY(fail, d_cdata.ensure((size_t)std::max<int64_t>(cbytes, (int64_t)max_blocks * 32768) + 32));
            CLAIR_HIP_TRY(fail, hipMemsetAsync(d_cdata.p, 0, d_cdata.bytes, stream));
        }
        CLAIR_HIP_TRY(fail, hipMemcpyAsync(d_cdata.p, cdata, (size_t)cbytes, hipMemcpyHostToDevice, stream));
        CLAIR_HIP_TRY(fail, clair_inf::launch_bgzf(stream, d_cdata.as<uint8_t>(), n, db, bytes));
        CLAIR_HIP_TRY(fail, hipMemcpyAsync(status.data(), db.status, N * 4, hipMemcpyDeviceToHost, stream));
    }
    // 2. the record starts (waits for the stream: the statuses are here with them)
    if (frame(fail, bytes, len, entry, &fr)) return 1;
    if (len == 0) CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
    for (int i = 0; i < n; ++i)
        if (status[(size_t)i] != 0) return fail("BGZF block at compressed offset %lld: %s", (long long)coffset[i], clair_inf::bgzf_status_text(status[(size_t)i]));
    return 0;
}

int Front::close_batch(const HipFail &fail, int last) {
    // the verdicts of the frame step: the 4 bytes of the size word the chain stopped on are all that is read back
    if (fr.bad) {
        uint8_t word[4] = {0, 0, 0, 0};
        CLAIR_HIP_TRY(fail, hipMemcpyAsync(word, bytes + fr.tail, 4, hipMemcpyDeviceToHost, stream));
        CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
        char buf[200];
        describe_bad_step(buf, sizeof buf, voffset(fr.tail), Bytes{word}.le32(0));
        return fail("%s", buf);
    }
    if (last && fr.tail < len) {
        CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
        char buf[200];
        describe_cut(buf, sizeof buf, voffset(fr.tail));
        return fail("%s", buf);
    }
    CLAIR_HIP_TRY(fail, hipStreamSynchronize(stream));
    cur = to;
    carry_at = fr.tail;
    carry = len - fr.tail;
    carry_voff = carry ? voffset(fr.tail) : 0;
    return 0;
}

}  // namespace clair_bix

namespace {

using clair_bix::at_least;
using clair_bix::PAD;

std::string g_bix_error;
inline HipFail bix_fail(clair_bamidx *h) { return {h ? h->error : g_bix_error}; }

}  // namespace

extern "C" {

const char *clair_bamidx_last_error(const clair_bamidx_t *h) { return h ? h->error.c_str() : g_bix_error.c_str(); }

int clair_bamidx_create(int device, int max_blocks, int segment_bytes, clair_bamidx_t **out) {
    if (!out) return bix_fail(nullptr)("out is NULL");
    *out = nullptr;
    clair_bamidx *h = new clair_bamidx;
    if (h->open(bix_fail(nullptr), device, max_blocks, segment_bytes, "the device index build runs on an MI355X only (the host one is index_bam --backend host)")) {
        clair_bamidx_destroy(h);
        return 1;
    }
    *out = h;
    return 0;
}

void clair_bamidx_destroy(clair_bamidx_t *h) {
    if (!h) return;
    h->settle();
    for (DeviceBuffer *b : {&h->d_first_window, &h->d_linear, &h->d_acc, &h->d_tid, &h->d_bin, &h->d_beg, &h->d_opens, &h->d_run_scan, &h->d_runs, &h->d_detail})
        b->reset();                              // before the stream goes, not in the destructor
    h->close();
    delete h;
}

int clair_bamidx_begin(clair_bamidx_t *h, int n_ref, const int64_t *ref_len) {
    using namespace clair_bix;
    if (!h) return bix_fail(nullptr)("bamidx handle is NULL");
    if (n_ref < 0 || (n_ref > 0 && !ref_len)) return bix_fail(h)("begin: bad arguments");
    h->n_ref = -1;
    h->first_window.assign((size_t)n_ref + 1, 0);
    for (int r = 0; r < n_ref; ++r) h->first_window[(size_t)r + 1] = h->first_window[(size_t)r] + windows_of(ref_len[r]);
    const size_t n_win = (size_t)h->first_window[(size_t)n_ref];
    CLAIR_HIP_TRY(bix_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(bix_fail(h), hipStreamSynchronize(h->stream));
    CLAIR_HIP_TRY(bix_fail(h), h->d_first_window.ensure(((size_t)n_ref + 1) * 8));
    CLAIR_HIP_TRY(bix_fail(h), h->d_linear.ensure(n_win * 8));
    CLAIR_HIP_TRY(bix_fail(h), h->d_acc.ensure(A_WORDS * 8));
    CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(h->d_first_window.p, h->first_window.data(), ((size_t)n_ref + 1) * 8, hipMemcpyHostToDevice, h->stream));
    if (n_win) CLAIR_HIP_TRY(bix_fail(h), hipMemsetAsync(h->d_linear.p, 0xff, n_win * 8, h->stream));
    const unsigned long long acc[A_WORDS] = {NO_ERROR, 0, 0, 0};
    CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(h->d_acc.p, acc, sizeof acc, hipMemcpyHostToDevice, h->stream));
    CLAIR_HIP_TRY(bix_fail(h), hipStreamSynchronize(h->stream));
    h->front.rewind();
    h->n_ref = n_ref;
    return 0;
}

int clair_bamidx_batch(clair_bamidx_t *h, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                       const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state, const clair_bamidx_run_t **runs) {
    using namespace clair_bix;
    using clair_scan::totals_kernel; using clair_scan::walk_kernel; using clair_scan::write_kernel;
    using Totals = clair_scan::SumScan<uint32_t, uint32_t>;
    if (!h) return bix_fail(nullptr)("bamidx handle is NULL");
    if (!state || !runs) return bix_fail(h)("batch: NULL argument");
    if (h->n_ref < 0) return bix_fail(h)("batch: begin first");
    if (check_batch_args(bix_fail(h), "batch", cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    const int n_ref = h->n_ref;
    h->n_ref = -1;                               // a batch that fails leaves a handle that wants begin
    CLAIR_HIP_TRY(bix_fail(h), hipSetDevice(h->device));
    // 1, 2. the stream and the record starts (bam_front.h)
    Front &front = h->front;
    if (front.open_batch(bix_fail(h), cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry)) return 1;
    const Framed &fr = front.fr;
    const int64_t len = front.len;
    uint8_t *d_stream = front.bytes;
    const int n_tab = front.n_tab;
    const int64_t n_rec = fr.n_rec;
    const Bytes m{d_stream};
    const Table table{front.d_at, front.d_voff, n_tab, n_ref, h->d_first_window.as<int64_t>()};
    h->runs.clear();
    uint32_t n_runs = 0;
    if (n_rec > 0) {
        // 3, 5. fields, virtual offsets, the linear index
        const int64_t nb = (n_rec + SCAN_BLOCK - 1) / SCAN_BLOCK;
        CLAIR_HIP_TRY(bix_fail(h), at_least(h->d_tid, (size_t)n_rec * 4));
        CLAIR_HIP_TRY(bix_fail(h), at_least(h->d_bin, (size_t)n_rec * 4));
        CLAIR_HIP_TRY(bix_fail(h), at_least(h->d_beg, (size_t)(n_rec + 1) * 8));
        CLAIR_HIP_TRY(bix_fail(h), at_least(h->d_opens, (size_t)n_rec));
        CLAIR_HIP_TRY(bix_fail(h), at_least(h->d_run_scan, (size_t)(nb + 1) * 4));
        CLAIR_HIP_TRY(bix_fail(h), at_least(h->d_runs, (size_t)n_rec * sizeof(clair_bamidx_run_t)));
        const int64_t *d_starts = front.starts();
        int32_t *d_tid = h->d_tid.as<int32_t>();
        uint32_t *d_bin = h->d_bin.as<uint32_t>(), *d_scan = h->d_run_scan.as<uint32_t>();
        uint64_t *d_beg = h->d_beg.as<uint64_t>();
        uint8_t *d_opens = h->d_opens.as<uint8_t>();
        unsigned long long *d_acc = h->d_acc.as<unsigned long long>();
        hipLaunchKernelGGL(fields_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, h->stream, m, d_starts, n_rec, fr.tail, table,
                           order_key((int32_t)state[ST_PREV_TID], (int32_t)state[ST_PREV_POS]), d_tid, d_bin, d_beg, h->d_linear.as<unsigned long long>(), d_acc);
        // 4. the runs
        hipLaunchKernelGGL(flag_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, h->stream, (const int32_t *)d_tid, (const uint32_t *)d_bin, n_rec, d_opens);
        const Flags opens{{d_opens}};
        hipLaunchKernelGGL((totals_kernel<Flags, ITEMS>), dim3((unsigned)nb), dim3(256), 0, h->stream, opens, n_rec, d_scan);
        hipLaunchKernelGGL((walk_kernel<Totals, false>), dim3(1), dim3(256), 0, h->stream, Totals{d_scan}, nb, d_scan, d_scan + nb);
        hipLaunchKernelGGL((write_kernel<Flags, ITEMS, WriteRuns>), dim3((unsigned)nb), dim3(256), 0, h->stream, opens, n_rec, (const uint32_t *)d_scan,
                           WriteRuns{d_tid, d_bin, d_beg, d_opens, h->d_runs.as<clair_bamidx_run_t>()});
        CLAIR_HIP_TRY(bix_fail(h), hipGetLastError());
        unsigned long long err = NO_ERROR;
        CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(&n_runs, d_scan + nb, 4, hipMemcpyDeviceToHost, h->stream));
        CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(&err, d_acc + A_ERROR, 8, hipMemcpyDeviceToHost, h->stream));
        CLAIR_HIP_TRY(bix_fail(h), hipStreamSynchronize(h->stream));
        if (err != NO_ERROR) {
            const int64_t k = (int64_t)(err >> 3);
            if (k >= n_rec) return bix_fail(h)("batch: offending record %lld of %lld: the fields pass is broken", (long long)k, (long long)n_rec);
            CLAIR_HIP_TRY(bix_fail(h), h->d_detail.ensure(sizeof(Detail)));
            hipLaunchKernelGGL(detail_kernel, dim3(1), dim3(64), 0, h->stream, m, d_starts, k, table, (int32_t)state[ST_PREV_TID], (int32_t)state[ST_PREV_POS], h->d_detail.as<Detail>());
            CLAIR_HIP_TRY(bix_fail(h), hipGetLastError());
            Detail d;
            CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(&d, h->d_detail.p, sizeof d, hipMemcpyDeviceToHost, h->stream));
            CLAIR_HIP_TRY(bix_fail(h), hipStreamSynchronize(h->stream));
            d.index += state[ST_RECORDS_BEFORE];
            d.verdict = (int32_t)(err & 7);
            char buf[400];
            describe(buf, sizeof buf, d);
            return bix_fail(h)("%s", buf);
        }
        if ((int64_t)n_runs > n_rec || n_runs == 0) return bix_fail(h)("batch: %u runs of %lld records: the run scan is broken", n_runs, (long long)n_rec);
        // 6. only the runs come back
        h->runs.resize(n_runs);
        CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(h->runs.data(), h->d_runs.p, (size_t)n_runs * sizeof(clair_bamidx_run_t), hipMemcpyDeviceToHost, h->stream));
    }
    if (front.close_batch(bix_fail(h), last)) return 1;
    // the last record's (tid, pos): 8 bytes
    int32_t last_key[2] = {(int32_t)state[ST_PREV_TID], (int32_t)state[ST_PREV_POS]};
    if (n_rec > 0) {
        int64_t last_start = 0;
        CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(&last_start, front.starts() + (n_rec - 1), 8, hipMemcpyDeviceToHost, h->stream));
        CLAIR_HIP_TRY(bix_fail(h), hipStreamSynchronize(h->stream));
        if (last_start < 0 || last_start + 12 > len) return bix_fail(h)("batch: last record at %lld of %lld bytes: the frame pass is broken", (long long)last_start, (long long)len);
        CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(last_key, d_stream + last_start + 4, 8, hipMemcpyDeviceToHost, h->stream));
    }
    CLAIR_HIP_TRY(bix_fail(h), hipStreamSynchronize(h->stream));
    state[ST_N_RECORDS] = n_rec;
    state[ST_N_RUNS] = (int64_t)n_runs;
    state[ST_LAST_TID] = last_key[0];
    state[ST_LAST_POS] = last_key[1];
    state[ST_CARRY] = front.carry;
    *runs = h->runs.data();
    h->n_ref = n_ref;
    return 0;
}

int clair_bamidx_finish(clair_bamidx_t *h, uint64_t *linear, int64_t n_windows, int64_t *counts) {
    using namespace clair_bix;
    if (!h) return bix_fail(nullptr)("bamidx handle is NULL");
    if (!counts || h->n_ref < 0) return bix_fail(h)("finish: no file begun, or counts is NULL");
    if (n_windows != h->first_window.back() || (n_windows > 0 && !linear)) return bix_fail(h)("finish: %lld windows, the handle has %lld", (long long)n_windows, (long long)h->first_window.back());
    CLAIR_HIP_TRY(bix_fail(h), hipSetDevice(h->device));
    unsigned long long acc[A_WORDS];
    if (n_windows) CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(linear, h->d_linear.p, (size_t)n_windows * 8, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(acc, h->d_acc.p, sizeof acc, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(bix_fail(h), hipStreamSynchronize(h->stream));
    for (int i = 0; i < 3; ++i) counts[i] = (int64_t)acc[A_RECORDS + i];
    return 0;
}

static int bix_begin(void *ctx, int n_ref, const int64_t *ref_len) { return clair_bamidx_begin((clair_bamidx_t *)ctx, n_ref, ref_len); }
static int bix_batch(void *ctx, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                     const int64_t *coffset, int64_t end_coffset, int64_t entry, int last, int64_t *state, const clair_bamidx_run_t **runs) {
    return clair_bamidx_batch((clair_bamidx_t *)ctx, cdata, cbytes, n, in_at, csize, out_len, coffset, end_coffset, entry, last, state, runs);
}
static int bix_finish(void *ctx, uint64_t *linear, int64_t n_windows, int64_t *counts) { return clair_bamidx_finish((clair_bamidx_t *)ctx, linear, n_windows, counts); }
static const char *bix_last_error(const void *ctx) { return clair_bamidx_last_error((const clair_bamidx_t *)ctx); }

int clair_bamidx_backend(clair_bamidx_t *h, clair_bamidx_backend_t *out) {
    if (!h || !out) return bix_fail(h)("backend: NULL argument");
    *out = clair_bamidx_backend_t{h, bix_begin, bix_batch, bix_finish, bix_last_error};
    return 0;
}

int clair_bamidx_debug_frame(clair_bamidx_t *h, const uint8_t *stream, int64_t n, int64_t entry, int64_t *starts, int64_t cap, int64_t *result) {
    using namespace clair_bix;
    if (!h) return bix_fail(nullptr)("bamidx handle is NULL");
    if (n < 0 || n > (int64_t)INT32_MAX || (n > 0 && !stream) || entry < 0 || entry > n || cap < 0 || (cap > 0 && !starts) || !result) return bix_fail(h)("debug_frame: bad arguments");
    CLAIR_HIP_TRY(bix_fail(h), hipSetDevice(h->device));
    Front &front = h->front;
    front.rewind();                              // the stream buffers are borrowed: a file in progress is over
    h->n_ref = -1;
    const int64_t max_rec = n / MIN_RECORD + 1;
    CLAIR_HIP_TRY(bix_fail(h), at_least(front.d_stream[0], (size_t)(n + PAD)));
    CLAIR_HIP_TRY(bix_fail(h), at_least(front.d_starts, (size_t)(max_rec + PAD) * 8));
    uint8_t *d_stream = front.d_stream[0].as<uint8_t>();
    // sentinels: PAD bytes behind the stream, PAD words behind the most offsets there can be
    CLAIR_HIP_TRY(bix_fail(h), hipMemsetAsync(d_stream + n, 0xa5, (size_t)PAD, h->stream));
    CLAIR_HIP_TRY(bix_fail(h), hipMemsetAsync(front.d_starts.as<int64_t>() + max_rec, 0xa5, (size_t)PAD * 8, h->stream));
    if (n) CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(d_stream, stream, (size_t)n, hipMemcpyHostToDevice, h->stream));
    Framed fr;
    if (front.frame(bix_fail(h), d_stream, n, entry, &fr)) return 1;
    if (fr.n_rec > cap) return bix_fail(h)("debug_frame: %lld records, room for %lld", (long long)fr.n_rec, (long long)cap);
    uint8_t behind[PAD + PAD * 8];
    if (fr.n_rec) CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(starts, front.d_starts.p, (size_t)fr.n_rec * 8, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(behind, d_stream + n, (size_t)PAD, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(bix_fail(h), hipMemcpyAsync(behind + PAD, front.d_starts.as<int64_t>() + max_rec, (size_t)PAD * 8, hipMemcpyDeviceToHost, h->stream));
    CLAIR_HIP_TRY(bix_fail(h), hipStreamSynchronize(h->stream));
    bool intact = true;
    for (uint8_t b : behind) intact = intact && b == 0xa5;
    result[FR_N_STARTS] = fr.n_rec;
    result[FR_TAIL] = fr.tail;
    result[FR_BAD] = fr.bad ? 1 : 0;
    result[FR_SENTINELS] = intact ? 1 : 0;
    return 0;
}

}  // extern "C"
