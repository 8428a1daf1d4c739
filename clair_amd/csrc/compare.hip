// clair_compare_*: compare_vcf on the device (include/clair_amd.h; docs/compare_vcf.md has the rule).  The rule is csrc/compare_core.h,
// shared with the host twin (hostsrc/host_compare.cpp); this file holds the handle and the kernels that run it side by side.  It is a
// translation unit of its own, outside the forward pass's sources (build.csrc_digest).
//
// _parse, per side:   1. the line starts: the line feeds of the text counted with the scan of device_scan.h (totals, one workgroup over the
//    totals, then every workgroup writes where the line after each of its line feeds begins).   2. one thread per line parses it into the two
//    record slots of its row (compare_core.h); drop counters and data rows are summed in LDS and flushed with one atomic each, the first
//    malformed line is a 64-bit minimum.   3. the kept slots are compacted in file order with the same scan.   4. one thread per record
//    clears the sortedness flag where its key is below its predecessor's.
// _permute: a gather.   _run:   5. one thread per truth record: duplicate, outside or pending; then one thread per call record: the same,
//    and a pending call looks its truth record up (lower bound of its key, then the run of equal keys) and writes both outcomes -- plain
//    byte stores, no two calls match one truth record once duplicates are out.   6. pending truth records become FN.   7. counts and QUAL
//    histograms in LDS, flushed with one 64-bit integer atomic per non-zero bin (integers: the order of the workgroups does not show).
//    8. one workgroup turns the histograms into suffix sums.
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>

#include "compare_core.h"
#include "device_buffer.h"
#include "device_scan.h"
#include "hip_status.h"

static_assert(CLAIR_CMP_COUNTS == CLAIR_COMPARE_COUNTS, "counter block");

namespace clair_cmp {

constexpr int ITEMS = 8, BLOCK = 256 * ITEMS;      // bytes / slots per thread and per workgroup of a scan (clair_amd/_capi.py COMPARE_SCAN_BLOCK)
constexpr int COUNT_ITEMS = 8;                     // records per thread of count_kernel
constexpr int N_HIST = CLAIR_CMP_TYPES * CLAIR_CMP_KINDS * CLAIR_CMP_QUAL_BINS, N_SIDE_COUNTS = CLAIR_CMP_TYPES * CLAIR_CMP_OUTCOMES;
constexpr unsigned long long NO_BAD_LINE = ~0ull;
// what the parse pass sums: data rows, then the three drop counters; then the first bad line (line << 8 | code) and the sortedness flag
enum { P_ROWS = 0, P_SYMBOLIC, P_CONTIG, P_LONG, P_SUMS, P_BAD = P_SUMS, P_SORTED, P_WORDS };

using NewlineScan = clair_scan::FlagScan<true>;
using SlotScan = clair_scan::FlagScan<false>;

// line k of the text is [start[k], start[k + 1] - 1): the entry past the last line feed closes a last line that has none
struct WriteLineStarts {
    static constexpr int PAST_END = 1;
    int64_t *start;
    static __device__ inline uint32_t seed() { return 0; }
    __device__ inline void write(const NewlineScan &, int64_t i, int64_t n, uint32_t before, uint32_t is_newline) const {
        if (i == 0) start[0] = 0;
        if (i == n || is_newline) start[before + 1] = i + 1;
    }
};

struct WriteRecords {
    static constexpr int PAST_END = 0;
    const clair_compare_record *slots;
    clair_compare_record *rec;
    static __device__ inline uint32_t seed() { return 0; }
    __device__ inline void write(const SlotScan &, int64_t i, int64_t, uint32_t before, uint32_t kept) const {
        if (kept) rec[before] = slots[i];
    }
};

__global__ __launch_bounds__(256) void parse_kernel(const uint8_t *text, const int64_t *start, int64_t n_lines, clair_compare_contigs contigs,
                                                    clair_compare_record *slots, uint8_t *kept, unsigned long long *sums) {
    __shared__ unsigned local[P_SUMS];
    if (threadIdx.x < P_SUMS) local[threadIdx.x] = 0;
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n_lines) {
        clair_compare_row row;
        const int code = clair_compare_parse_line(text, start[k], start[k + 1] - 1, (uint32_t)(k + 1), contigs, &row);
        if (code > CLAIR_CMP_ROW_DATA) atomicMin(&sums[P_BAD], ((unsigned long long)(k + 1) << 8) | (unsigned)code);
        if (code == CLAIR_CMP_ROW_DATA) atomicAdd(&local[P_ROWS], 1u);
        for (int w = 0; w < 2; ++w) {
            const bool keep = code == CLAIR_CMP_ROW_DATA && row.slot[w] == CLAIR_CMP_SLOT_KEPT;
            kept[2 * k + w] = keep;
            if (keep) slots[2 * k + w] = row.rec[w];
            else if (code == CLAIR_CMP_ROW_DATA && row.slot[w] != CLAIR_CMP_SLOT_NONE) atomicAdd(&local[P_SYMBOLIC + row.slot[w] - CLAIR_CMP_SLOT_SYMBOLIC], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < P_SUMS && local[threadIdx.x]) atomicAdd(&sums[threadIdx.x], (unsigned long long)local[threadIdx.x]);
}

__global__ __launch_bounds__(256) void sorted_kernel(const clair_compare_record *rec, int64_t n, unsigned long long *sums) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > 0 && i < n && clair_compare_key(rec[i - 1]) > clair_compare_key(rec[i])) sums[P_SORTED] = 0;      // every writer writes 0
}

__global__ __launch_bounds__(256) void keys_kernel(const clair_compare_record *rec, int64_t n, int64_t *keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) keys[i] = clair_compare_key(rec[i]);
}

// to[i] = from[perm[i]]; the host has checked that perm is a permutation of 0 .. n - 1
__global__ __launch_bounds__(256) void gather_kernel(const clair_compare_record *from, const int64_t *perm, int64_t n, clair_compare_record *to) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) to[i] = from[perm[i]];
}

struct Side {
    const uint8_t *text;
    const clair_compare_record *rec;
    uint8_t *outcome;
    int64_t n;
};

// CALLS = false: the truth's own pass, which must be complete before the calls' pass writes into truth.outcome
template <bool CALLS> __global__ __launch_bounds__(256) void join_kernel(Side me, Side truth, clair_compare_regions regions) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= me.n) return;
    uint8_t o = clair_compare_classify(me.rec, me.text, i, regions);
    if (CALLS && o == CLAIR_CMP_PENDING) {
        const clair_compare_record call = me.rec[i];
        const int64_t j = clair_compare_find(truth.rec, truth.n, truth.text, call, me.text);
        o = j < 0 ? CLAIR_CMP_FP : truth.rec[j].copies == call.copies ? CLAIR_CMP_TP : CLAIR_CMP_GT;
        if (j >= 0) truth.outcome[j] = o;
    }
    me.outcome[i] = o;
}

__global__ __launch_bounds__(256) void fn_kernel(uint8_t *outcome, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && outcome[i] == CLAIR_CMP_PENDING) outcome[i] = CLAIR_CMP_FN;
}

// a workgroup counts 256 x COUNT_ITEMS records; counts = the whole block, `side` picks the rows of counts[side][type][outcome]
template <bool CALLS> __global__ __launch_bounds__(256) void count_kernel(const clair_compare_record *rec, const uint8_t *outcome, int64_t n,
                                                                          unsigned long long *counts) {
    __shared__ unsigned hist[CALLS ? N_HIST : 1];
    __shared__ unsigned by_type[N_SIDE_COUNTS];
    if (CALLS) for (int i = threadIdx.x; i < N_HIST; i += 256) hist[i] = 0;
    if (threadIdx.x < N_SIDE_COUNTS) by_type[threadIdx.x] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * (256 * COUNT_ITEMS);
    for (int k = 0; k < COUNT_ITEMS; ++k) {
        const int64_t i = first + k * 256 + threadIdx.x;
        if (i >= n) break;
        const unsigned type = rec[i].type, o = outcome[i];
        if (type >= CLAIR_CMP_TYPES || o >= CLAIR_CMP_OUTCOMES) continue;      // neither can be: nothing is ever counted out of bounds
        atomicAdd(&by_type[type * CLAIR_CMP_OUTCOMES + o], 1u);
        if (CALLS && o < CLAIR_CMP_KINDS) atomicAdd(&hist[(type * CLAIR_CMP_KINDS + o) * CLAIR_CMP_QUAL_BINS + min((unsigned)rec[i].qual_bin, CLAIR_CMP_QUAL_BINS - 1u)], 1u);
    }
    __syncthreads();
    const int side = CALLS ? CLAIR_CMP_CALLS : CLAIR_CMP_TRUTH;
    if (threadIdx.x < N_SIDE_COUNTS && by_type[threadIdx.x]) atomicAdd(&counts[CLAIR_CMP_AT_COUNTS + side * N_SIDE_COUNTS + threadIdx.x], (unsigned long long)by_type[threadIdx.x]);
    if (CALLS) for (int i = threadIdx.x; i < N_HIST; i += 256) if (hist[i]) atomicAdd(&counts[CLAIR_CMP_AT_HIST + i], (unsigned long long)hist[i]);
}

// one workgroup: at_least[row][q] = the sum of hist[row][q ..]; thread t owns the four bins 1023 - 4 t down to 1020 - 4 t
__global__ __launch_bounds__(256) void suffix_kernel(unsigned long long *counts) {
    using Sum = clair_scan::SumScan<long long, long long>;
    for (int row = 0; row < CLAIR_CMP_TYPES * CLAIR_CMP_KINDS; ++row) {
        const unsigned long long *hist = counts + CLAIR_CMP_AT_HIST + row * CLAIR_CMP_QUAL_BINS;
        unsigned long long *at_least = counts + CLAIR_CMP_AT_AT_LEAST + row * CLAIR_CMP_QUAL_BINS;
        long long v[4], mine = 0, total;
        for (int k = 0; k < 4; ++k) { v[k] = (long long)hist[CLAIR_CMP_QUAL_BINS - 1 - (4 * (int)threadIdx.x + k)]; mine += v[k]; }
        long long run = clair_scan::block_exclusive<Sum>(mine, &total);
        for (int k = 0; k < 4; ++k) { run += v[k]; at_least[CLAIR_CMP_QUAL_BINS - 1 - (4 * (int)threadIdx.x + k)] = (unsigned long long)run; }
    }
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace clair_cmp

#include <vector>

struct clair_compare {
    int device = 0;
    std::string error;
    int n_contigs = -1;
    DeviceBuffer d_names, d_name_off, d_first, d_starts, d_ends, d_counts, d_sums, d_scan, d_slot_scan, d_line_start, d_slots, d_kept, d_perm;
    bool have_regions = false, ran = false;
    struct SideState {
        DeviceBuffer d_text, d_rec, d_other, d_outcome;      // d_other: what _permute gathers into, then swapped with d_rec
        int64_t n = 0, drops[3] = {0, 0, 0};
        bool parsed = false, sorted = false;
    } side[2];
};

namespace {

std::string g_cmp_error;
inline HipFail cmp_fail(clair_compare *h) { return {h ? h->error : g_cmp_error}; }
const char *const SIDE_NAME[2] = {"calls", "truth"};

}  // namespace

extern "C" {

const char *clair_compare_last_error(const clair_compare_t *h) { return h ? h->error.c_str() : g_cmp_error.c_str(); }

int clair_compare_create(int device, clair_compare_t **out) {
    if (!out) return cmp_fail(nullptr)("out is NULL");
    *out = nullptr;
    if (hip_device_check(cmp_fail(nullptr), device, "the device comparison runs on an MI355X only (the host twin is --backend host)")) return 1;
    clair_compare *h = new clair_compare;
    h->device = device;
    *out = h;
    return 0;
}

void clair_compare_destroy(clair_compare_t *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

int clair_compare_set_contigs(clair_compare_t *h, const uint8_t *names, const int64_t *offsets, int n_contigs) {
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (n_contigs < 0 || !offsets || (n_contigs > 0 && !names)) return cmp_fail(h)("set_contigs: bad arguments");
    for (int k = 0; k < n_contigs; ++k) if (offsets[0] != 0 || offsets[k] > offsets[k + 1]) return cmp_fail(h)("set_contigs: offsets must ascend from 0");
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    const size_t bytes = n_contigs > 0 ? (size_t)offsets[n_contigs] : 0;
    CLAIR_HIP_TRY(cmp_fail(h), h->d_names.ensure(bytes));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_name_off.ensure((size_t)(n_contigs + 1) * sizeof(int64_t)));
    if (bytes) CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_names.p, names, bytes, hipMemcpyHostToDevice));
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_name_off.p, offsets, (size_t)(n_contigs + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    h->n_contigs = n_contigs;
    h->side[0].parsed = h->side[1].parsed = h->have_regions = h->ran = false;      // ids mean something else now
    return 0;
}

int clair_compare_set_regions(clair_compare_t *h, const int64_t *first, const int64_t *starts, const int64_t *ends, int64_t n_intervals) {
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    h->ran = false;
    if (n_intervals < 0) { h->have_regions = false; return 0; }
    if (h->n_contigs < 0) return cmp_fail(h)("set_regions: set the contigs first");
    if (!first || (n_intervals > 0 && (!starts || !ends))) return cmp_fail(h)("set_regions: NULL argument");
    if (first[0] != 0 || first[h->n_contigs] != n_intervals) return cmp_fail(h)("set_regions: first[] must run from 0 to n_intervals");
    for (int k = 0; k < h->n_contigs; ++k) {
        if (first[k] > first[k + 1]) return cmp_fail(h)("set_regions: first[] must ascend");
        for (int64_t i = first[k]; i < first[k + 1]; ++i)
            if (starts[i] >= ends[i] || (i > first[k] && starts[i] <= ends[i - 1])) return cmp_fail(h)("set_regions: interval %lld is empty or not sorted and merged", (long long)i);
    }
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_first.ensure((size_t)(h->n_contigs + 1) * sizeof(int64_t)));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_starts.ensure((size_t)n_intervals * sizeof(int64_t)));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_ends.ensure((size_t)n_intervals * sizeof(int64_t)));
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_first.p, first, (size_t)(h->n_contigs + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (n_intervals) {
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_starts.p, starts, (size_t)n_intervals * sizeof(int64_t), hipMemcpyHostToDevice));
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_ends.p, ends, (size_t)n_intervals * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    h->have_regions = true;
    return 0;
}

int clair_compare_parse(clair_compare_t *h, int side, const uint8_t *text, int64_t len, int64_t *stats) {
    using namespace clair_cmp;
    using clair_scan::totals_kernel; using clair_scan::walk_kernel; using clair_scan::write_kernel;
    using Totals = clair_scan::SumScan<uint32_t, uint32_t>;
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (side < 0 || side > 1 || len < 0 || (len > 0 && !text) || !stats) return cmp_fail(h)("parse: bad arguments");
    if (h->n_contigs < 0) return cmp_fail(h)("parse: set the contigs first");
    if (len > (int64_t)UINT32_MAX) return cmp_fail(h)("parse: the %s text has %lld bytes, the limit is 2^32 - 1", SIDE_NAME[side], (long long)len);
    clair_compare::SideState &s = h->side[side];
    s.parsed = false;
    h->ran = false;
    s.n = 0;
    s.drops[0] = s.drops[1] = s.drops[2] = 0;
    int64_t n_lines = 0;
    unsigned long long sums[P_WORDS] = {0, 0, 0, 0, NO_BAD_LINE, 1};
    if (len > 0) {
        CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
        CLAIR_HIP_TRY(cmp_fail(h), s.d_text.ensure((size_t)len));
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(s.d_text.p, text, (size_t)len, hipMemcpyHostToDevice));
        CLAIR_HIP_TRY(cmp_fail(h), h->d_sums.ensure(sizeof sums));
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_sums.p, sums, sizeof sums, hipMemcpyHostToDevice));
        // 1. the line starts
        const int64_t nb = (len + 1 + BLOCK - 1) / BLOCK;      // + 1: the entry past the end has a thread of its own
        CLAIR_HIP_TRY(cmp_fail(h), h->d_scan.ensure((size_t)(nb + 1) * sizeof(uint32_t)));
        uint32_t *d_scan = h->d_scan.as<uint32_t>();
        const NewlineScan newlines{{s.d_text.as<uint8_t>()}};
        hipLaunchKernelGGL((totals_kernel<NewlineScan, ITEMS>), dim3((unsigned)nb), dim3(256), 0, nullptr, newlines, len, d_scan);
        hipLaunchKernelGGL((walk_kernel<Totals, false>), dim3(1), dim3(256), 0, nullptr, Totals{d_scan}, nb, d_scan, d_scan + nb);
        CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
        uint32_t n_feeds = 0;
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(&n_feeds, d_scan + nb, sizeof n_feeds, hipMemcpyDeviceToHost));
        if ((int64_t)n_feeds > len) return cmp_fail(h)("parse: %u line feeds in %lld bytes: the line scan is broken", n_feeds, (long long)len);
        n_lines = (int64_t)n_feeds + (text[len - 1] != '\n');
        CLAIR_HIP_TRY(cmp_fail(h), h->d_line_start.ensure((size_t)(n_feeds + 2) * sizeof(int64_t)));
        hipLaunchKernelGGL((write_kernel<NewlineScan, ITEMS, WriteLineStarts>), dim3((unsigned)nb), dim3(256), 0, nullptr, newlines, len, (const uint32_t *)d_scan,
                           WriteLineStarts{h->d_line_start.as<int64_t>()});
        // 2. one thread per line
        CLAIR_HIP_TRY(cmp_fail(h), h->d_slots.ensure((size_t)n_lines * 2 * sizeof(clair_compare_record)));
        CLAIR_HIP_TRY(cmp_fail(h), h->d_kept.ensure((size_t)n_lines * 2));
        const clair_compare_contigs contigs{h->d_names.as<uint8_t>(), h->d_name_off.as<int64_t>(), h->n_contigs};
        hipLaunchKernelGGL(parse_kernel, dim3(blocks_of(n_lines, 256)), dim3(256), 0, nullptr, (const uint8_t *)s.d_text.as<uint8_t>(),
                           (const int64_t *)h->d_line_start.as<int64_t>(), n_lines, contigs, h->d_slots.as<clair_compare_record>(), h->d_kept.as<uint8_t>(),
                           h->d_sums.as<unsigned long long>());
        // 3. the kept slots, in file order
        const int64_t n_slots = 2 * n_lines, nsb = (n_slots + BLOCK - 1) / BLOCK;
        CLAIR_HIP_TRY(cmp_fail(h), h->d_slot_scan.ensure((size_t)(nsb + 1) * sizeof(uint32_t)));      // (d_scan is still being read)
        d_scan = h->d_slot_scan.as<uint32_t>();
        const SlotScan kept{{h->d_kept.as<uint8_t>()}};
        hipLaunchKernelGGL((totals_kernel<SlotScan, ITEMS>), dim3((unsigned)nsb), dim3(256), 0, nullptr, kept, n_slots, d_scan);
        hipLaunchKernelGGL((walk_kernel<Totals, false>), dim3(1), dim3(256), 0, nullptr, Totals{d_scan}, nsb, d_scan, d_scan + nsb);
        CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
        uint32_t n_rec = 0;
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(&n_rec, d_scan + nsb, sizeof n_rec, hipMemcpyDeviceToHost));
        if ((int64_t)n_rec > n_slots) return cmp_fail(h)("parse: %u records in %lld slots: the slot scan is broken", n_rec, (long long)n_slots);
        CLAIR_HIP_TRY(cmp_fail(h), s.d_rec.ensure((size_t)n_rec * sizeof(clair_compare_record)));
        hipLaunchKernelGGL((write_kernel<SlotScan, ITEMS, WriteRecords>), dim3((unsigned)nsb), dim3(256), 0, nullptr, kept, n_slots, (const uint32_t *)d_scan,
                           WriteRecords{h->d_slots.as<clair_compare_record>(), s.d_rec.as<clair_compare_record>()});
        // 4. are they in order as they stand
        if (n_rec > 1)
            hipLaunchKernelGGL(sorted_kernel, dim3(blocks_of(n_rec, 256)), dim3(256), 0, nullptr, (const clair_compare_record *)s.d_rec.as<clair_compare_record>(),
                               (int64_t)n_rec, h->d_sums.as<unsigned long long>());
        CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(sums, h->d_sums.p, sizeof sums, hipMemcpyDeviceToHost));
        if (sums[P_BAD] != NO_BAD_LINE)
            return cmp_fail(h)("%s line %lld: %s", SIDE_NAME[side], (long long)(sums[P_BAD] >> 8), clair_compare_row_error((int)(sums[P_BAD] & 255)));
        s.n = n_rec;
    }
    for (int d = 0; d < 3; ++d) s.drops[d] = (int64_t)sums[P_SYMBOLIC + d];
    s.sorted = sums[P_SORTED] != 0;
    s.parsed = true;
    const int64_t out[CLAIR_CMP_STATS] = {n_lines, (int64_t)sums[P_ROWS], s.n, s.drops[0], s.drops[1], s.drops[2], s.sorted ? 1 : 0, 0};
    for (int i = 0; i < CLAIR_CMP_STATS; ++i) stats[i] = out[i];
    return 0;
}

int clair_compare_keys(clair_compare_t *h, int side, int64_t *keys) {
    using namespace clair_cmp;
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (side < 0 || side > 1 || !h->side[side].parsed) return cmp_fail(h)("keys: no parsed text on that side");
    clair_compare::SideState &s = h->side[side];
    if (s.n == 0) return 0;
    if (!keys) return cmp_fail(h)("keys: NULL argument");
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_perm.ensure((size_t)s.n * sizeof(int64_t)));
    hipLaunchKernelGGL(keys_kernel, dim3(blocks_of(s.n, 256)), dim3(256), 0, nullptr, (const clair_compare_record *)s.d_rec.as<clair_compare_record>(), s.n,
                       h->d_perm.as<int64_t>());
    CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(keys, h->d_perm.p, (size_t)s.n * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

int clair_compare_permute(clair_compare_t *h, int side, const int64_t *perm) {
    using namespace clair_cmp;
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (side < 0 || side > 1 || !h->side[side].parsed) return cmp_fail(h)("permute: no parsed text on that side");
    clair_compare::SideState &s = h->side[side];
    h->ran = false;
    if (s.n == 0) return 0;
    if (!perm) return cmp_fail(h)("permute: NULL argument");
    {
        std::vector<uint8_t> seen((size_t)s.n, 0);      // the gather reads rec[perm[i]]: nothing but a permutation goes to the device
        for (int64_t i = 0; i < s.n; ++i) {
            if (perm[i] < 0 || perm[i] >= s.n || seen[(size_t)perm[i]]) return cmp_fail(h)("permute: entry %lld is no permutation of 0 .. %lld", (long long)i, (long long)s.n - 1);
            seen[(size_t)perm[i]] = 1;
        }
    }
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_perm.ensure((size_t)s.n * sizeof(int64_t)));
    CLAIR_HIP_TRY(cmp_fail(h), s.d_other.ensure((size_t)s.n * sizeof(clair_compare_record)));
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_perm.p, perm, (size_t)s.n * sizeof(int64_t), hipMemcpyHostToDevice));
    unsigned long long sums[P_WORDS] = {0, 0, 0, 0, NO_BAD_LINE, 1};
    CLAIR_HIP_TRY(cmp_fail(h), h->d_sums.ensure(sizeof sums));
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_sums.p, sums, sizeof sums, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(gather_kernel, dim3(blocks_of(s.n, 256)), dim3(256), 0, nullptr, (const clair_compare_record *)s.d_rec.as<clair_compare_record>(),
                       (const int64_t *)h->d_perm.as<int64_t>(), s.n, s.d_other.as<clair_compare_record>());
    hipLaunchKernelGGL(sorted_kernel, dim3(blocks_of(s.n, 256)), dim3(256), 0, nullptr, (const clair_compare_record *)s.d_other.as<clair_compare_record>(), s.n,
                       h->d_sums.as<unsigned long long>());
    CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(sums, h->d_sums.p, sizeof sums, hipMemcpyDeviceToHost));
    std::swap(s.d_rec.p, s.d_other.p);
    std::swap(s.d_rec.bytes, s.d_other.bytes);
    s.sorted = sums[P_SORTED] != 0;
    return 0;
}

int clair_compare_run(clair_compare_t *h) {
    using namespace clair_cmp;
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    for (int k = 0; k < 2; ++k) {
        if (!h->side[k].parsed) return cmp_fail(h)("run: the %s were not parsed", SIDE_NAME[k]);
        if (!h->side[k].sorted) return cmp_fail(h)("run: the %s records are not in (contig, pos) order: permute them first", SIDE_NAME[k]);
    }
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_counts.ensure(sizeof(unsigned long long) * CLAIR_CMP_COUNTS));
    CLAIR_HIP_TRY(cmp_fail(h), hipMemsetAsync(h->d_counts.p, 0, sizeof(unsigned long long) * CLAIR_CMP_COUNTS, nullptr));
    Side sd[2];
    for (int k = 0; k < 2; ++k) {
        clair_compare::SideState &s = h->side[k];
        CLAIR_HIP_TRY(cmp_fail(h), s.d_outcome.ensure((size_t)s.n));
        sd[k] = Side{s.d_text.as<uint8_t>(), s.d_rec.as<clair_compare_record>(), s.d_outcome.as<uint8_t>(), s.n};
    }
    const Side calls = sd[CLAIR_CMP_CALLS], truth = sd[CLAIR_CMP_TRUTH];
    const clair_compare_regions regions{h->have_regions ? h->d_first.as<int64_t>() : nullptr, h->d_starts.as<int64_t>(), h->d_ends.as<int64_t>()};
    unsigned long long *counts = h->d_counts.as<unsigned long long>();
    if (truth.n) hipLaunchKernelGGL((join_kernel<false>), dim3(blocks_of(truth.n, 256)), dim3(256), 0, nullptr, truth, truth, regions);
    if (calls.n) hipLaunchKernelGGL((join_kernel<true>), dim3(blocks_of(calls.n, 256)), dim3(256), 0, nullptr, calls, truth, regions);
    if (truth.n) hipLaunchKernelGGL(fn_kernel, dim3(blocks_of(truth.n, 256)), dim3(256), 0, nullptr, truth.outcome, truth.n);
    if (calls.n) hipLaunchKernelGGL((count_kernel<true>), dim3(blocks_of(calls.n, 256 * COUNT_ITEMS)), dim3(256), 0, nullptr, calls.rec, (const uint8_t *)calls.outcome, calls.n, counts);
    if (truth.n) hipLaunchKernelGGL((count_kernel<false>), dim3(blocks_of(truth.n, 256 * COUNT_ITEMS)), dim3(256), 0, nullptr, truth.rec, (const uint8_t *)truth.outcome, truth.n, counts);
    hipLaunchKernelGGL(suffix_kernel, dim3(1), dim3(256), 0, nullptr, counts);
    CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
    CLAIR_HIP_TRY(cmp_fail(h), hipDeviceSynchronize());
    h->ran = true;
    return 0;
}

int clair_compare_counts(clair_compare_t *h, int64_t *counts) {
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (!counts || !h->ran) return cmp_fail(h)("counts: nothing was run");
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(counts, h->d_counts.p, sizeof(int64_t) * CLAIR_CMP_COUNTS, hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; ++k) for (int d = 0; d < 3; ++d) counts[CLAIR_CMP_AT_DROPS + k * 3 + d] = h->side[k].drops[d];
    return 0;
}

int clair_compare_records(clair_compare_t *h, int side, clair_compare_record_t *records, uint8_t *outcomes) {
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (side < 0 || side > 1 || !h->side[side].parsed) return cmp_fail(h)("records: no parsed text on that side");
    clair_compare::SideState &s = h->side[side];
    if (outcomes && !h->ran) return cmp_fail(h)("records: nothing was run, so there are no outcomes");
    if (s.n == 0) return 0;
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    if (records) CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(records, s.d_rec.p, (size_t)s.n * sizeof(clair_compare_record), hipMemcpyDeviceToHost));
    if (outcomes) CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(outcomes, s.d_outcome.p, (size_t)s.n, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
