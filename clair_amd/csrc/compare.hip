// clair_compare_*: compare_vcf on the device (include/clair_amd.h; docs/compare_vcf.md has the rule).  The rule is csrc/compare_core.h,
// shared with the host twin (hostsrc/host_compare.cpp); this file holds the handle and the kernels that run it side by side.  It is a
// translation unit of its own, outside the forward pass's sources (build.csrc_digest).
//
// _parse, per side:   1. the line starts: the line feeds of the text counted with the scan of device_scan.h (totals, one workgroup over the
//    totals, then every workgroup writes where the line after each of its line feeds begins).   2. one thread per line parses it into the two
//    record slots of its row (compare_core.h); drop counters and data rows are summed in LDS and flushed with one atomic each, the first
//    malformed line is a 64-bit minimum.   3. the kept slots are compacted in file order with the same scan.   4. one thread per record
//    clears the sortedness flag where its key is below its predecessor's.
// _left_align, per side (docs/compare_vcf.md, "Left alignment"):   a. the records' arena slots: an exclusive sum of ref_len + alt_len with the same
//    scan.   b. one thread per record decides its case (compare_core.h), copies the alleles of a record that stays to its slot and flags a
//    candidate; the counters are summed in LDS.   c. the candidates are compacted in record order, again with the scan.   d. one wave per
//    candidate: 64 steps to the left per ballot until a lane's bytes differ or the contig starts, then the lanes write the alleles to the slot
//    and lane 0 the record.   e. the order flag on the new positions.
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

// *in_order was set to 1 before the launch
__global__ __launch_bounds__(256) void sorted_kernel(const clair_compare_record *rec, int64_t n, unsigned long long *in_order) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i > 0 && i < n && clair_compare_key(rec[i - 1]) > clair_compare_key(rec[i])) *in_order = 0;      // every writer writes 0
}

// -- left alignment ----------------------------------------------------------------------------------------------------------------------------
constexpr int LA_WAVES = 4;      // candidates per workgroup of shift_kernel: one wave each
// what the pass sums (the first words of _left_align's stats, CLAIR_CMP_LA_*), then the sortedness flag
enum { LA_SUMS = CLAIR_CMP_LA_NO_SEQUENCE + 1, LA_IN_ORDER = CLAIR_CMP_LA_SORTED, LA_WORDS };

// the bytes a record takes in the arena; below 2^32 in all, as the alleles are parts of a text that is
struct AlleleBytes : clair_scan::SumScan<uint8_t, uint32_t> {
    const clair_compare_record *rec;
    __device__ inline T item(int64_t i) const { return (T)rec[i].ref_len + rec[i].alt_len; }
};
using CandidateScan = clair_scan::FlagScan<false>;

struct WriteSlots {
    static constexpr int PAST_END = 0;
    uint32_t *slot;
    static __device__ inline uint32_t seed() { return 0; }
    __device__ inline void write(const AlleleBytes &, int64_t i, int64_t, uint32_t before, uint32_t) const { slot[i] = before; }
};

struct WriteCandidates {
    static constexpr int PAST_END = 0;
    uint32_t *list;
    static __device__ inline uint32_t seed() { return 0; }
    __device__ inline void write(const CandidateScan &, int64_t i, int64_t, uint32_t before, uint32_t is_candidate) const {
        if (is_candidate) list[before] = (uint32_t)i;
    }
};

// One thread per record.  A record that stays is copied to its slot here and points there afterwards; a candidate is left to its wave.
__global__ __launch_bounds__(256) void la_case_kernel(const uint8_t *text, clair_compare_reference ref, clair_compare_record *rec, int64_t n, const uint32_t *slot,
                                                      uint8_t *arena, uint8_t *is_candidate, unsigned long long *sums) {
    __shared__ unsigned local[LA_SUMS];
    if (threadIdx.x < LA_SUMS) local[threadIdx.x] = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) {
        const clair_compare_record r = rec[i];
        clair_compare_event ev;
        const int what = clair_compare_la_case(ref, text, r, &ev);
        if (what != CLAIR_CMP_LA_UNTOUCHED) atomicAdd(&local[CLAIR_CMP_LA_EXAMINED], 1u);
        if (what == CLAIR_CMP_LA_IS_NO_SEQUENCE) atomicAdd(&local[CLAIR_CMP_LA_NO_SEQUENCE], 1u);
        if (what == CLAIR_CMP_LA_IS_REF_MISMATCH) atomicAdd(&local[CLAIR_CMP_LA_REF_MISMATCH], 1u);
        is_candidate[i] = what == CLAIR_CMP_LA_CANDIDATE;
        if (what != CLAIR_CMP_LA_CANDIDATE) {
            const uint32_t mine = slot[i];
            clair_compare_la_copy(text, r, mine, arena);
            rec[i].ref_off = mine;
            rec[i].alt_off = mine + r.ref_len;
        }
    }
    __syncthreads();
    if (threadIdx.x < LA_SUMS && local[threadIdx.x]) atomicAdd(&sums[threadIdx.x], (unsigned long long)local[threadIdx.x]);
}

// One wave per candidate.  Lane l of round s asks whether the event stops after s + l steps to the left; the ballot's lowest set bit is the
// answer, and as the ballot is the same in every lane, so is the loop's exit: all 64 lanes reach every ballot.  Every read of the reference
// is at a position >= 1 of the record's own contig (compare_core.h); every store is to the record's own slot, or lane 0's to its record.
__global__ __launch_bounds__(64 * LA_WAVES) void shift_kernel(const uint8_t *text, clair_compare_reference ref, clair_compare_record *rec, const uint32_t *slot,
                                                              const uint32_t *list, int64_t n_candidates, uint8_t *arena, unsigned long long *sums) {
    const int lane = threadIdx.x & 63;
    const int64_t c = (int64_t)blockIdx.x * LA_WAVES + (threadIdx.x >> 6);
    if (c >= n_candidates) return;                 // the whole wave
    const uint32_t i = list[c];
    const clair_compare_record r = rec[i];
    clair_compare_event ev;
    if (clair_compare_la_case(ref, text, r, &ev) != CLAIR_CMP_LA_CANDIDATE) return;      // cannot be: the same function flagged it; the whole wave
    const uint8_t *contig = ref.seq + ref.off[r.ctg];
    int64_t steps = 0;
    for (;;) {
        const unsigned long long stops = __ballot(clair_compare_la_stops(contig, text, ev, steps + lane));
        if (stops) { steps += __ffsll(stops) - 1; break; }
        steps += 64;
    }
    const uint32_t ref_len = r.ref_len;
    const bool ins = ref_len < r.alt_len;
    const uint32_t mine = slot[i], at_short = ins ? mine : mine + ref_len, at_long = ins ? mine + ref_len : mine;
    for (uint32_t k = lane; k <= ev.len; k += 64) arena[at_long + k] = clair_compare_la_long_byte(contig, text, ev, steps, k);
    if (lane == 0) {
        arena[at_short] = clair_compare_la_short_byte(contig, text, ev, steps);
        rec[i].ref_off = mine;
        rec[i].alt_off = mine + ref_len;
        if (ev.a - steps < 1) atomicAdd(&sums[CLAIR_CMP_LA_AT_CONTIG_START], 1ull);
        else if (ev.a - steps != r.pos) {
            rec[i].pos = (int32_t)(ev.a - steps);
            atomicAdd(&sums[CLAIR_CMP_LA_SHIFTED], 1ull);
        }
    }
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
    DeviceBuffer d_ref, d_ref_off, d_arena_slot, d_candidate, d_candidates;      // left alignment: the reference; per record its slot and flag; the list
    bool have_regions = false, have_reference = false, ran = false;
    struct SideState {
        DeviceBuffer d_text, d_rec, d_other, d_outcome;      // d_other: what _permute gathers into, then swapped with d_rec
        DeviceBuffer d_arena;                                // the alleles of a left-aligned side: what its records point into then
        int64_t n = 0, drops[3] = {0, 0, 0}, arena_bytes = 0;
        bool parsed = false, sorted = false, aligned = false;
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
    h->side[0].parsed = h->side[1].parsed = h->have_regions = h->have_reference = h->ran = false;      // ids mean something else now
    return 0;
}

int clair_compare_set_reference(clair_compare_t *h, const uint8_t *seq, const int64_t *offsets, int n_contigs) {
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (!offsets) return cmp_fail(h)("set_reference: bad arguments");
    if (h->n_contigs < 0) return cmp_fail(h)("set_reference: set the contigs first");
    if (n_contigs != h->n_contigs) return cmp_fail(h)("set_reference: %d contigs, the contig table has %d", n_contigs, h->n_contigs);
    for (int k = 0; k < n_contigs; ++k) if (offsets[0] != 0 || offsets[k] > offsets[k + 1]) return cmp_fail(h)("set_reference: offsets must ascend from 0");
    const size_t bytes = (size_t)offsets[n_contigs];
    if (bytes && !seq) return cmp_fail(h)("set_reference: NULL sequence");
    h->have_reference = false;
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_ref.ensure(bytes));
    CLAIR_HIP_TRY(cmp_fail(h), h->d_ref_off.ensure((size_t)(n_contigs + 1) * sizeof(int64_t)));
    if (bytes) CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_ref.p, seq, bytes, hipMemcpyHostToDevice));
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_ref_off.p, offsets, (size_t)(n_contigs + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    h->have_reference = true;
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
    s.parsed = s.aligned = false;
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
                               (int64_t)n_rec, h->d_sums.as<unsigned long long>() + P_SORTED);
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

int clair_compare_left_align(clair_compare_t *h, int side, int64_t *stats) {
    using namespace clair_cmp;
    using clair_scan::totals_kernel; using clair_scan::walk_kernel; using clair_scan::write_kernel;
    using Totals = clair_scan::SumScan<uint32_t, uint32_t>;
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (side < 0 || side > 1 || !stats || !h->side[side].parsed) return cmp_fail(h)("left_align: no parsed text on that side");
    if (!h->have_reference) return cmp_fail(h)("left_align: set the reference first");
    clair_compare::SideState &s = h->side[side];
    if (s.aligned) return cmp_fail(h)("left_align: the %s are left-aligned already", SIDE_NAME[side]);
    h->ran = false;
    unsigned long long sums[LA_WORDS] = {0, 0, 0, 0, 0, 1};
    uint32_t arena_bytes = 0;
    if (s.n > 0) {
        CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
        CLAIR_HIP_TRY(cmp_fail(h), h->d_sums.ensure(sizeof sums));
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(h->d_sums.p, sums, sizeof sums, hipMemcpyHostToDevice));
        clair_compare_record *rec = s.d_rec.as<clair_compare_record>();
        const uint8_t *text = s.d_text.as<uint8_t>();
        const clair_compare_reference ref{h->d_ref.as<uint8_t>(), h->d_ref_off.as<int64_t>()};
        // a. the slots
        const int64_t nb = (s.n + BLOCK - 1) / BLOCK;
        CLAIR_HIP_TRY(cmp_fail(h), h->d_scan.ensure((size_t)(nb + 1) * sizeof(uint32_t)));
        CLAIR_HIP_TRY(cmp_fail(h), h->d_slot_scan.ensure((size_t)(nb + 1) * sizeof(uint32_t)));
        CLAIR_HIP_TRY(cmp_fail(h), h->d_arena_slot.ensure((size_t)s.n * sizeof(uint32_t)));
        CLAIR_HIP_TRY(cmp_fail(h), h->d_candidate.ensure((size_t)s.n));
        uint32_t *d_scan = h->d_scan.as<uint32_t>();
        AlleleBytes lengths;
        lengths.v = nullptr;
        lengths.rec = rec;
        hipLaunchKernelGGL((totals_kernel<AlleleBytes, ITEMS>), dim3((unsigned)nb), dim3(256), 0, nullptr, lengths, s.n, d_scan);
        hipLaunchKernelGGL((walk_kernel<Totals, false>), dim3(1), dim3(256), 0, nullptr, Totals{d_scan}, nb, d_scan, d_scan + nb);
        hipLaunchKernelGGL((write_kernel<AlleleBytes, ITEMS, WriteSlots>), dim3((unsigned)nb), dim3(256), 0, nullptr, lengths, s.n, (const uint32_t *)d_scan,
                           WriteSlots{h->d_arena_slot.as<uint32_t>()});
        CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(&arena_bytes, d_scan + nb, sizeof arena_bytes, hipMemcpyDeviceToHost));
        if (arena_bytes < (uint64_t)s.n || (uint64_t)arena_bytes > (uint64_t)s.n * 2 * 65535)
            return cmp_fail(h)("left_align: %u allele bytes in %lld records: the slot scan is broken", arena_bytes, (long long)s.n);
        CLAIR_HIP_TRY(cmp_fail(h), s.d_arena.ensure((size_t)arena_bytes));
        // b. the cases; c. the candidates in record order
        hipLaunchKernelGGL(la_case_kernel, dim3(blocks_of(s.n, 256)), dim3(256), 0, nullptr, text, ref, rec, s.n, (const uint32_t *)h->d_arena_slot.as<uint32_t>(),
                           s.d_arena.as<uint8_t>(), h->d_candidate.as<uint8_t>(), h->d_sums.as<unsigned long long>());
        d_scan = h->d_slot_scan.as<uint32_t>();
        const CandidateScan flags{{h->d_candidate.as<uint8_t>()}};
        hipLaunchKernelGGL((totals_kernel<CandidateScan, ITEMS>), dim3((unsigned)nb), dim3(256), 0, nullptr, flags, s.n, d_scan);
        hipLaunchKernelGGL((walk_kernel<Totals, false>), dim3(1), dim3(256), 0, nullptr, Totals{d_scan}, nb, d_scan, d_scan + nb);
        CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
        uint32_t n_candidates = 0;
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(&n_candidates, d_scan + nb, sizeof n_candidates, hipMemcpyDeviceToHost));
        if ((int64_t)n_candidates > s.n) return cmp_fail(h)("left_align: %u candidates among %lld records: the candidate scan is broken", n_candidates, (long long)s.n);
        if (n_candidates) {
            CLAIR_HIP_TRY(cmp_fail(h), h->d_candidates.ensure((size_t)n_candidates * sizeof(uint32_t)));
            hipLaunchKernelGGL((write_kernel<CandidateScan, ITEMS, WriteCandidates>), dim3((unsigned)nb), dim3(256), 0, nullptr, flags, s.n, (const uint32_t *)d_scan,
                               WriteCandidates{h->d_candidates.as<uint32_t>()});
            // d. one wave per candidate
            hipLaunchKernelGGL(shift_kernel, dim3(blocks_of(n_candidates, LA_WAVES)), dim3(64 * LA_WAVES), 0, nullptr, text, ref, rec,
                               (const uint32_t *)h->d_arena_slot.as<uint32_t>(), (const uint32_t *)h->d_candidates.as<uint32_t>(), (int64_t)n_candidates,
                               s.d_arena.as<uint8_t>(), h->d_sums.as<unsigned long long>());
        }
        // e. the order as it is now
        if (s.n > 1)
            hipLaunchKernelGGL(sorted_kernel, dim3(blocks_of(s.n, 256)), dim3(256), 0, nullptr, (const clair_compare_record *)rec, s.n,
                               h->d_sums.as<unsigned long long>() + LA_IN_ORDER);
        CLAIR_HIP_TRY(cmp_fail(h), hipGetLastError());
        CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(sums, h->d_sums.p, sizeof sums, hipMemcpyDeviceToHost));
    }
    s.arena_bytes = arena_bytes;
    s.aligned = true;
    s.sorted = sums[LA_IN_ORDER] != 0;
    for (int i = 0; i < LA_SUMS; ++i) stats[i] = (int64_t)sums[i];
    stats[CLAIR_CMP_LA_SORTED] = s.sorted ? 1 : 0;
    stats[CLAIR_CMP_LA_ARENA] = arena_bytes;
    stats[7] = 0;
    return 0;
}

int clair_compare_allele_text(clair_compare_t *h, int side, uint8_t *out) {
    if (!h) return cmp_fail(nullptr)("compare handle is NULL");
    if (side < 0 || side > 1 || !h->side[side].parsed || !h->side[side].aligned) return cmp_fail(h)("allele_text: that side was not left-aligned");
    clair_compare::SideState &s = h->side[side];
    if (s.arena_bytes == 0) return 0;
    if (!out) return cmp_fail(h)("allele_text: NULL argument");
    CLAIR_HIP_TRY(cmp_fail(h), hipSetDevice(h->device));
    CLAIR_HIP_TRY(cmp_fail(h), hipMemcpy(out, s.d_arena.p, (size_t)s.arena_bytes, hipMemcpyDeviceToHost));
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
                       h->d_sums.as<unsigned long long>() + P_SORTED);
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
        sd[k] = Side{s.aligned ? s.d_arena.as<uint8_t>() : s.d_text.as<uint8_t>(), s.d_rec.as<clair_compare_record>(), s.d_outcome.as<uint8_t>(), s.n};
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
