// The training-set builder on the device (include/clair_amd.h: clair_frontend_sample_candidates, _pair, _train_set_info, _train_set_counts;
// docs/train_set.md).  Included at the end of frontend.hip: it works on that handle's tallies, candidate flags and windows.
//
// What the reference does in three processes over text (ExtractVariantCandidates.py --gen4Training thins the positions with Python's
// random module, PairWithNonVariants.py thins the non-variant tensors against the variant ones, get_training_array joins the truth
// labels) is done here on the tables that are in HBM already:
//   ts_sample_kernel        a thread per position: fe_candidate_flags_kernel has marked the eligible ones (its rule with min_af = 0); this
//                           one bisects the truth positions for the class, draws, and clears the flag of a position that is not sampled;
//   ts_window_class_kernel  a thread per window: at a truth position / a usable non-variant;
//   ts_pair_kernel          a thread per window: the usable non-variant windows whose draw is below r;
//   ts_label_kernel         a thread per byte of the kept rows' reference bases; the first of a row also writes its centre, its four label
//                           bytes and its data-set flag;
//   ts_gather_kernel        a wave per kept row: its 2 112 bytes of counts into a staging buffer, 16 bytes per lane and step.
// The rules are csrc/train_set_core.h, the code hostsrc/host_train_set.cpp runs.  Counting and compaction go through the block scan of
// frontend.hip; the two sampling counters are integer atomics.  Nothing is ordered by arrival: the same inputs give the same bytes.
#include "train_set_core.h"

namespace {

constexpr int TS_ROW_VEC = WINDOW_VALUES * 2 / 16;      // 132 vectors of 16 bytes per window
constexpr int64_t TS_STAGE_ROWS = 4096;                 // rows gathered per launch: 8.6 MB of staging (a larger request goes in several)

__global__ __launch_bounds__(256) void ts_sample_kernel(int64_t lo, int64_t n, uint8_t *flags, const int64_t *truth, int64_t n_truth, double p_near,
                                                        double p_outside, uint64_t key, unsigned long long *counters) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int cls = CLAIR_TS_TRUTH;
    bool sampled = false;
    if (t < n && flags[t]) {
        const int64_t pos = lo + t + 1;
        cls = clair_ts_class(truth, n_truth, pos);
        sampled = clair_ts_sampled(cls, clair_ts_draw(key, pos), p_near, p_outside);
        if (!sampled) flags[t] = 0;
    }
    // the reference's two log counters: one atomic per wave and counter
    const unsigned long long near = __ballot(sampled && cls == CLAIR_TS_NEAR), outside = __ballot(sampled && cls != CLAIR_TS_NEAR);
    if ((threadIdx.x & 63) == 0) {
        if (near) atomicAdd(&counters[0], (unsigned long long)__popcll(near));
        if (outside) atomicAdd(&counters[1], (unsigned long long)__popcll(outside));
    }
}

struct TruthAndBed {
    const int64_t *truth;
    const uint8_t *truth_labels;     // [n_truth][4]
    int64_t n_truth;
    const int64_t *bed_start, *bed_end;
    int64_t n_bed;                   // -1: no bed file
};

__global__ __launch_bounds__(256) void ts_window_class_kernel(const int64_t *centre, int64_t n_windows, TruthAndBed tb, uint8_t *is_variant, uint8_t *usable) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_windows) return;
    const int64_t pos = centre[i];
    is_variant[i] = clair_ts_class(tb.truth, tb.n_truth, pos) == CLAIR_TS_TRUTH ? 1 : 0;
    usable[i] = clair_ts_usable(tb.truth, tb.n_truth, tb.bed_start, tb.bed_end, tb.n_bed, pos) ? 1 : 0;
}

__global__ __launch_bounds__(256) void ts_pair_kernel(const int64_t *centre, int64_t n_windows, const uint8_t *usable, double r, uint64_t key, uint8_t *keep) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_windows) return;
    keep[i] = usable[i] && clair_ts_paired(clair_ts_draw(key, centre[i]), r) ? 1 : 0;
}

__global__ __launch_bounds__(256) void ts_label_kernel(const int64_t *centre, const uint8_t *refseq, const int64_t *kept, int64_t n_kept, TruthAndBed tb,
                                                       int64_t *out_centre, uint8_t *out_refseq, uint8_t *labels, uint8_t *in_set) {
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = id / 34;
    if (j >= n_kept) return;
    const int k = (int)(id - j * 34);
    const int64_t i = kept[j];
    out_refseq[id] = refseq[i * 34 + k];
    if (k) return;
    const int64_t pos = centre[i];
    const uint8_t base = refseq[i * 34 + 16];
    out_centre[j] = pos;
    clair_ts_label(tb.truth, tb.truth_labels, tb.n_truth, pos, base, labels + j * 4);
    in_set[j] = clair_ts_in_set(tb.bed_start, tb.bed_end, tb.n_bed, pos, base) ? 1 : 0;
}

// rows [0, n) of `kept` (window indices, all < n_windows by construction of the list) -> stage[n][132]
__global__ __launch_bounds__(256) void ts_gather_kernel(const uint4 *counts, const int64_t *kept, int64_t n, uint4 *stage) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const uint4 *src = counts + kept[row] * TS_ROW_VEC;
    uint4 *dst = stage + row * TS_ROW_VEC;
    for (int q = threadIdx.x & 63; q < TS_ROW_VEC; q += 64) dst[q] = src[q];
}

// truth positions (ascending) and the contig's bed intervals on the device, for the length of one call
struct TruthOnDevice {
    DeviceBuffer positions, labels;
    TruthAndBed view{};
};

int upload_truth(clair_frontend *f, const int64_t *truth, const uint8_t *labels, int64_t n_truth, const int64_t *bed_start, const int64_t *bed_end, int64_t n_bed,
                 TruthOnDevice &d) {
    for (int64_t i = 1; i < n_truth; ++i)
        if (truth[i] < truth[i - 1]) return fe_fail(f)("truth positions not ascending");
    CLAIR_HIP_TRY(fe_fail(f), d.positions.ensure((size_t)n_truth * sizeof(int64_t)));
    if (n_truth) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(d.positions.p, truth, (size_t)n_truth * sizeof(int64_t), hipMemcpyHostToDevice));
    if (labels) {
        CLAIR_HIP_TRY(fe_fail(f), d.labels.ensure((size_t)n_truth * 4));
        if (n_truth) CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(d.labels.p, labels, (size_t)n_truth * 4, hipMemcpyHostToDevice));
    }
    d.view = TruthAndBed{d.positions.as<const int64_t>(), d.labels.as<const uint8_t>(), n_truth, nullptr, nullptr, n_bed < 0 ? -1 : 0};
    if (n_bed > 0 && upload_bed(f, bed_start, bed_end, n_bed, &d.view.bed_start, &d.view.bed_end, &d.view.n_bed)) return 1;
    return 0;
}

}  // namespace

extern "C" {

int clair_frontend_sample_candidates(clair_frontend_t *f, double min_coverage, int64_t ctg_start, int64_t ctg_end, const int64_t *bed_start, const int64_t *bed_end,
                                     int64_t n_bed, const int64_t *truth_positions, int64_t n_truth, double p_near, double p_outside, int64_t key, int add_truth,
                                     int64_t *n_candidates, int64_t *n_near, int64_t *n_outside) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!n_candidates || !n_near || !n_outside) return fe_fail(f)("NULL output pointer");
    if (n_truth < 0 || (n_truth > 0 && !truth_positions)) return fe_fail(f)("bad truth list");
    if (n_bed > 0 && (!bed_start || !bed_end)) return fe_fail(f)("bed intervals missing");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    TruthOnDevice d;
    if (upload_truth(f, truth_positions, nullptr, n_truth, bed_start, bed_end, n_bed, d)) return 1;
    const bool have_range = ctg_start >= 0 && ctg_end >= 0;
    // the eligible positions: the candidate filter with min_af = 0, which is what --gen4Training makes of it (ExtractVariantCandidates.py:197-199)
    const CandidateRule rule{min_coverage, 0.0, have_range ? ctg_start : -1, ctg_end, d.view.bed_start, d.view.bed_end, d.view.n_bed};
    uint8_t *flags = f->flags.as<uint8_t>();
    DeviceBuffer counters;
    CLAIR_HIP_TRY(fe_fail(f), counters.ensure(2 * sizeof(unsigned long long)));
    CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(counters.p, 0, counters.bytes, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipMemsetAsync(flags, 0, (size_t)f->g.n + 1, f->stream));
    hipLaunchKernelGGL(fe_candidate_flags_kernel, dim3(blocks_for(f->g.n, 256)), dim3(256), 0, f->stream, f->g, rule, flags);
    hipLaunchKernelGGL(ts_sample_kernel, dim3(blocks_for(f->g.n, 256)), dim3(256), 0, f->stream, f->g.lo, f->g.n, flags, d.view.truth, n_truth, p_near, p_outside,
                       (uint64_t)key, counters.as<unsigned long long>());
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    DeviceBuffer d_add;
    if (add_truth) {             // the truth sites of the range join the list (as callVarBam --vcf_fn restricts them); a repeated position is one site
        std::vector<int64_t> add;
        for (int64_t i = 0; i < n_truth; ++i)
            if (!have_range || (ctg_start <= truth_positions[i] && truth_positions[i] <= ctg_end)) add.push_back(truth_positions[i]);
        if (!add.empty()) {
            CLAIR_HIP_TRY(fe_fail(f), d_add.ensure(add.size() * sizeof(int64_t)));
            CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(d_add.p, add.data(), add.size() * sizeof(int64_t), hipMemcpyHostToDevice, f->stream));
            hipLaunchKernelGGL(fe_given_flags_kernel, dim3(blocks_for((int64_t)add.size(), 256)), dim3(256), 0, f->stream, d_add.as<const int64_t>(), (int64_t)add.size(),
                               f->g.lo, f->g.n, flags);
            CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
        }
        CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));     // `add` is read by the copy until here
    }
    unsigned long long counted[2] = {0, 0};
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync(counted, counters.p, sizeof counted, hipMemcpyDeviceToHost, f->stream));
    CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    *n_near = (int64_t)counted[0];
    *n_outside = (int64_t)counted[1];
    return finish_candidates(f, n_candidates);
}

int clair_frontend_pair(clair_frontend_t *f, const int64_t *truth_positions, const uint8_t *truth_labels, int64_t n_truth, const int64_t *bed_start,
                        const int64_t *bed_end, int64_t n_bed, double amp, int64_t key, int64_t *stats) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (!stats) return fe_fail(f)("stats is NULL");
    if (f->n_windows < 0) return fe_fail(f)("no windows yet: call clair_frontend_build_windows first");
    if (n_truth < 0 || (n_truth > 0 && (!truth_positions || !truth_labels))) return fe_fail(f)("bad truth list");
    if (n_bed > 0 && (!bed_start || !bed_end)) return fe_fail(f)("bed intervals missing");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    CandidateBuffers &cb = *f->cand;
    cb.ts_n_kept = -1;
    TruthOnDevice d;
    if (upload_truth(f, truth_positions, truth_labels, n_truth, bed_start, bed_end, n_bed, d)) return 1;
    const int64_t nw = f->n_windows, room = std::max<int64_t>(nw, 1);
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_flags.ensure(3 * ((size_t)room + 1)));
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_kept.ensure((size_t)room * sizeof(int64_t)));
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_block_sum.ensure(((size_t)blocks_for(room + 1, SCAN_BLOCK) + 1) * sizeof(uint32_t)));
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_total.ensure(sizeof(uint32_t)));
    uint8_t *is_variant = cb.ts_flags.as<uint8_t>(), *usable = is_variant + room + 1, *keep = usable + room + 1;
    uint32_t *block_sum = cb.ts_block_sum.as<uint32_t>(), *d_total = cb.ts_total.as<uint32_t>();
    int64_t *kept = cb.ts_kept.as<int64_t>();
    const int64_t *centre = cb.out_centre.as<const int64_t>();
    if (nw) hipLaunchKernelGGL(ts_window_class_kernel, dim3(blocks_for(nw, 256)), dim3(256), 0, f->stream, centre, nw, d.view, is_variant, usable);
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    // v and the variant windows, in position order, at the head of the kept list
    int64_t v = 0, c = 0, kept_non = 0, in_set = 0;
    if (scan_count(f, is_variant, nw, block_sum, d_total, &v)) return 1;
    if (scan_write(f, is_variant, nw, block_sum, d_total, nullptr, kept, 0)) return 1;
    if (scan_count(f, usable, nw, block_sum, d_total, &c)) return 1;
    const double r = clair_ts_ratio(v, amp, c);
    if (nw) hipLaunchKernelGGL(ts_pair_kernel, dim3(blocks_for(nw, 256)), dim3(256), 0, f->stream, centre, nw, (const uint8_t *)usable, r, (uint64_t)key, keep);
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    // ... then the kept non-variant windows, in position order: the order of the reference's paired file
    if (scan_count(f, keep, nw, block_sum, d_total, &kept_non)) return 1;
    if (scan_write(f, keep, nw, block_sum, d_total, nullptr, kept + v, 0)) return 1;
    const int64_t nk = v + kept_non, rows = std::max<int64_t>(nk, 1);
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_centre.ensure((size_t)rows * sizeof(int64_t)));
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_refseq.ensure((size_t)rows * 34));
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_labels.ensure((size_t)rows * 4));
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_in_set.ensure((size_t)rows + 1));
    if (nk)
        hipLaunchKernelGGL(ts_label_kernel, dim3(blocks_for(nk * 34, 256)), dim3(256), 0, f->stream, centre, cb.out_refseq.as<const uint8_t>(), (const int64_t *)kept, nk, d.view,
                           cb.ts_centre.as<int64_t>(), cb.ts_refseq.as<uint8_t>(), cb.ts_labels.as<uint8_t>(), cb.ts_in_set.as<uint8_t>());
    CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
    if (scan_count(f, cb.ts_in_set.as<uint8_t>(), nk, block_sum, d_total, &in_set)) return 1;     // (synchronises: `d` may go)
    cb.ts_n_kept = nk;
    stats[0] = v;
    stats[1] = c;
    stats[2] = v;
    stats[3] = kept_non;
    stats[4] = in_set;
    return 0;
}

static int ts_range(clair_frontend *f, int64_t first, int64_t n) {
    if (f->n_windows < 0 || f->cand->ts_n_kept < 0) return fe_fail(f)("no paired set yet: call clair_frontend_pair after clair_frontend_build_windows");
    if (first < 0 || n < 0 || first + n > f->cand->ts_n_kept)
        return fe_fail(f)("rows [%lld, %lld) out of range [0, %lld)", (long long)first, (long long)(first + n), (long long)f->cand->ts_n_kept);
    return 0;
}

int clair_frontend_train_set_info(clair_frontend_t *f, int64_t first, int64_t n, int64_t *centres, char *refseq, uint8_t *labels, uint8_t *in_set) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (ts_range(f, first, n)) return 1;
    if (n == 0) return 0;
    if (!centres || !refseq || !labels || !in_set) return fe_fail(f)("NULL output pointer");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    const CandidateBuffers &cb = *f->cand;
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(centres, cb.ts_centre.as<int64_t>() + first, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(refseq, cb.ts_refseq.as<uint8_t>() + first * 34, (size_t)n * 34, hipMemcpyDeviceToHost));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(labels, cb.ts_labels.as<uint8_t>() + first * 4, (size_t)n * 4, hipMemcpyDeviceToHost));
    CLAIR_HIP_TRY(fe_fail(f), hipMemcpy(in_set, cb.ts_in_set.as<uint8_t>() + first, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

int clair_frontend_train_set_counts(clair_frontend_t *f, int64_t first, int64_t n, int16_t *counts) {
    if (!f) return fe_fail(nullptr)("front end is NULL");
    if (ts_range(f, first, n)) return 1;
    if (n == 0) return 0;
    if (!counts) return fe_fail(f)("NULL output pointer");
    CLAIR_HIP_TRY(fe_fail(f), hipSetDevice(f->device));
    CandidateBuffers &cb = *f->cand;
    const size_t row_bytes = (size_t)WINDOW_VALUES * sizeof(int16_t);
    CLAIR_HIP_TRY(fe_fail(f), cb.ts_stage.ensure((size_t)std::min(n, TS_STAGE_ROWS) * row_bytes));
    for (int64_t at = 0; at < n; at += TS_STAGE_ROWS) {
        const int64_t m = std::min(TS_STAGE_ROWS, n - at);
        hipLaunchKernelGGL(ts_gather_kernel, dim3(blocks_for(m, 4)), dim3(256), 0, f->stream, cb.counts.as<const uint4>(), cb.ts_kept.as<const int64_t>() + first + at, m,
                           cb.ts_stage.as<uint4>());
        CLAIR_HIP_TRY(fe_fail(f), hipGetLastError());
        CLAIR_HIP_TRY(fe_fail(f), hipMemcpyAsync((uint8_t *)counts + (size_t)at * row_bytes, cb.ts_stage.p, (size_t)m * row_bytes, hipMemcpyDeviceToHost, f->stream));
        CLAIR_HIP_TRY(fe_fail(f), hipStreamSynchronize(f->stream));
    }
    return 0;
}

}  // extern "C"
