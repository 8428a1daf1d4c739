// clair_overlap_keep: the overlap filter's walk on the device (include/clair_amd.h).  The pair rule and the sequential walk are
// csrc/overlap_core.h, shared with the host twin (hostsrc/host_overlap.cpp); this file finds where the walk may be cut and runs the
// pieces side by side.  It is a translation unit of its own, outside the forward pass's sources (build.csrc_digest).
//
// The walk keeps one row L, the last it kept, and compares every row with L alone.  After row i - 1, L lies in the contig run of
// row i - 1 (a row that starts a run cannot overlap an L of another contig, so it is kept and becomes L).  Row i is a HEAD when no row of
// its run before it can overlap it, whichever of them L is:
//     i == 0, or ctg[i] != ctg[i - 1], or  pos[i] >= M[i] and (not body[i] or pos[i] > R[i])
// with M[i] the largest pos and R[i] the largest pos + del over the rows with del > 0, both over the rows of the run before i.  (pos[i] >= M[i]:
// every earlier row is the lower one of the pair, so only ITS deletion counts; then body[i] and pos[i] <= pos[j] + del[j] for some j is
// what an overlap needs.)  A head is kept whatever came before, and everything before it is final: the stretches between heads are
// independent walks.  A row out of position order simply is no head, which costs parallelism and never correctness.
//
// 1. M and R: a segmented max-scan (cut at the contig changes) with the scan of device_scan.h -- block totals, one workgroup over the
//    totals, then every workgroup writes its head flags.   2. the heads compacted into a list, the same three steps with a sum.
// 3. one lane per head walks to the next head with clair_overlap_walk and writes keep (plain byte stores).
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>

#include "device_buffer.h"
#include "device_scan.h"
#include "hip_status.h"
#include "overlap_core.h"

static_assert(sizeof(clair_overlap_span) == 24, "span record layout");

namespace clair_ov {

constexpr int ITEMS = 8, BLOCK = 256 * ITEMS;      // rows per thread and per workgroup of a scan (clair_amd/_capi.py OVERLAP_SCAN_BLOCK)
constexpr int64_t NONE = INT64_MIN;

// what the rows of a range leave for the rows after it: the maxima since the last contig change inside the range
struct Reach {
    long long m, r;      // largest pos; largest pos + del of a row with del > 0 (NONE: no such row)
    int cut;             // a contig run starts inside the range: what came before the range does not pass through it
};

struct ReachScan {
    using T = Reach;
    const clair_overlap_span *s;
    static __device__ inline T identity() { return Reach{NONE, NONE, 0}; }
    static __device__ inline T join(const T &a, const T &b) {          // a: the earlier range
        if (b.cut) return b;
        return Reach{a.m > b.m ? a.m : b.m, a.r > b.r ? a.r : b.r, a.cut};
    }
    static __device__ inline T up(const T &x, int d) { return Reach{__shfl_up(x.m, d, 64), __shfl_up(x.r, d, 64), __shfl_up(x.cut, d, 64)}; }
    __device__ inline bool starts_run(int64_t i) const { return i == 0 || s[i].ctg != s[i - 1].ctg; }
    __device__ inline T item(int64_t i) const {
        const clair_overlap_span v = s[i];
        return Reach{v.pos, v.del > 0 ? clair_overlap_reach(v) : NONE, starts_run(i) ? 1 : 0};
    }
};

using CountScan = clair_scan::FlagScan<false>;      // over the head flags

// what is written for row i, `before` the join of the rows before it
struct WriteHeads {
    static constexpr int PAST_END = 0;
    uint8_t *head;
    static __device__ inline Reach seed() { return ReachScan::identity(); }
    __device__ inline void write(const ReachScan &p, int64_t i, int64_t, const Reach &before, const Reach &) const {
        const clair_overlap_span v = p.s[i];
        head[i] = p.starts_run(i) || (v.pos >= before.m && (!clair_overlap_body(v) || v.pos > before.r));
    }
};
struct WriteSegments {
    static constexpr int PAST_END = 0;
    int64_t *first;      // first[k] = the row head k is
    static __device__ inline uint32_t seed() { return 0; }
    __device__ inline void write(const CountScan &, int64_t i, int64_t, uint32_t before, uint32_t is_head) const {
        if (is_head) first[before] = i;
    }
};

// one lane per head: rows [first[k], first[k + 1]) (the last: up to n)
__global__ __launch_bounds__(256) void ov_walk_kernel(const clair_overlap_span *s, int64_t n, const int64_t *first, int64_t n_heads, uint8_t *keep) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_heads) return;
    clair_overlap_walk(s, first[k], k + 1 < n_heads ? first[k + 1] : n, keep);
}

}  // namespace clair_ov

#include <mutex>

namespace {

std::string g_ov_error;
std::mutex g_ov_mutex;      // one call at a time: the message is per process
const HipFail ov_fail{g_ov_error};

}  // namespace

extern "C" {

const char *clair_overlap_last_error(void) { return g_ov_error.c_str(); }

int clair_overlap_keep(int device, const clair_overlap_span_t *spans, int64_t n, uint8_t *keep) {
    using namespace clair_ov;
    std::lock_guard<std::mutex> lock(g_ov_mutex);
    if (n < 0 || n > INT32_MAX) return ov_fail("%lld rows: 0 .. 2^31 - 1", (long long)n);
    if (n > 0 && (!spans || !keep)) return ov_fail("NULL argument");
    if (hip_device_check(ov_fail, device, "the device overlap filter runs on an MI355X only (the host twin is --overlap_filter host)")) return 1;
    if (n == 0) return 0;
    CLAIR_HIP_TRY(ov_fail, hipSetDevice(device));

    const int64_t nb = (n + BLOCK - 1) / BLOCK;
    DeviceBuffer d_spans, d_reach, d_count, d_head, d_first, d_keep;
    CLAIR_HIP_TRY(ov_fail, d_spans.ensure((size_t)n * sizeof(clair_overlap_span)));
    CLAIR_HIP_TRY(ov_fail, d_reach.ensure((size_t)(nb + 1) * sizeof(Reach)));
    CLAIR_HIP_TRY(ov_fail, d_count.ensure((size_t)(nb + 1) * sizeof(uint32_t)));
    CLAIR_HIP_TRY(ov_fail, d_head.ensure((size_t)n));
    CLAIR_HIP_TRY(ov_fail, d_first.ensure((size_t)n * sizeof(int64_t)));
    CLAIR_HIP_TRY(ov_fail, d_keep.ensure((size_t)n));
    CLAIR_HIP_TRY(ov_fail, hipMemcpy(d_spans.p, spans, (size_t)n * sizeof(clair_overlap_span), hipMemcpyHostToDevice));
    CLAIR_HIP_TRY(ov_fail, hipMemsetAsync(d_keep.p, 0, (size_t)n, nullptr));

    using clair_scan::totals_kernel; using clair_scan::walk_kernel; using clair_scan::write_kernel;
    const ReachScan reach{d_spans.as<clair_overlap_span>()};
    const clair_scan::Stored<ReachScan> reach_totals{reach, d_reach.as<Reach>()};
    hipLaunchKernelGGL((totals_kernel<ReachScan, ITEMS>), dim3((unsigned)nb), dim3(256), 0, nullptr, reach, n, d_reach.as<Reach>());
    hipLaunchKernelGGL((walk_kernel<clair_scan::Stored<ReachScan>, false>), dim3(1), dim3(256), 0, nullptr, reach_totals, nb, d_reach.as<Reach>(), d_reach.as<Reach>() + nb);
    hipLaunchKernelGGL((write_kernel<ReachScan, ITEMS, WriteHeads>), dim3((unsigned)nb), dim3(256), 0, nullptr, reach, n, (const Reach *)d_reach.as<Reach>(),
                       WriteHeads{d_head.as<uint8_t>()});
    const CountScan count{{d_head.as<uint8_t>()}};
    const clair_scan::SumScan<uint32_t, uint32_t> count_totals{d_count.as<uint32_t>()};
    hipLaunchKernelGGL((totals_kernel<CountScan, ITEMS>), dim3((unsigned)nb), dim3(256), 0, nullptr, count, n, d_count.as<uint32_t>());
    hipLaunchKernelGGL((walk_kernel<clair_scan::SumScan<uint32_t, uint32_t>, false>), dim3(1), dim3(256), 0, nullptr, count_totals, nb, d_count.as<uint32_t>(),
                       d_count.as<uint32_t>() + nb);
    hipLaunchKernelGGL((write_kernel<CountScan, ITEMS, WriteSegments>), dim3((unsigned)nb), dim3(256), 0, nullptr, count, n, (const uint32_t *)d_count.as<uint32_t>(),
                       WriteSegments{d_first.as<int64_t>()});
    CLAIR_HIP_TRY(ov_fail, hipGetLastError());
    uint32_t n_heads = 0;
    CLAIR_HIP_TRY(ov_fail, hipMemcpy(&n_heads, d_count.as<uint32_t>() + nb, sizeof n_heads, hipMemcpyDeviceToHost));
    if (n_heads < 1 || (int64_t)n_heads > n) return ov_fail("%u heads among %lld rows: the head scan is broken", n_heads, (long long)n);
    hipLaunchKernelGGL(ov_walk_kernel, dim3((n_heads + 255) / 256), dim3(256), 0, nullptr, (const clair_overlap_span *)d_spans.as<clair_overlap_span>(), n,
                       (const int64_t *)d_first.as<int64_t>(), (int64_t)n_heads, d_keep.as<uint8_t>());
    CLAIR_HIP_TRY(ov_fail, hipGetLastError());
    CLAIR_HIP_TRY(ov_fail, hipMemcpy(keep, d_keep.p, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
