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
// 1. M and R: a segmented max-scan (cut at the contig changes), block scan as in frontend.hip -- block totals, one workgroup over the
//    totals, then every workgroup writes its head flags.   2. the heads compacted into a list, the same three steps with a sum.
// 3. one lane per head walks to the next head with clair_overlap_walk and writes keep (plain byte stores).
#include "../../include/clair_amd.h"

#include <hip/hip_runtime.h>

#include "device_buffer.h"
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

struct CountScan {
    using T = uint32_t;
    const uint8_t *head;
    static __device__ inline T identity() { return 0; }
    static __device__ inline T join(T a, T b) { return a + b; }
    static __device__ inline T up(T x, int d) { return __shfl_up(x, d, 64); }
    __device__ inline T item(int64_t i) const { return head[i] != 0; }
};

// 256 threads, v in thread order: -> the join of the values of the threads before this one; *total = the join of all 256
template <typename P> __device__ inline typename P::T block_exclusive(typename P::T v, typename P::T *total) {
    using T = typename P::T;
    __shared__ T wave_total[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T y = P::up(x, d);
        if (lane >= d) x = P::join(y, x);
    }
    if (lane == 63) wave_total[w] = x;
    T ex = P::up(x, 1);
    if (lane == 0) ex = P::identity();
    __syncthreads();
    T before = P::identity(), all = P::identity();
    for (int i = 0; i < 4; ++i) { if (i < w) before = P::join(before, wave_total[i]); all = P::join(all, wave_total[i]); }
    __syncthreads();
    *total = all;
    return P::join(before, ex);
}

template <typename P> __global__ __launch_bounds__(256) void ov_block_totals_kernel(P p, int64_t n, typename P::T *block_total) {
    const int64_t at = (int64_t)blockIdx.x * BLOCK + (int64_t)threadIdx.x * ITEMS;
    typename P::T c = P::identity(), total;
    for (int i = 0; i < ITEMS; ++i) if (at + i < n) c = P::join(c, p.item(at + i));
    (void)block_exclusive<P>(c, &total);
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

// one workgroup: block_total[0 .. nb) -> in place, what the blocks before each leave; block_total[nb] = the join of all
template <typename P> __global__ __launch_bounds__(256) void ov_block_prefix_kernel(typename P::T *block_total, int64_t nb) {
    typename P::T carry = P::identity(), total;
    for (int64_t at = 0; at < nb; at += 256) {
        const int64_t i = at + threadIdx.x;
        const typename P::T x = i < nb ? block_total[i] : P::identity();
        const typename P::T ex = block_exclusive<P>(x, &total);
        if (i < nb) block_total[i] = P::join(carry, ex);
        carry = P::join(carry, total);
    }
    if (threadIdx.x == 0) block_total[nb] = carry;
}

// what is written for row i, `before` the join of the rows before it
struct WriteHeads {
    uint8_t *head;
    __device__ inline void write(const ReachScan &p, int64_t i, const Reach &before) const {
        const clair_overlap_span v = p.s[i];
        head[i] = p.starts_run(i) || (v.pos >= before.m && (!clair_overlap_body(v) || v.pos > before.r));
    }
};
struct WriteSegments {
    int64_t *first;      // first[k] = the row head k is
    __device__ inline void write(const CountScan &p, int64_t i, uint32_t before) const {
        if (p.head[i]) first[before] = i;
    }
};

template <typename P, typename W>
__global__ __launch_bounds__(256) void ov_write_kernel(P p, int64_t n, const typename P::T *block_prefix, W w) {
    const int64_t at = (int64_t)blockIdx.x * BLOCK + (int64_t)threadIdx.x * ITEMS;
    typename P::T f[ITEMS];
    typename P::T c = P::identity(), total;
    for (int i = 0; i < ITEMS; ++i) { f[i] = at + i < n ? p.item(at + i) : P::identity(); c = P::join(c, f[i]); }
    typename P::T run = P::join(block_prefix[blockIdx.x], block_exclusive<P>(c, &total));
    for (int i = 0; i < ITEMS; ++i) {
        if (at + i >= n) break;
        w.write(p, at + i, run);
        run = P::join(run, f[i]);
    }
}

// one lane per head: rows [first[k], first[k + 1]) (the last: up to n)
__global__ __launch_bounds__(256) void ov_walk_kernel(const clair_overlap_span *s, int64_t n, const int64_t *first, int64_t n_heads, uint8_t *keep) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= n_heads) return;
    clair_overlap_walk(s, first[k], k + 1 < n_heads ? first[k + 1] : n, keep);
}

}  // namespace clair_ov

#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>

namespace {

std::string g_ov_error;
std::mutex g_ov_mutex;      // one call at a time: the message is per process

int ov_fail(const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_ov_error = buf;
    return 1;
}

#define OV_TRY(call)                                                                                      \
    do {                                                                                                  \
        hipError_t err__ = (call);                                                                        \
        if (err__ != hipSuccess)                                                                          \
            return ov_fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(err__), __FILE__, __LINE__); \
    } while (0)

}  // namespace

extern "C" {

const char *clair_overlap_last_error(void) { return g_ov_error.c_str(); }

int clair_overlap_keep(int device, const clair_overlap_span_t *spans, int64_t n, uint8_t *keep) {
    using namespace clair_ov;
    std::lock_guard<std::mutex> lock(g_ov_mutex);
    if (n < 0 || n > INT32_MAX) return ov_fail("%lld rows: 0 .. 2^31 - 1", (long long)n);
    if (n > 0 && (!spans || !keep)) return ov_fail("NULL argument");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev < 1)
        return ov_fail("no HIP device is visible: the device overlap filter runs on an MI355X only (the host twin is --overlap_filter host)");
    if (device < 0 || device >= n_dev) return ov_fail("device %d out of range [0,%d)", device, n_dev);
    if (n == 0) return 0;
    OV_TRY(hipSetDevice(device));

    const int64_t nb = (n + BLOCK - 1) / BLOCK;
    DeviceBuffer d_spans, d_reach, d_count, d_head, d_first, d_keep;
    OV_TRY(d_spans.ensure((size_t)n * sizeof(clair_overlap_span)));
    OV_TRY(d_reach.ensure((size_t)(nb + 1) * sizeof(Reach)));
    OV_TRY(d_count.ensure((size_t)(nb + 1) * sizeof(uint32_t)));
    OV_TRY(d_head.ensure((size_t)n));
    OV_TRY(d_first.ensure((size_t)n * sizeof(int64_t)));
    OV_TRY(d_keep.ensure((size_t)n));
    OV_TRY(hipMemcpy(d_spans.p, spans, (size_t)n * sizeof(clair_overlap_span), hipMemcpyHostToDevice));
    OV_TRY(hipMemsetAsync(d_keep.p, 0, (size_t)n, nullptr));

    const ReachScan reach{d_spans.as<clair_overlap_span>()};
    hipLaunchKernelGGL(ov_block_totals_kernel<ReachScan>, dim3((unsigned)nb), dim3(256), 0, nullptr, reach, n, d_reach.as<Reach>());
    hipLaunchKernelGGL(ov_block_prefix_kernel<ReachScan>, dim3(1), dim3(256), 0, nullptr, d_reach.as<Reach>(), nb);
    hipLaunchKernelGGL((ov_write_kernel<ReachScan, WriteHeads>), dim3((unsigned)nb), dim3(256), 0, nullptr, reach, n, (const Reach *)d_reach.as<Reach>(),
                       WriteHeads{d_head.as<uint8_t>()});
    const CountScan count{d_head.as<uint8_t>()};
    hipLaunchKernelGGL(ov_block_totals_kernel<CountScan>, dim3((unsigned)nb), dim3(256), 0, nullptr, count, n, d_count.as<uint32_t>());
    hipLaunchKernelGGL(ov_block_prefix_kernel<CountScan>, dim3(1), dim3(256), 0, nullptr, d_count.as<uint32_t>(), nb);
    hipLaunchKernelGGL((ov_write_kernel<CountScan, WriteSegments>), dim3((unsigned)nb), dim3(256), 0, nullptr, count, n, (const uint32_t *)d_count.as<uint32_t>(),
                       WriteSegments{d_first.as<int64_t>()});
    OV_TRY(hipGetLastError());
    uint32_t n_heads = 0;
    OV_TRY(hipMemcpy(&n_heads, d_count.as<uint32_t>() + nb, sizeof n_heads, hipMemcpyDeviceToHost));
    if (n_heads < 1 || (int64_t)n_heads > n) return ov_fail("%u heads among %lld rows: the head scan is broken", n_heads, (long long)n);
    hipLaunchKernelGGL(ov_walk_kernel, dim3((n_heads + 255) / 256), dim3(256), 0, nullptr, (const clair_overlap_span *)d_spans.as<clair_overlap_span>(), n,
                       (const int64_t *)d_first.as<int64_t>(), (int64_t)n_heads, d_keep.as<uint8_t>());
    OV_TRY(hipGetLastError());
    OV_TRY(hipMemcpy(keep, d_keep.p, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
