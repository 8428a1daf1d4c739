// The device-wide scan of the stages outside the forward pass (frontend.hip, train_set.hip, overlap.hip): totals of 256 x ITEMS items per
// workgroup, one workgroup that walks the totals, then every workgroup writes.  Three launches; the caller picks ITEMS and the grids.
//
// A policy P says what is scanned: P::T the running value, identity(), join(earlier, later) (associative; need not commute), up(x, d) the
// wave shuffle of a T, and item(i), the value of item i.  Sums are a policy (SumScan, FlagScan below); overlap.hip has a segmented maximum.
// A writer W says what becomes of it: seed() is joined in front of everything, write(p, i, n, before, item) gets the join of the seed and
// the items before i, and W::PAST_END = 1 has the thread that owns index n write too (item = identity, `before` = the total).
// (The site table of engine.hip has a one-workgroup scan of its own on block_scan.hip.h: sites.hip.h.)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace clair_scan {

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

// block_total[b] = the join of the items of workgroup b
template <typename P, int ITEMS> __global__ __launch_bounds__(256) void totals_kernel(P p, int64_t n, typename P::T *block_total) {
    const int64_t at = (int64_t)blockIdx.x * (256 * ITEMS) + (int64_t)threadIdx.x * ITEMS;
    typename P::T c = P::identity(), total;
    for (int i = 0; i < ITEMS; ++i) if (at + i < n) c = P::join(c, p.item(at + i));
    (void)block_exclusive<P>(c, &total);
    if (threadIdx.x == 0) block_total[blockIdx.x] = total;
}

// one workgroup walks n items 256 at a time: out[i] = the join of the items before i (INCLUSIVE: and of item i), in place where out is
// what p reads; *grand_total (unless NULL) = the join of all
template <typename P, bool INCLUSIVE> __global__ __launch_bounds__(256) void walk_kernel(P p, int64_t n, typename P::T *out, typename P::T *grand_total) {
    typename P::T carry = P::identity(), total;
    for (int64_t at = 0; at < n; at += 256) {
        const int64_t i = at + threadIdx.x;
        const typename P::T x = i < n ? p.item(i) : P::identity();
        const typename P::T ex = P::join(carry, block_exclusive<P>(x, &total));
        if (i < n) out[i] = INCLUSIVE ? P::join(ex, x) : ex;
        carry = P::join(carry, total);
    }
    if (grand_total && threadIdx.x == 0) *grand_total = carry;
}

// after the walk over the totals (block_prefix[b] = the join of the workgroups before b): every item is written
template <typename P, int ITEMS, typename W>
__global__ __launch_bounds__(256) void write_kernel(P p, int64_t n, const typename P::T *block_prefix, W w) {
    const int64_t at = (int64_t)blockIdx.x * (256 * ITEMS) + (int64_t)threadIdx.x * ITEMS;
    typename P::T f[ITEMS];
    typename P::T c = P::identity(), total;
    for (int i = 0; i < ITEMS; ++i) { f[i] = at + i < n ? p.item(at + i) : P::identity(); c = P::join(c, f[i]); }
    typename P::T run = P::join(P::join(w.seed(), block_prefix[blockIdx.x]), block_exclusive<P>(c, &total));
    for (int i = 0; i < ITEMS; ++i) {
        if (at + i >= n + W::PAST_END) break;
        w.write(p, at + i, n, run, f[i]);
        run = P::join(run, f[i]);
    }
}

// sums: an In widened to the Sum the scan runs in (signed sums in two's complement) ...
template <typename In, typename Sum> struct SumScan {
    using T = Sum;
    const In *v;
    static __device__ inline T identity() { return 0; }
    static __device__ inline T join(T a, T b) { return a + b; }
    static __device__ inline T up(T x, int d) { return __shfl_up(x, d, 64); }
    __device__ inline T item(int64_t i) const { return (T)v[i]; }
};
// ... or a byte that counts one when it is set (NEWLINES: the bytes are text and a line feed is a set flag)
template <bool NEWLINES> struct FlagScan : SumScan<uint8_t, uint32_t> {
    __device__ inline T item(int64_t i) const { return NEWLINES ? v[i] == '\n' : v[i] != 0; }
};
// the values of a scan under P, stored: what the walk over the block totals reads
template <typename P> struct Stored : P {
    const typename P::T *stored;
    __device__ inline typename P::T item(int64_t i) const { return stored[i]; }
};

}  // namespace clair_scan
