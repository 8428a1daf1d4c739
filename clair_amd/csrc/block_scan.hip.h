// The exclusive scan of one value per thread over a workgroup of 256: what the front end's scans (frontend.hip) and the site table's
// (sites.hip.h) are built on.  Shuffles inside the four waves, four wave sums through LDS.
#pragma once
#include <hip/hip_runtime.h>

template <typename T> __device__ inline T block_exclusive_scan(T v, T *total) {   // 256 threads
    __shared__ T wave_sum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_sum[w] = x;
    __syncthreads();
    T before = 0, all = 0;
    for (int i = 0; i < 4; ++i) { if (i < w) before += wave_sum[i]; all += wave_sum[i]; }
    __syncthreads();
    *total = all;
    return before + x - v;
}
