// Batch accuracy of a training micro-batch, counted where the probabilities and the labels already lie (csrc/train.hip:
// clair_train_accuracy; docs/train_clr.md).
//
// The rule is the learning-rate finder's (clair/learning_rate_finder.py:21-73): per row the arg-max of each head against the true index;
// the two indel-length heads as SORTED pairs -- (label 1, label 2) ascending against (arg-max 1, arg-max 2) ascending, the smaller elements
// compared for tp[2], the larger for tp[3].  Arg-max is the LOWEST index among equal values (np.argmax), the rule of csrc/evaluate.hip.h.
// NaN probabilities are out of scope, as there (every comparison with them is false).
//
// Shape.  One thread per row, 256 rows per workgroup: a row is 90 floats and 4 label bytes, a micro-batch at most 4096 rows, so this is a
// latency kernel, not a throughput one.  Each head's hits are counted over the workgroup (__syncthreads_count) and added to the four
// 64-bit counters with one integer atomic per head and workgroup: integers only, so the counts depend neither on the grid nor on the order
// the workgroups finish in.  The caller zeroes tp first.
//
// Twin: clair_amd.model.accuracy_counts (NumPy), the same rule.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace clair_train {

__device__ inline int argmax_lowest(const float *p, int size) {
    int best = 0;
    float top = p[0];
    for (int c = 1; c < size; ++c)
        if (p[c] > top) { top = p[c]; best = c; }
    return best;
}

// probs [n][90] (gt21 21 | genotype 3 | len1 33 | len2 33), labels [n][4] true indices, tp [4] zeroed by the caller
__global__ __launch_bounds__(256) void accuracy_kernel(const float *probs, const uint8_t *labels, int n, unsigned long long *tp) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int hit[4] = {0, 0, 0, 0};
    if (row < n) {                                   // no early return: every thread of the workgroup takes part in the counts below
        const float *p = probs + row * 90;
        const uint8_t *y = labels + row * 4;
        hit[0] = argmax_lowest(p, 21) == y[0];
        hit[1] = argmax_lowest(p + 21, 3) == y[1];
        const int a = argmax_lowest(p + 24, 33), b = argmax_lowest(p + 57, 33);
        hit[2] = min(a, b) == min((int)y[2], (int)y[3]);
        hit[3] = max(a, b) == max((int)y[2], (int)y[3]);
    }
    for (int k = 0; k < 4; ++k) {
        const int count = __syncthreads_count(hit[k]);
        if (threadIdx.x == 0 && count) atomicAdd(tp + k, (unsigned long long)count);
    }
}

}  // namespace clair_train
