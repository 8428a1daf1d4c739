// Device scoring: probabilities + truth labels -> confusion counters, where the probabilities already are.
//
// The reference scores a checkpoint against labelled tensors in clair/evaluate.py:87-129 (evaluate_model): per candidate it
// adds one to a cell of four confusion matrices (gt21 21x21, genotype 3x3, the two indel lengths 33x33 each) and keeps three
// counters (all, top-1, top-2 on the gt21 head).  eval_kernel does the same on the [n][90] rows tail_kernel leaves in HBM, so
// that in evaluation mode nothing but the counter block (CLAIR_EVAL_COUNTS int64, include/clair_amd.h) ever crosses the host link.
//
// Shape.  A workgroup of 256 threads takes EVAL_CAND = 64 candidates: their 5 760 floats come in with coalesced loads into LDS,
// thread t then scans head t & 3 of candidate t >> 2 (21, 3, 33 or 33 floats), the increments go to a workgroup histogram in LDS
// with LDS atomics, and the non-zero bins are added to the global block with one 64-bit integer atomic each.  Counts only: the
// block does not depend on lane, workgroup or launch order, nor on how many lanes of the engine run at once.
//
// Ties.  arg-max is the LOWEST index among equal values (np.argmax, evaluate.py:92-93, :109, :118-121).  For top-1 / top-2 the
// reference takes argsort()[::-1] (:97), whose order among exactly equal float32 values is an accident of NumPy's sort; this
// build defines it as descending probability, then DESCENDING index (a stable ascending sort, reversed): the true class t is
// "first" when no class j has p[j] > p[t] or (p[j] == p[t] and j > t), "first or second" when at most one has.  Real softmax rows
// do not tie; tests/test_evaluate*.py pin the rule on crafted rows.  NaN probabilities are out of scope (every comparison with
// them is false here; the reference's order is undefined there).
//
// Twin: clair_amd.evaluate.evaluate_counts_host (NumPy), same counter layout, same tie rule.
#pragma once
#include "common.hip.h"

namespace clair {

constexpr int EVAL_CAND = 64;                               // candidates per workgroup
constexpr int EVAL_ALL = 0, EVAL_TOP1 = 1, EVAL_TOP2 = 2;   // counter block: all, top1, top2, then the matrices row-major [true][pred]
constexpr int EVAL_GT21 = 3, EVAL_GENOTYPE = EVAL_GT21 + 21 * 21, EVAL_LEN1 = EVAL_GENOTYPE + 3 * 3, EVAL_LEN2 = EVAL_LEN1 + 33 * 33;
constexpr int EVAL_COUNTS = EVAL_LEN2 + 33 * 33;            // 2631 = CLAIR_EVAL_COUNTS

struct EvalArgs {
    const float *probs;               // [n][90]  gt21 (21) | genotype (3) | len1 (33) | len2 (33)
    const unsigned char *labels;      // [n][4]   true indices: gt21 0..20, genotype 0..2, len1 0..32, len2 0..32 (checked on the host)
    unsigned long long *counts;       // [EVAL_COUNTS]
    int n;
};

__global__ __launch_bounds__(256) void eval_kernel(EvalArgs p) {
    __shared__ float rows[EVAL_CAND * OUT_FLOATS];
    __shared__ unsigned hist[EVAL_COUNTS];
    __shared__ unsigned char len_pred[EVAL_CAND][2];
    const int first = blockIdx.x * EVAL_CAND;
    const int m = min(EVAL_CAND, p.n - first);               // candidates of this workgroup (>= 1: the grid is ceil(n / EVAL_CAND))
    for (int i = threadIdx.x; i < EVAL_COUNTS; i += 256) hist[i] = 0;
    {
        const float *src = p.probs + (size_t)first * OUT_FLOATS;
        for (int i = threadIdx.x; i < m * OUT_FLOATS; i += 256) rows[i] = src[i];
    }
    __syncthreads();
    const int c = threadIdx.x >> 2, head = threadIdx.x & 3;
    const bool active = c < m;
    unsigned char lab[4] = {0, 0, 0, 0};
    if (active) {
        const uchar4 l = ((const uchar4 *)p.labels)[first + c];
        lab[0] = l.x; lab[1] = l.y; lab[2] = l.z; lab[3] = l.w;
    }
    // the host refuses labels out of range before anything is enqueued; a candidate that had one would be left out, never counted out of bounds
    const bool in_range = lab[0] < 21 && lab[1] < 3 && lab[2] < 33 && lab[3] < 33;
    if (active && in_range) {
        const int offset = head == 0 ? 0 : head == 1 ? 21 : head == 2 ? 24 : 57;
        const int width = head == 0 ? 21 : head == 1 ? 3 : 33;
        const float *v = rows + c * OUT_FLOATS + offset;
        int best = 0;
        float bv = v[0];
        for (int j = 1; j < width; ++j)
            if (v[j] > bv) { bv = v[j]; best = j; }
        if (head == 0) {
            const int t = lab[0];
            const float pt = v[t];
            int ahead = 0;                                   // classes in front of the true one: larger, or equal with a larger index
            for (int j = 0; j < 21; ++j) ahead += (v[j] > pt || (v[j] == pt && j > t)) ? 1 : 0;
            atomicAdd(&hist[EVAL_GT21 + t * 21 + best], 1u);
            atomicAdd(&hist[EVAL_ALL], 1u);
            if (ahead == 0) atomicAdd(&hist[EVAL_TOP1], 1u);
            if (ahead <= 1) atomicAdd(&hist[EVAL_TOP2], 1u);
        } else if (head == 1) {
            atomicAdd(&hist[EVAL_GENOTYPE + lab[1] * 3 + best], 1u);
        } else {
            len_pred[c][head - 2] = (unsigned char)best;
        }
    }
    __syncthreads();
    if (active && in_range && head == 2) {                   // both pairs in ascending order first (evaluate.py:123-126)
        const int la = lab[2], lb = lab[3], a = len_pred[c][0], b = len_pred[c][1];
        const int t1 = min(la, lb), t2 = max(la, lb);
        atomicAdd(&hist[EVAL_LEN1 + t1 * 33 + min(a, b)], 1u);
        atomicAdd(&hist[EVAL_LEN2 + t2 * 33 + max(a, b)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < EVAL_COUNTS; i += 256) {
        const unsigned h = hist[i];
        if (h) atomicAdd(&p.counts[i], (unsigned long long)h);
    }
}

}  // namespace clair
