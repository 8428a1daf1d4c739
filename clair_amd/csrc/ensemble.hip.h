// Ensemble calling on the device: the probabilities of K checkpoints over one batch, averaged where they already are.
//
// The reference averages models through text: K runs of call_var --output_for_ensemble (clair/call_var.py:950-1000), the filter
// clair/post_processing/ensemble.py:10-75, then call_var --input_probabilities (:1276-1309) -- 3 KB of text per candidate and model.
// Here the K forward passes of a slot run back to back on the slot's lane over the same input, and ensemble_kernel follows each of
// them on the [n][90] rows tail_kernel has just left in HBM: the first pass stores the re-read values into the slot's accumulator
// (double [max_pad][90]), later passes add theirs, the last one divides, rounds to six decimals and writes the float32 rows back in
// place, where decode_kernel and the result copy read.  The order of the additions is the order of the passes on the stream: no
// atomics, and the same bits on every run.  The arithmetic is csrc/ensemble_core.h, the text round trip value for value.
//
// Shape.  Element-wise and tiny beside a forward pass (92 160 values for a batch of 1 024): a thread takes two neighbouring values,
// one 8-byte load of the row and one 16-byte access of the accumulator, both coalesced.  n * 90 is even for every n.
//
// Twin: clair_host_ensemble_average (hostsrc/host_ensemble.cpp), the same header compiled by the host compiler.
#pragma once
#include "common.hip.h"
#include "ensemble_core.h"

namespace clair {

static_assert(OUT_FLOATS % 2 == 0, "ensemble_kernel takes the values of a batch in pairs");

struct EnsembleArgs {
    float *rows;        // [n][90] probabilities of the pass that has just run; the averaged rows when `last`
    double *acc;        // [n][90] running sums of the re-read values
    int n_pairs;        // n * 90 / 2
    int models;         // K: what the last pass divides by
    int first, last;    // this is the first / the last of the K passes (both for K = 1)
};

__global__ __launch_bounds__(256) void ensemble_kernel(EnsembleArgs p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n_pairs) return;
    const float2 v = ((const float2 *)p.rows)[i];
    double2 s = {clair_ens_reread(v.x), clair_ens_reread(v.y)};
    if (!p.first) {
        const double2 a = ((const double2 *)p.acc)[i];
        s.x = a.x + s.x;
        s.y = a.y + s.y;
    }
    if (p.last) ((float2 *)p.rows)[i] = float2{clair_ens_finish(s.x, p.models), clair_ens_finish(s.y, p.models)};
    else ((double2 *)p.acc)[i] = s;
}

}  // namespace clair
