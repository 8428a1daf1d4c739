// Framing a stream of BAM records on the host, for the twins that take batches of inflated blocks (host_bam_index.cpp, host_bam_sort.cpp):
// the sequential walk, and -- so that the parallel rule can be held against the walk on a machine without a GPU -- a restatement of the
// segmented framing the device runs (csrc/bam_index.hip: jump table per segment, pointer jumping, the chain over the segments, counts,
// offsets).  The rules themselves are csrc/bam_index_core.h.  Host only.
#pragma once
#include "../csrc/bam_index_core.h"

#include <algorithm>
#include <vector>

namespace clair_frame {

using namespace clair_bix;

// ---- framing.  Both give the record starts from `entry`, the tail (where the chain stops) and whether it stopped on a bad step.
inline void frame_walk(const Bytes &m, int64_t len, int64_t entry, std::vector<int64_t> &starts, int64_t *tail, bool *bad) {
    int64_t o = entry, next = 0;
    int rc;
    while ((rc = step(m, o, len, &next)) == STEP_NEXT) { starts.push_back(o); o = next; }
    *tail = o;
    *bad = rc == STEP_BAD;
}

// the device's rule, restated: what each kernel of csrc/bam_index.hip does, a loop per kernel
inline void frame_segmented(const Bytes &m, int64_t len, int64_t entry, uint32_t seg, std::vector<int64_t> &starts, int64_t *tail, bool *bad) {
    const int64_t n_seg = (len + seg - 1) / seg;
    std::vector<uint32_t> exit((size_t)(n_seg * seg)), now(seg);
    const int rounds = jump_rounds(seg);
    for (int64_t s = 0; s < n_seg; ++s) {                    // exits_kernel: a workgroup per segment
        uint32_t *e = exit.data() + s * seg;
        for (uint32_t o = 0; o < seg; ++o) e[o] = seg_next(m, s * (int64_t)seg, o, len);
        for (int r = 0; r < rounds; ++r) {
            for (uint32_t o = 0; o < seg; ++o) now[o] = e[o] < seg ? e[e[o]] : e[o];     // every lane reads, a barrier, every lane writes
            std::copy(now.begin(), now.end(), e);
        }
    }
    std::vector<int64_t> seg_entry((size_t)n_seg), first((size_t)n_seg + 1, 0);
    int64_t result[2];
    chain_walk(m, len, entry, seg, n_seg, exit.data(), seg_entry.data(), result);        // chain_kernel: one thread
    for (int64_t s = 0; s < n_seg; ++s)                      // count_kernel and the scan
        first[(size_t)s + 1] = first[(size_t)s] + (seg_entry[(size_t)s] < 0 ? 0 : seg_records(m, len, seg, s, seg_entry[(size_t)s], nullptr, 0, 0));
    const size_t before = starts.size();
    starts.resize(before + (size_t)first[(size_t)n_seg]);
    for (int64_t s = 0; s < n_seg; ++s)                      // emit_kernel
        if (seg_entry[(size_t)s] >= 0) seg_records(m, len, seg, s, seg_entry[(size_t)s], starts.data() + before, first[(size_t)s], first[(size_t)n_seg]);
    *tail = result[0];
    *bad = result[1] != 0;
}

inline bool good_segment(int segment_bytes) {
    return segment_bytes >= (int)SEG_MIN && segment_bytes <= (int)SEG_MAX && (segment_bytes & (segment_bytes - 1)) == 0;
}

}  // namespace clair_frame
