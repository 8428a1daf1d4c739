// The front of a batch on the host, for the twins that take batches of BGZF blocks (host_bam_index.cpp, host_bam_sort.cpp,
// host_markdup.cpp): HostFront, which inflates the blocks behind the carried bytes and frames the records, over the two framings:
// the sequential walk, and -- so that the parallel rule can be held against the walk on a machine without a GPU -- a restatement of the
// segmented framing the device runs (csrc/bam_index.hip: jump table per segment, pointer jumping, the chain over the segments, counts,
// offsets).  The rules themselves are csrc/bam_index_core.h.  Host only.
#pragma once
#include "../csrc/bam_index_core.h"
#include "bgzf_file.h"

#include <algorithm>
#include <cstring>
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

// the BGZF blocks of a batch: of a handle, and of the file driver that feeds it
inline int check_max_blocks(int max_blocks) {
    return max_blocks < 1 || max_blocks > 16384 ? clair_host_fail("max_blocks %d: 1 .. 16384", max_blocks) : 0;
}

// ---- the front of a batch on the host, what clair_bix::Front (csrc/bam_front.h) is on the device: the blocks of a batch inflated behind the
// bytes the batch before carried over, the records framed there, the table that turns a stream position into a virtual offset, the verdicts
// of the frame step and the carry to the next batch.  `who` names the stage in the messages ("bamsort batch").
struct HostFront {
    int threads = 4, max_blocks = 0;
    uint32_t seg = 0;                            // 0: the sequential walk
    std::vector<uint8_t> stream, carry;
    uint64_t carry_voff = 0;
    std::vector<int64_t> at, starts;
    std::vector<uint64_t> voff;
    // the batch between open_batch and close_batch
    int64_t len = 0, tail = 0;
    bool bad = false;

    // what every _create takes, checked; segment_bytes 0: the sequential walk
    int configure(int n_threads, int blocks, int segment_bytes) {
        if (n_threads < 1 || n_threads > 16) return clair_host_fail("BAM threads: %d (1 .. 16)", n_threads);
        if (check_max_blocks(blocks)) return 1;
        if (segment_bytes != 0 && !good_segment(segment_bytes)) return clair_host_fail("segment_bytes %d: a power of two in %u .. %u, or 0", segment_bytes, SEG_MIN, SEG_MAX);
        threads = n_threads;
        max_blocks = blocks;
        seg = (uint32_t)segment_bytes;
        return 0;
    }
    void rewind() { carry.clear(); carry_voff = 0; }         // a new file, or a new read of one
    uint64_t voffset(int64_t p) const { return voffset_at(at.data(), voff.data(), (int)at.size(), p); }

    int open_batch(const char *who, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                   const int64_t *coffset, int64_t end_coffset, int64_t entry) {
        if (n > 0 && (!cdata || !in_at || !csize || !out_len || !coffset)) return clair_host_fail("%s: NULL argument", who);
        if (cbytes < 0 || end_coffset < 0 || entry < 0) return clair_host_fail("%s: negative argument", who);
        if (clair_inf::check_blocks(clair_host_fail, n, max_blocks, cbytes, in_at, csize, out_len)) return 1;
        len = (int64_t)carry.size();
        for (int i = 0; i < n; ++i) {
            if (coffset[i] < 0) return clair_host_fail("block %d: negative offset", i);
            len += out_len[i];
        }
        if (entry > len) return clair_host_fail("%s: entry %lld beyond the %lld bytes of the batch", who, (long long)entry, (long long)len);
        // 1. the stream and the table of its pieces
        stream.resize((size_t)len);
        at.clear();
        voff.clear();
        if (!carry.empty()) {
            memcpy(stream.data(), carry.data(), carry.size());
            at.push_back(0);
            voff.push_back(carry_voff);
        }
        std::vector<int32_t> status((size_t)n, 0);
        int64_t pos = (int64_t)carry.size();
        const size_t first_block = at.size();
        for (int i = 0; i < n; ++i) {
            at.push_back(pos);
            voff.push_back((uint64_t)coffset[i] << 16);
            pos += out_len[i];
        }
        at.push_back(len);
        voff.push_back((uint64_t)end_coffset << 16);
        clair_bgzf::inflate_blocks(threads, cdata, n, in_at, csize, at.data() + first_block, out_len, stream.data(), status.data());
        for (int i = 0; i < n; ++i)
            if (status[(size_t)i]) return clair_host_fail("BGZF block at compressed offset %lld: %s", (long long)coffset[i], clair_bgzf::inflate_text(status[(size_t)i]));
        // 2. the record starts
        const Bytes m{stream.data()};
        starts.clear();
        tail = 0;
        bad = false;
        if (seg) frame_segmented(m, len, entry, seg, starts, &tail, &bad);
        else frame_walk(m, len, entry, starts, &tail, &bad);
        return 0;
    }
    // the verdicts of the frame step (a size word that cannot be; with `last`, bytes behind the last whole record), then the carry
    int close_batch(int last) {
        char buf[200];
        if (bad) {
            describe_bad_step(buf, sizeof buf, voffset(tail), Bytes{stream.data()}.le32(tail));
            return clair_host_fail("%s", buf);
        }
        if (last && tail < len) {
            describe_cut(buf, sizeof buf, voffset(tail));
            return clair_host_fail("%s", buf);
        }
        carry_voff = tail < len ? voffset(tail) : 0;
        std::vector<uint8_t> keep(stream.begin() + (ptrdiff_t)tail, stream.end());
        carry.swap(keep);
        return 0;
    }
};

}  // namespace clair_frame
