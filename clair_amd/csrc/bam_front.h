// The front of a batch for the stages that work on BAM records where they lie on the device (bam_index.hip, bam_sort.hip, markdup.hip), and
// what their handles start from (StageHandle: the device, the stream, the message, the front).  The front: the raw BGZF
// blocks of a batch inflated (inflate_bgzf_kernel) behind the bytes the batch before carried over, into a stream that stays on the device;
// the records framed there (exits_kernel, chain_kernel, count_kernel, the scan, emit_kernel: bam_index.hip, which defines what is declared
// here); the table that turns a stream position into a virtual offset; the verdicts of the frame step and the carry to the next batch.
// Host side only; every launch goes to the owner's stream, every message through the owner's HipFail.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "bam_index_core.h"
#include "device_buffer.h"
#include "hip_status.h"

namespace clair_bix {

constexpr int64_t PAD = 16;                      // behind the stream and the offsets array: room the kernels must leave alone

// at least n bytes, grown by half when it has to grow: a record longer than a batch makes the stream longer batch by batch
hipError_t at_least(DeviceBuffer &b, size_t n);

struct Framed { int64_t n_rec = 0, tail = 0; bool bad = false; };

struct Front {
    int max_blocks = 0;
    uint32_t seg = SEG_DEFAULT;
    hipStream_t stream = nullptr;                // the owner's
    // the stream of a batch: two buffers, so that the bytes carried over are copied from one to the front of the other
    DeviceBuffer d_stream[2];
    int cur = 0;
    int64_t carry_at = 0, carry = 0;             // in d_stream[cur]
    uint64_t carry_voff = 0;
    DeviceBuffer d_cdata, d_meta, d_exit, d_seg_entry, d_count, d_first, d_scan, d_starts, d_result;
    std::vector<uint8_t> meta;
    // the batch between open_batch and close_batch
    int to = 0, n_tab = 0;
    int64_t len = 0;
    uint8_t *bytes = nullptr;                    // the stream, on the device: len bytes and PAD behind them
    const int64_t *d_at = nullptr;               // the table of its pieces (voffset_at), on the device ...
    const uint64_t *d_voff = nullptr;
    const int64_t *m_at = nullptr;               // ... and on the host
    const uint64_t *m_voff = nullptr;
    Framed fr;

    uint64_t voffset(int64_t p) const { return voffset_at(m_at, m_voff, n_tab, p); }
    const int64_t *starts() const { return d_starts.as<int64_t>(); }
    void rewind() { carry = carry_at = 0; carry_voff = 0; }      // a new file, or a new read of one
    void reset();                                // every buffer freed: before the owner's stream goes

    // the framing of stream[0 .. len) from `entry`, enqueued and waited for: -> d_starts [n_rec], and what the chain ended on
    int frame(const HipFail &fail, const uint8_t *stream_bytes, int64_t stream_len, int64_t entry, Framed *out);
    // the blocks of a batch (checked here) inflated behind the carried bytes and framed from `entry`; waits for the stream
    int open_batch(const HipFail &fail, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize, const int32_t *out_len,
                   const int64_t *coffset, int64_t end_coffset, int64_t entry);
    // the verdicts of the frame step (a size word that cannot be; with `last`, bytes behind the last whole record), then the carry
    int close_batch(const HipFail &fail, int last);
};

// the arguments every entry point that takes a batch is given, before anything is done with them.  who: "batch", "mark"
inline int check_batch_args(const HipFail &fail, const char *who, const uint8_t *cdata, int64_t cbytes, int n, const int64_t *in_at, const int32_t *csize,
                            const int32_t *out_len, const int64_t *coffset, int64_t end_coffset, int64_t entry) {
    if (n > 0 && (!cdata || !in_at || !csize || !out_len || !coffset)) return fail("%s: NULL argument", who);
    if (cbytes < 0 || end_coffset < 0 || entry < 0) return fail("%s: negative argument", who);
    return 0;
}

// what the handle of a stage starts from (clair_bamidx, clair_bamsort, clair_markdup derive from it)
struct StageHandle {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;
    Front front;

    // a new handle: the arguments of _create checked, the device set, the stream made.  fail: the stage's, for a handle that is not there
    // yet; device_only: its sentence for a machine without an MI355X.  A handle that fails here goes through the stage's _destroy
    int open(const HipFail &fail, int on_device, int max_blocks, int segment_bytes, const char *device_only) {
        if (max_blocks < 1 || max_blocks > 16384) return fail("max_blocks %d: 1 .. 16384", max_blocks);
        if (segment_bytes == 0) segment_bytes = (int)SEG_DEFAULT;
        if (segment_bytes < (int)SEG_MIN || segment_bytes > (int)SEG_MAX || (segment_bytes & (segment_bytes - 1)))
            return fail("segment_bytes %d: a power of two in %u .. %u, or 0", segment_bytes, SEG_MIN, SEG_MAX);
        if (hip_device_check(fail, on_device, device_only)) return 1;
        device = on_device;
        front.max_blocks = max_blocks;
        front.seg = (uint32_t)segment_bytes;
        CLAIR_HIP_TRY(fail, hipSetDevice(device));
        CLAIR_HIP_TRY(fail, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        front.stream = stream;
        return 0;
    }
    // the two halves of _destroy, the stage's own buffers freed between them: before the stream goes, not in a destructor
    void settle() {
        if (!stream) return;                     // open failed: nothing was enqueued, no buffer is held
        (void)hipSetDevice(device);
        (void)hipStreamSynchronize(stream);
    }
    void close() {
        front.reset();
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};

}  // namespace clair_bix
