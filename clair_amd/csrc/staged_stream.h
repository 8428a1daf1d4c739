// What the BGZF codecs' handles (inflate.hip, deflate.hip) are made of: one non-blocking stream, page-locked staging for both directions and
// the device buffers, sized once when the handle is created and reused by every batch.  Host side only.
#pragma once
#include "device_buffer.h"
#include "hip_status.h"

struct StagedStream {
    int device = 0;
    int max_blocks = 0;
    hipStream_t stream = nullptr;
    PinnedBuffer h_in, h_out, h_meta;
    DeviceBuffer d_in, d_out, d_meta;
    std::string error;

    // d_in_bytes >= in_bytes: the kernels read whole words around their input, so the device side has a margin and starts out zeroed
    int open(const HipFail &fail, int device_, int max_blocks_, size_t in_bytes, size_t out_bytes, size_t meta_bytes, size_t d_in_bytes) {
        device = device_;
        max_blocks = max_blocks_;
        CLAIR_HIP_TRY(fail, hipSetDevice(device));
        CLAIR_HIP_TRY(fail, hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        CLAIR_HIP_TRY(fail, h_in.ensure(in_bytes));
        CLAIR_HIP_TRY(fail, h_out.ensure(out_bytes));
        CLAIR_HIP_TRY(fail, h_meta.ensure(meta_bytes));
        CLAIR_HIP_TRY(fail, d_in.ensure(d_in_bytes));
        CLAIR_HIP_TRY(fail, d_out.ensure(out_bytes));
        CLAIR_HIP_TRY(fail, d_meta.ensure(meta_bytes));
        // on the handle's own (non-blocking) stream: a fill on the null stream is not ordered before this stream's first copy into the buffer
        CLAIR_HIP_TRY(fail, hipMemsetAsync(d_in.p, 0, d_in_bytes, stream));
        return 0;
    }

    void close() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (DeviceBuffer *b : {&d_in, &d_out, &d_meta}) b->reset();     // before the stream goes, not in the destructor
        for (PinnedBuffer *b : {&h_in, &h_out, &h_meta}) b->reset();
        if (stream) (void)hipStreamDestroy(stream);
        stream = nullptr;
    }
};
