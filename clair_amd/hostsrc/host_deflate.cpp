// The host twin of the device deflate (include/clair_host.h: clair_host_deflate_bgzf): the compressor of csrc/deflate_core.h compiled by the
// host compiler, its 64 lanes a loop.  No zlib here: this is the code that runs on the GPU, made testable and sanitizable on a machine
// without one, and what `--bgzf_deflate host` writes files with.
#include "../../include/clair_host.h"
#include "../csrc/deflate_core.h"

#include <cstring>
#include <memory>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

namespace {

using namespace clair_def;

struct HostCtx {
    Work *w;
    uint8_t *out;                            // SLOT bytes

    Work &work() { return *w; }
    void sync() {}
    void fence() {}
    uint32_t uniform(uint32_t v) const { return v; }
    void or_word(uint32_t *p, uint32_t v) { *p |= v; }
    void add_word(uint32_t *p, uint32_t v) { *p += v; }
    void store_word(uint32_t index, uint32_t v) {
        if (index >= SLOT / 4) return;
        const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
        memcpy(out + (size_t)index * 4, b, 4);
    }
    void store_bsize(uint32_t v) {
        out[16] = (uint8_t)v;
        out[17] = (uint8_t)(v >> 8);
    }
};

}  // namespace

extern "C" {

int clair_host_deflate_bgzf(const uint8_t *in, int64_t n_in, uint8_t *out, int64_t *n_out) {
    if ((!in && n_in > 0) || !out || !n_out) return clair_host_fail("NULL argument");
    if (n_in < 0 || n_in > (int64_t)MAX_IN) return clair_host_fail("deflate: %lld bytes in a BGZF block: 0 .. %u", (long long)n_in, MAX_IN);
    std::unique_ptr<Work> w(new Work);
    if (n_in) memcpy(w->in32, in, (size_t)n_in);
    memset(out, 0, SLOT);
    HostCtx c{w.get(), out};
    *n_out = deflate_bgzf(c, (uint32_t)n_in);
    return 0;
}

}  // extern "C"
