// The host twin of the device inflate (include/clair_host.h: clair_host_inflate_block, clair_host_inflate_bgzf): the decoder of
// csrc/inflate_core.h compiled by the host compiler, with its own CRC-32.  No zlib here: this is the code that runs on the GPU, made
// testable, fuzzable and sanitizable on a machine without one.  The reader's default path (host_bam.cpp) stays on zlib.
#include "../../include/clair_host.h"
#include "../csrc/bam_record_core.h"         // u32: the little-endian fields of the block's footer
#include "../csrc/inflate_core.h"

#include <cstring>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

namespace {

using namespace clair_inf;

constexpr uint32_t CRC_LANES = 64;           // the CRC is split and combined as the wave does it

struct HostCtx {
    const uint8_t *in;
    uint32_t n_in;
    uint8_t *out;
    Tables t;

    uint32_t word(uint32_t i) const {
        uint32_t w = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if ((uint64_t)i * 4 + k < n_in) w |= (uint32_t)in[(size_t)i * 4 + k] << (8 * k);
        return w;
    }
    void put(uint32_t pos, uint32_t byte) { out[pos] = (uint8_t)byte; }
    void copy(uint32_t pos, uint32_t dist, uint32_t len) {
        for (uint32_t k = 0; k < len; ++k) out[pos + k] = out[pos - dist + (k < dist ? k : k % dist)];
    }
    void stored(uint32_t pos, uint32_t at, uint32_t len) { memcpy(out + pos, in + at, len); }
    uint32_t uniform(uint32_t v) const { return v; }
    uint32_t lane() const { return 0; }
    uint32_t lanes() const { return 1; }
    void sync() {}
    Tables &tables() { return t; }
};

uint32_t crc_of(const uint8_t *p, uint32_t n) {
    static uint32_t table[256];
    static bool made = false;
    if (!made) {                             // idempotent: a race writes the same values
        for (uint32_t i = 0; i < 256; ++i) table[i] = crc_table_entry(i);
        made = true;
    }
    const auto byte_at = [p](uint32_t i) { return (uint32_t)p[i]; };
    uint32_t acc = crc_init_share(n);
    for (uint32_t lane = 0; lane < CRC_LANES; ++lane) acc ^= crc_lane_share(byte_at, table, n, lane, CRC_LANES);
    return ~acc;
}

}  // namespace

extern "C" {

int clair_host_inflate_block(const uint8_t *in, int64_t n_in, uint8_t *out, int64_t cap, int64_t *n_out, uint32_t *crc32, int *status) {
    if ((!in && n_in > 0) || (!out && cap > 0) || !n_out || !crc32 || !status) return clair_host_fail("NULL argument");
    if (n_in < 0 || n_in > (1 << 24) || cap < 0 || cap > (1 << 24)) return clair_host_fail("inflate: %lld bytes in, room for %lld: 0 .. 2^24 each", (long long)n_in, (long long)cap);
    HostCtx c{in, (uint32_t)n_in, out, {}};
    uint32_t produced = 0;
    const bool ended = inflate(c, 0, (uint32_t)n_in, (uint32_t)cap, &produced);
    *n_out = ended ? produced : 0;
    *crc32 = ended ? crc_of(out, produced) : 0;
    *status = ended ? BGZF_OK : BGZF_CORRUPT;
    return 0;
}

int clair_host_inflate_bgzf(const uint8_t *block, int64_t csize, uint8_t *out, int64_t *n_out, int *status) {
    if (!block || !out || !n_out || !status) return clair_host_fail("NULL argument");
    if (csize < 26 || csize > 65536) return clair_host_fail("BGZF block of %lld bytes: 26 .. 65536", (long long)csize);
    using clair_rec::u32;
    const uint32_t want = u32(block + csize - 8), isize = u32(block + csize - 4);
    if (isize > 65536) return clair_host_fail("BGZF block claims %u bytes", isize);
    HostCtx c{block + 18, (uint32_t)csize - 26, out, {}};
    uint32_t produced = 0;
    const bool ended = inflate(c, 0, (uint32_t)csize - 26, isize + 1, &produced);
    *n_out = ended ? produced : 0;
    *status = bgzf_status(ended, produced, isize, ended && produced == isize ? crc_of(out, produced) : 0, want);
    return 0;
}

}  // extern "C"
