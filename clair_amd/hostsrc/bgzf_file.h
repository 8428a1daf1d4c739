// BGZF as a file format, for the host sources that read BAM files (host_bam.cpp, host_bam_index.cpp): the constants, one block of an open
// file read and checked, one block inflated by zlib and judged, a batch of blocks inflated on a few threads.  Which blocks to read and how
// many to a batch is the caller's policy.  Host only: plain C++17 + zlib.
#pragma once
#include "../csrc/bam_record_core.h"
#include "../csrc/inflate_core.h"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

namespace clair_bgzf {

using clair_rec::u16;
using clair_rec::u32;

constexpr int BGZF_HEADER = 18, BGZF_FOOTER = 8, BGZF_MAX_BLOCK = 65536;
const uint8_t BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// a block's header, piece by piece: a gzip member of deflate data with FLG.FEXTRA (4 bytes seen); XLEN == 6 and the subfield BC (14 bytes
// seen); the subfield's two bytes, BSIZE (the whole header)
inline bool gzip_with_extra(const uint8_t *h) { return h[0] == 0x1f && h[1] == 0x8b && h[2] == 8 && (h[3] & 4); }
inline bool bc_subfield(const uint8_t *h) { return u16(h + 10) == 6 && h[12] == 'B' && h[13] == 'C'; }
inline bool block_header(const uint8_t *h) { return gzip_with_extra(h) && bc_subfield(h) && u16(h + 14) == 2; }

// the block at compressed offset `coffset` of `file` (`file_size` bytes, named `path` in messages): its header checked, its bytes appended to
// cbuf.  -> 0 and *csize (the whole block) and *isize (what it says it inflates to, at most BGZF_MAX_BLOCK), or the message set
inline int read_block(FILE *file, const char *path, uint64_t file_size, uint64_t coffset, std::vector<uint8_t> &cbuf, uint32_t *csize, uint32_t *isize) {
    uint8_t h[BGZF_HEADER];
    const auto cut = [&] { return clair_host_fail("%s: truncated BGZF block at compressed offset %llu", path, (unsigned long long)coffset); };
    if (coffset + BGZF_HEADER > file_size || fseeko(file, (off_t)coffset, SEEK_SET) != 0 || fread(h, 1, BGZF_HEADER, file) != BGZF_HEADER) return cut();
    if (!block_header(h)) return clair_host_fail("%s: not a BGZF block at compressed offset %llu", path, (unsigned long long)coffset);
    const uint32_t size = u16(h + 16) + 1;
    if (size < BGZF_HEADER + BGZF_FOOTER || coffset + size > file_size) return cut();
    const size_t at = cbuf.size();
    cbuf.resize(at + size);
    memcpy(cbuf.data() + at, h, BGZF_HEADER);
    if (fread(cbuf.data() + at + BGZF_HEADER, 1, size - BGZF_HEADER, file) != size - BGZF_HEADER) { cbuf.resize(at); return cut(); }
    *csize = size;
    *isize = u32(cbuf.data() + at + size - 4);
    if (*isize > (uint32_t)BGZF_MAX_BLOCK)
        return clair_host_fail("%s: BGZF block at compressed offset %llu claims %u bytes", path, (unsigned long long)coffset, *isize);
    return 0;
}

// one block -> out_len bytes at out: the status of the device inflate (inflate_core.h: BGZF_OK .. BGZF_CRC, output beyond out_len + 1 bytes
// is corrupt data there as here), or INFLATE_NO_ZLIB, which is no verdict on the block
constexpr int INFLATE_NO_ZLIB = -1;
inline int inflate_block(const uint8_t *block, uint32_t csize, uint8_t *out, uint32_t out_len) {
    z_stream z{};
    if (inflateInit2(&z, -15) != Z_OK) return INFLATE_NO_ZLIB;
    uint8_t spill = 0;
    z.next_in = const_cast<uint8_t *>(block) + BGZF_HEADER;
    z.avail_in = csize - BGZF_HEADER - BGZF_FOOTER;
    z.next_out = out_len ? out : &spill;
    z.avail_out = out_len;
    int rc = inflate(&z, Z_FINISH);
    if (rc != Z_STREAM_END && z.avail_out == 0) {            // room for one byte more: a block that inflates to more than ISIZE says so
        z.next_out = &spill;
        z.avail_out = 1;
        rc = inflate(&z, Z_FINISH);
    }
    const size_t got = z.total_out;
    inflateEnd(&z);
    if (rc != Z_STREAM_END) return clair_inf::BGZF_CORRUPT;
    if (got != out_len) return clair_inf::BGZF_SIZE;
    return (uint32_t)crc32(0L, out, out_len) == u32(block + csize - 8) ? clair_inf::BGZF_OK : clair_inf::BGZF_CRC;
}
inline const char *inflate_text(int status) { return status == INFLATE_NO_ZLIB ? "inflateInit2 failed" : clair_inf::bgzf_status_text(status); }

// block i of n: csize[i] bytes at cdata + in_at[i] -> out_len[i] bytes at out + out_at[i], status[i]; thread t of up to `threads` takes
// blocks t, t + nt, ...
inline void inflate_blocks(int threads, const uint8_t *cdata, int n, const int64_t *in_at, const int32_t *csize, const int64_t *out_at, const int32_t *out_len,
                           uint8_t *out, int32_t *status) {
    const auto one = [&](int i) { status[i] = inflate_block(cdata + in_at[i], (uint32_t)csize[i], out + out_at[i], (uint32_t)out_len[i]); };
    const int nt = std::max(1, std::min(threads, n));
    if (nt == 1) {
        for (int i = 0; i < n; ++i) one(i);
        return;
    }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; ++t) pool.emplace_back([&, t] { for (int i = t; i < n; i += nt) one(i); });
    for (auto &th : pool) th.join();
}

}  // namespace clair_bgzf
