// The BAM header, parsed once for the host sources that open BAM files (host_bam.cpp, host_bam_index.cpp): the magic, the text (skipped), the
// reference names and lengths.  Written over what the caller has of the inflated stream: need(bytes) makes at least `bytes` bytes from the
// stream's start available (non-zero: it could not, and has said why), data() is where they are now (need may move them).  Host only.
#pragma once
#include "../csrc/bam_record_core.h"

#include <cstring>
#include <string>
#include <vector>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

struct BamHeader {
    std::vector<std::string> names;
    std::vector<int64_t> lengths;
    size_t end = 0;                          // the first record's position in the inflated stream
};

// `advice`: what the caller adds to the refusal of a BGZF file that is no BAM ("" for nothing)
template <class Need, class Data>
inline int parse_bam_header(const char *path, const char *advice, const Need &need, const Data &data, BamHeader *out) {
    using clair_rec::u32;
    if (need(12)) return 1;
    if (memcmp(data(), "BAM\1", 4)) return clair_host_fail("%s: BGZF but not BAM (no BAM\\1 magic)%s", path, advice);
    const uint32_t l_text = u32(data() + 4);
    if (need(12 + (size_t)l_text)) return 1;
    size_t at = 8 + (size_t)l_text;
    const int32_t n_ref = (int32_t)u32(data() + at);
    if (n_ref < 0) return clair_host_fail("%s: negative n_ref in the BAM header", path);
    at += 4;
    for (int32_t i = 0; i < n_ref; ++i) {
        if (need(at + 4)) return 1;
        const uint32_t l_name = u32(data() + at);
        if (l_name == 0 || l_name > (1u << 20)) return clair_host_fail("%s: bad reference name length in the BAM header", path);
        if (need(at + 4 + l_name + 4)) return 1;
        const uint8_t *name = data() + at + 4;
        out->names.emplace_back((const char *)name, strnlen((const char *)name, l_name));
        out->lengths.push_back((int64_t)u32(name + l_name));
        at += 4 + (size_t)l_name + 4;
    }
    out->end = at;
    return 0;
}
