// index_bam's host side (clair_amd/hostsrc/host_bam_index.cpp over csrc/bam_index_core.h) as a stand-alone program, for a build with
// -fsanitize=address,undefined (tests/test_index_bam.py): the index of the BAM it is given, through the twin and the file driver.
//
//     index_bam_sanitize reads.bam segment_bytes max_blocks        segment_bytes 0: the sequential walk; else the segmented framing
// Prints one line: references, records, mapped, unplaced, runs, windows, and a checksum (FNV-1a, 64 bit) over the runs and the linear
// index -- what the test compares with the library's own answer.  A file the driver refuses: its message on the standard output, exit
// status 2.
#include "../include/clair_host.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

static std::string g_message;

int clair_host_fail(const char *fmt, ...) {      // host_io.cpp's, without the rest of that file
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_message = buf;
    return 1;
}
extern "C" const char *clair_host_last_error(void) { return g_message.c_str(); }

static uint64_t fnv(uint64_t h, const void *p, size_t n) {
    const unsigned char *b = (const unsigned char *)p;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: index_bam_sanitize reads.bam segment_bytes max_blocks\n"); return 1; }
    clair_host_bamidx_t *twin = nullptr;
    if (clair_host_bamidx_create(2, atoi(argv[3]), atoi(argv[2]), &twin) != 0) { printf("%s\n", g_message.c_str()); return 2; }
    clair_bamidx_backend_t backend;
    clair_host_bamidx_result_t *res = nullptr;
    int status = 0;
    if (clair_host_bamidx_backend(twin, &backend) != 0 || clair_host_bamidx_build(argv[1], &backend, atoi(argv[3]), &res) != 0) {
        printf("%s\n", g_message.c_str());
        status = 2;
    } else {
        int64_t info[6];
        clair_host_bamidx_result_info(res, info);
        std::vector<clair_bamidx_run_t> runs((size_t)info[4]);                   // exactly as long as their contents: a write past an end is seen
        std::vector<uint64_t> linear((size_t)info[5]);
        std::vector<int64_t> first_window((size_t)info[0] + 1);
        clair_host_bamidx_result_copy(res, runs.data(), linear.data(), first_window.data());
        uint64_t h = 0xcbf29ce484222325ull;
        for (const clair_bamidx_run_t &r : runs) {
            h = fnv(h, &r.tid, 4); h = fnv(h, &r.bin, 4); h = fnv(h, &r.beg, 8); h = fnv(h, &r.end, 8);
        }
        h = fnv(h, linear.data(), linear.size() * 8);
        printf("%lld %lld %lld %lld %lld %lld %016llx\n", (long long)info[0], (long long)info[1], (long long)info[2], (long long)info[3], (long long)info[4],
               (long long)info[5], (unsigned long long)h);
        clair_host_bamidx_result_free(res);
    }
    clair_host_bamidx_destroy(twin);
    return status;
}
