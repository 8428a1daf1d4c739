// sort_bam's host side (clair_amd/hostsrc/host_bam_sort.cpp over csrc/bam_sort_core.h, with host_deflate.cpp) as a stand-alone program, for
// a build with -fsanitize=address,undefined (tests/test_sort_bam.py): the records of the BAM it is given, sorted through the twin and the
// file driver and appended to an output that starts empty.
//
//     sort_bam_sanitize in.bam out segment_bytes max_blocks memory        segment_bytes 0: the sequential walk; else the segmented framing
// Prints one line: records, groups, reads of the input, whether the input was sorted, and a checksum (FNV-1a, 64 bit) over the bytes the
// driver wrote -- what the test compares with the library's own answer.  A file the driver refuses: its message on the standard output,
// exit status 2, and no output file.
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

int main(int argc, char **argv) {
    if (argc != 6) { fprintf(stderr, "usage: sort_bam_sanitize in.bam out segment_bytes max_blocks memory\n"); return 1; }
    const int segment = atoi(argv[3]), max_blocks = atoi(argv[4]);
    const int64_t memory = atoll(argv[5]);
    clair_host_bamsort_t *twin = nullptr;
    clair_host_bam_job_t *job = nullptr;
    clair_bamsort_backend_t backend;
    int64_t stats[CLAIR_BAMSORT_STATS] = {0};
    int status = 0;
    remove(argv[2]);
    if (clair_host_bamsort_create(2, max_blocks, segment, &twin) != 0 || clair_host_bamsort_backend(twin, &backend) != 0 ||
        clair_host_bam_job_open(argv[1], &job) != 0 || clair_host_bamsort_run(job, &backend, argv[2], 0, memory, max_blocks, 2, stats) != 0) {
        printf("%s\n", g_message.c_str());
        remove(argv[2]);
        status = 2;
    } else {
        int64_t header_bytes = 0;
        clair_host_bam_job_header(job, nullptr, 0, &header_bytes);
        std::vector<uint8_t> header((size_t)header_bytes);                       // exactly as long as its contents: a write past the end is seen
        clair_host_bam_job_header(job, header.data(), header_bytes, &header_bytes);
        uint64_t h = 0xcbf29ce484222325ull;
        int64_t bytes = 0;
        FILE *f = fopen(argv[2], "rb");
        for (int c; f && (c = fgetc(f)) != EOF; ++bytes) h = (h ^ (unsigned char)c) * 0x100000001b3ull;
        if (f) fclose(f);
        if (bytes != stats[6] || header_bytes < 12) { printf("%lld bytes in the file, %lld reported\n", (long long)bytes, (long long)stats[6]); status = 2; }
        else printf("%lld %lld %lld %lld %016llx\n", (long long)stats[0], (long long)stats[3], (long long)stats[4], (long long)stats[5], (unsigned long long)h);
    }
    clair_host_bam_job_close(job);
    clair_host_bamsort_destroy(twin);
    return status;
}
