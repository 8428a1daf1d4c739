// Host-side helpers of the Clair hot path (include/clair_host.h): the overlap filter's walk, the twin of the device's
// (clair_amd/csrc/overlap.hip).  Plain C++17, no HIP.  The rule itself is csrc/overlap_core.h, the code the kernel runs; this is the
// sequential walk over all rows that the device path splits into independent segments.
#include "../../include/clair_host.h"
#include "../csrc/overlap_core.h"

#include <string.h>

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

static_assert(sizeof(clair_overlap_span) == 24, "span record layout");

extern "C" {

int clair_host_overlap_keep(const clair_overlap_span_t *spans, int64_t n, uint8_t *keep) {
    if (n < 0 || (n > 0 && (!spans || !keep))) return clair_host_fail("overlap keep: bad arguments");
    if (n == 0) return 0;
    memset(keep, 0, (size_t)n);
    clair_overlap_walk(spans, 0, n, keep);
    return 0;
}

}  // extern "C"
