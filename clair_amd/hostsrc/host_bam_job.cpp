// The input of the tools that rewrite a BAM as a job (include/clair_host.h: clair_host_bam_job_*): sort_bam and markdup_bam open it, read
// the header's bytes from it and hand it to their file driver (clair_host_bamsort_run, clair_host_markdup_run).  The job itself is
// hostsrc/bam_job.h.  Plain C++17 + zlib, no HIP.
#include "bam_job.h"

extern "C" {

int clair_host_bam_job_open(const char *path, clair_host_bam_job_t **out) {
    if (!out) return clair_host_fail("out is NULL");
    *out = nullptr;
    if (!path) return clair_host_fail("bam job open: NULL argument");
    clair_host_bam_job *job = new clair_host_bam_job;
    if (clair_job::open_job(path, "(SAM text and CRAM are out of scope)", job)) { delete job; return 1; }
    *out = job;
    return 0;
}

void clair_host_bam_job_close(clair_host_bam_job_t *job) { delete job; }

int clair_host_bam_job_header(const clair_host_bam_job_t *job, uint8_t *out, int64_t cap, int64_t *bytes) {
    if (!job || !bytes) return clair_host_fail("bam job header: NULL argument");
    *bytes = (int64_t)job->header.end;
    if (out && cap >= *bytes) memcpy(out, job->text.data(), job->header.end);
    return 0;
}

}  // extern "C"
