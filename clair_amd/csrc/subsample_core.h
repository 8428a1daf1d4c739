// The rule of read subsampling, one read name at a time: shared by the device path (csrc/frontend.hip: fe_bam_records_kernel, set by
// clair_frontend_bam_subsample) and the host twin (hostsrc/host_bam.cpp: clair_host_bam_render, clair_host_subsample_keeps).
// docs/subsample.md states it (htslib's, restated); nothing else in the native code restates it.
//
//   h = 0;  for every byte c of QNAME:  h = (h << 5) - h + (int8)c          (mod 2^32; the first byte alone gives (int8)c)
//   k = h ^ seed, through Wang's 32-bit mix
//   dropped  <=>  (double)(k & 0xffffff) / 16777216.0 >= frac                (both exact in double: host and device cannot disagree)
// frac <= 0: the rule is off (everything is kept); frac >= 1 keeps everything as well, the quotient being below 1.
#ifndef CLAIR_SUBSAMPLE_CORE_H
#define CLAIR_SUBSAMPLE_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CLAIR_SS_HD __host__ __device__
#else
#define CLAIR_SS_HD
#endif

// the hash of bytes[0 .. n), continued from h: a name may be handed over in pieces (the device reads it a dword at a time)
CLAIR_SS_HD inline uint32_t subsample_hash(const uint8_t *bytes, int64_t n, uint32_t h = 0) {
    for (int64_t i = 0; i < n; ++i) h = (h << 5) - h + (uint32_t)(int32_t)(int8_t)bytes[i];
    return h;
}

CLAIR_SS_HD inline bool subsample_keeps(uint32_t hash, uint32_t seed, double frac) {
    if (!(frac > 0.0)) return true;
    uint32_t k = hash ^ seed;
    k += ~(k << 15);
    k ^= k >> 10;
    k += k << 3;
    k ^= k >> 6;
    k += ~(k << 11);
    k ^= k >> 16;
    return !((double)(k & 0xffffffu) / 16777216.0 >= frac);
}

#endif /* CLAIR_SUBSAMPLE_CORE_H */
