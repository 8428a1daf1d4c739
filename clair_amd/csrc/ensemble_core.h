// The averaging rule of ensemble calling, one probability at a time: shared by the device kernel (csrc/ensemble.hip.h) and the host
// twin (hostsrc/host_ensemble.cpp: clair_host_ensemble_average).  docs/ensemble.md derives it.
//
// The reference's result is defined by a TEXT round trip, not by a float32 mean: call_var --output_for_ensemble prints every
// probability with '{:0.6f}' (clair/call_var.py:950-1000), clair/post_processing/ensemble.py:33-43 reads the rows of a site back with
// float(), adds them in input order in double, :67 divides by their count and prints '{:.6f}' again, and call_var
// --input_probabilities reads that into float32 (clair/call_var.py:1291).  The functions below reproduce each of those steps value for
// value, so that K models averaged in process give the bits the chain of K + 2 processes gives.
//
// Every product whose rounding matters is a ROUNDED product: hipcc contracts a * b + c into a fused multiply-add by default, which
// would skip exactly the rounding step printf has.  NaN is out of scope; probabilities lie in [0, 1].
#ifndef CLAIR_ENSEMBLE_CORE_H
#define CLAIR_ENSEMBLE_CORE_H

#include <math.h>

#if defined(__HIPCC__)
#define CLAIR_ENS_HD __host__ __device__
#else
#define CLAIR_ENS_HD
#endif

#define CLAIR_ENSEMBLE_MAX_MODELS 8

// a * b rounded to double once, whatever the compiler's contraction setting
CLAIR_ENS_HD inline double clair_ens_mul(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    volatile double p = a * b;
    return p;
#endif
}

// Steps 1 and 2: what float("%.6f" % p) is.  p * 1e6 is exact in double (a 24-bit significand times 1e6 < 2^20 needs 44 bits), so its
// rint -- ties to even -- is the integer printf prints; k / 1e6, correctly rounded, is the double strtod reads from those digits.
CLAIR_ENS_HD inline double clair_ens_quantise(float p) { return rint(clair_ens_mul((double)p, 1e6)); }
CLAIR_ENS_HD inline double clair_ens_reread(float p) { return clair_ens_quantise(p) / 1e6; }

// Step 4: the exact binary value of `a`, rounded half-even to six decimals, as an integer count of millionths -- what '{:.6f}' prints.
// rint(a * 1e6) is NOT that: the product is rounded before rint sees it, and a mean of an even number of six-decimal values sits on or
// a hair beside a half-way point more often than not.  t = the rounded product, r = its exact residual (a * 1e6 == t + r exactly),
// f = floor(t), g = t - f (exact): the true fraction is g + r with |r| far below any gap that matters.
CLAIR_ENS_HD inline double clair_ens_millionths(double a) {
    const double t = clair_ens_mul(a, 1e6);
    const double r = fma(a, 1e6, -t);
    const double f = floor(t);
    const double g = t - f;
    if (g > 0.5 || (g == 0.5 && r > 0.0)) return f + 1.0;
    if (g == 0.5 && r == 0.0) return floor(f * 0.5) * 2.0 == f ? f : f + 1.0;    // an exact tie: the even neighbour
    return f;                                                              // g == 0 with r < 0 included: a hair below f, f is the nearest
}

// Step 5: the float32 the reader of the averaged row holds for the digits of m millionths (np.array(["0.xxxxxx"], dtype=np.float32)).
CLAIR_ENS_HD inline float clair_ens_value(double m) { return (float)(m / 1e6); }

// Steps 3 (the division) to 5: the sum of K re-read values -> that float32.
CLAIR_ENS_HD inline float clair_ens_finish(double sum, int models) { return clair_ens_value(clair_ens_millionths(sum / (double)models)); }

#endif /* CLAIR_ENSEMBLE_CORE_H */
