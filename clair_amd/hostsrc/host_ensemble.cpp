// Host-side helpers of the Clair hot path (include/clair_host.h): the averaging of ensemble calling, the twin of the device's
// (clair_amd/csrc/ensemble.hip.h).  Plain C++17, no HIP.  The rule itself is csrc/ensemble_core.h, the code the kernel runs, so that
// both give the same bits; what it is measured against in tests is the text path it restates (printf "%.6f" and strtod).
#include "../../include/clair_host.h"
#include "../csrc/ensemble_core.h"

int clair_host_fail(const char *fmt, ...);   // host_io.cpp

extern "C" {

int clair_host_ensemble_average(const float *probs, int models, int64_t count, float *out) {
    if (models < 1 || models > CLAIR_ENSEMBLE_MAX_MODELS) return clair_host_fail("ensemble average: %d models, 1 .. %d", models, CLAIR_ENSEMBLE_MAX_MODELS);
    if (count < 0 || (count > 0 && (!probs || !out))) return clair_host_fail("ensemble average: bad arguments");
    for (int64_t i = 0; i < count; ++i) {
        double s = clair_ens_reread(probs[i]);
        for (int j = 1; j < models; ++j) s = s + clair_ens_reread(probs[(size_t)j * (size_t)count + (size_t)i]);
        out[i] = clair_ens_finish(s, models);
    }
    return 0;
}

int clair_host_ensemble_quantise(const float *p, int64_t count, int32_t *millionths) {
    if (count < 0 || (count > 0 && (!p || !millionths))) return clair_host_fail("ensemble quantise: bad arguments");
    for (int64_t i = 0; i < count; ++i) millionths[i] = (int32_t)clair_ens_quantise(p[i]);
    return 0;
}

int clair_host_ensemble_value(const int32_t *millionths, int64_t count, float *out) {
    if (count < 0 || (count > 0 && (!millionths || !out))) return clair_host_fail("ensemble value: bad arguments");
    for (int64_t i = 0; i < count; ++i) out[i] = clair_ens_value((double)millionths[i]);
    return 0;
}

}  // extern "C"
