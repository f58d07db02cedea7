// sample_device.h -- the uniforms and the chi^2 draw that sample.hip (include/dpmm_hip_sample.h) and the imputation draws of missing.hip
// (include/dpmm_hip_impute.h) share.  Device code only.
#pragma once
#include "dpmm_device.h"

namespace dpmm {

__device__ __forceinline__ float sample_u32(uint32_t v) {       // (v + 0.5) 2^-32, rounded to Float32: in (0, 1]
    return __builtin_fmaf((float)v, 2.3283064365386963e-10f, 1.1641532182693481e-10f);
}
__device__ __forceinline__ double sample_u53(uint32_t a, uint32_t b) {          // (0, 1), 53 bits
    return ((double)((((uint64_t)a << 32) | b) >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}

// g ~ chi^2(df) = 2 Gamma(df / 2, 1) of sample i.  Marsaglia-Tsang, at most SN_ROUNDS rounds with fresh blocks (2t, 2t + 1), then the last
// positive proposal stands (none in 8 rounds -- probability below 1e-60 -- : the mode's neighbourhood d).  A round rejects with probability
// below 0.05 for every shape >= 1, so the law differs from Gamma by less than 0.05^8 < 4e-11 in total variation.
// stream / block0: the Philox stream and the first of the 64 blocks the draw may use (the sampler: STREAM_SAMPLE_CHI, 0).
constexpr int SN_ROUNDS = 8;
__device__ __forceinline__ double sample_chi2(double df, uint64_t seed, uint64_t i, uint32_t stream = STREAM_SAMPLE_CHI, uint32_t block0 = 0u) {
    double a = 0.5 * df, boost = 1.0;
    if (a < 1.0) {
        const Philox4 ru = philox4x32_10(seed, i, block0 + 63u, stream);
        boost = pow(sample_u53(ru.v[0], ru.v[1]), 1.0 / a);
        a += 1.0;
    }
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double last = d;
    for (uint32_t t = 0; t < (uint32_t)SN_ROUNDS; ++t) {
        const Philox4 rn = philox4x32_10(seed, i, block0 + 2u * t, stream);
        const double x = sqrt(-2.0 * log(sample_u53(rn.v[0], rn.v[1]))) * cos(6.283185307179586476925 * sample_u53(rn.v[2], rn.v[3]));
        const Philox4 ru = philox4x32_10(seed, i, block0 + 2u * t + 1u, stream);
        const double u = sample_u53(ru.v[0], ru.v[1]);
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        last = d * v;
        if (u < 1.0 - 0.0331 * x * x * x * x) break;
        if (log(u) < 0.5 * x * x + d * (1.0 - v + log(v))) break;
    }
    return 2.0 * last * boost;
}

}  // namespace dpmm
