// score_device.h -- the per-entry arithmetic of include/dpmm_hip_score.h, stated once for the kernels that must reproduce the bits of
// `probs` (score.hip, overlap.hip): a kernel that walks a row of the table a_k(i) with these functions in increasing k forms M, the
// label, S and p_k = probs[i][k] exactly as score_finish_kernel does.  (score.hip keeps the loop of its pass 1 written out -- as a
// function the same statements cost it another register allocation -- and takes score_e and score_p from here.)
#pragma once
#include "dpmm_device.h"

namespace dpmm {

// pass 1, entry k: the running maximum with NaN skipped and the label by Julia's argmax (the first NaN wins, else the first maximum)
__device__ __forceinline__ void score_max_step(float a, int k, float &m, int &best, bool &nan_seen) {
    if (a != a) {
        if (!nan_seen) { nan_seen = true; best = k; }
    } else if (a > m) {
        m = a;
        if (!nan_seen) best = k;
    }
}

// pass 2, entry k: e_k = expf(a_k - M), NaN -> -Inf first; S is their Float32 sum in increasing k
__device__ __forceinline__ float score_e(float a, float m) {
    if (a != a) a = -INFINITY;
    return expf(a - m);
}

// the probability probs holds
__device__ __forceinline__ float score_p(float e, float s) { return e / s; }

// the value logdens holds: the statement of score_finish_kernel's pass 2, for kernels that compare it with a floor (batchstats.hip)
__device__ __forceinline__ float score_logdens(float m, float s) { return (m == -INFINITY) ? -INFINITY : m + logf(s); }

}  // namespace dpmm
