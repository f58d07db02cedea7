// batchstats_device.h -- what the prep kernels of batchstats.hip (NIW) and countstats.hip (Multinomial) have in common: the class of a point
// from its row of the score table (passes 1 and 2 of score_finish_kernel, score_device.h) and the counters of a workgroup, integer adds in
// LDS.  The two kernels differ only in how they find a feature that is not finite -- that depends on the point store -- and call these
// functions around their own scan; the statements are those batchstats_prep_kernel was written with, moved here unchanged.
#pragma once
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"

namespace dpmm {

__device__ __forceinline__ bool bs_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// passes 1 and 2 over the column of one point: M, the label (0-based), NaN seen, S; rs: floats between two clusters' rows
__device__ __forceinline__ void bs_table_passes(const float *col, int64_t rs, int K, float &m, int &best, bool &nan_seen, float &s) {
    m = -INFINITY;
    best = 0;
    nan_seen = false;
    for (int k = 0; k < K; ++k) score_max_step(col[(int64_t)k * rs], k, m, best, nan_seen);
    s = 0.f;
    for (int k = 0; k < K; ++k) s += score_e(col[(int64_t)k * rs], m);
}

// the counters of one trip (as overlap_prep_kernel): cnt[0..K) the points that take part by label, cnt[K] skipped, cnt[K + 1] held out,
// cnt[K + 2] incomplete.  Called by whole waves.
__device__ __forceinline__ void bs_count(unsigned *cnt, int K, int lane, bool valid, bool scored, bool held, bool incomplete, bool part, int best) {
    const unsigned long long pm = __ballot(part);
    if (pm) {
        const int first = __ffsll((long long)pm) - 1;
        const int k0 = __shfl(best, first);
        if (__ballot(part && best != k0) == 0) {
            if (lane == first) atomicAdd(&cnt[k0], (unsigned)__popcll(pm));
        } else if (part) {
            atomicAdd(&cnt[best], 1u);
        }
    }
    const unsigned long long sm = __ballot(valid && !scored), hm = __ballot(held), im = __ballot(incomplete);
    if (lane == 0) {
        if (sm) atomicAdd(&cnt[K], (unsigned)__popcll(sm));
        if (hm) atomicAdd(&cnt[K + 1], (unsigned)__popcll(hm));
        if (im) atomicAdd(&cnt[K + 2], (unsigned)__popcll(im));
    }
}

// the workgroup's counters to one of the RANK_REPL replicas of the global ones: sums of integers, order-free
__device__ __forceinline__ void bs_flush(const unsigned *cnt, unsigned long long *count, int K, int tid, int nthreads) {
    unsigned long long *dst = count + (int64_t)(blockIdx.x % RANK_REPL) * (K + BATCHSTATS_COUNTERS);
    for (int k = tid; k < K + BATCHSTATS_COUNTERS; k += nthreads)
        if (cnt[k]) atomicAdd(&dst[k], (unsigned long long)cnt[k]);
}

}  // namespace dpmm
