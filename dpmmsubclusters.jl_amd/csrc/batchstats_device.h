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

// rows base .. base + rows - 1 of X, flat: word f is feature f % ldx of row f / ldx; a word that is not finite (features d < D only) marks
// its row in gap[] (LDS, cleared by the caller; every writer writes 1).  Called by whole workgroups of `nthreads`.
__device__ __forceinline__ void bs_mark_gaps(unsigned *gap, const float *xr, int rows, int ldx, int D, int tid, int nthreads) {
    for (int f = tid; f < rows * ldx; f += nthreads) {
        const int r = f / ldx;
        if (f - r * ldx < D && !bs_finite(xr[f])) gap[r] = 1;
    }
}

// the class of point i of a range from what bs_table_passes left and its mark: skipped, else held out, else incomplete, else it takes part.
// tail: the range's tails as launch_typicality_range wrote them, read only if use_tail.  batchstats_prep_kernel (batchstats.hip) and
// holdout_class_kernel (holdout.hip) both call this: one rule, one piece of code.
__device__ __forceinline__ void bs_class(bool valid, bool nan_seen, float m, float s, unsigned gapped, int use_floor, float min_logdens, int use_tail,
                                         float min_tail, const float *tail, int64_t i, bool &scored, bool &held, bool &incomplete, bool &part) {
    scored = valid && !nan_seen && m > -INFINITY && m < INFINITY;
    // (the tail of a point with a feature that is not finite is NaN and compares false: such a point stays incomplete)
    held = scored && ((use_floor && score_logdens(m, s) < min_logdens) || (use_tail && gapped == 0 && tail[i] < min_tail));
    incomplete = scored && !held && gapped != 0;
    part = scored && !held && !incomplete;
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
