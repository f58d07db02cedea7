// countstats_device.h -- what countstats_prep_kernel (countstats.hip) and countholdout_class_kernel (holdout.hip) have in common: the
// scan of a workgroup's points for a value that is not finite, over whichever of the three point stores is live, and the class of a point
// under the Multinomial model -- skipped, else held out, else incomplete, else it takes part -- with both floors, the raw one on logdens and
// the one per count.  One rule, one piece of code: the counters of the two headers are equal because the same statements form them.
#pragma once
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"
#include "batchstats_device.h"

namespace dpmm {

// Points base .. base + rows - 1 of a range (X / cpb already stand at point `base`): a value that is not finite marks its point in gap[]
// (LDS, cleared by the caller; every writer writes 1).  Float32 store: the rows read flat, word f is feature f % ldx of row f / ldx; sparse
// store: the entries cpb[0] .. cpb[rows] read flat and the (rare) offender's column found by bisection in cpb; a byte is finite.  Called by
// whole workgroups of `nthreads`.
__device__ __forceinline__ void cs_mark_gaps(unsigned *gap, int store, const float *X, int ldx, const int64_t *cpb, const float *val, int rows, int D, int tid,
                                             int nthreads) {
    if (store == COUNTSTATS_F32) {
        bs_mark_gaps(gap, X, rows, ldx, D, tid, nthreads);
    } else if (store == COUNTSTATS_SPARSE) {
        const int64_t e1 = cpb[rows];
        for (int64_t e = cpb[0] + tid; e < e1; e += nthreads)
            if (!bs_finite(val[e])) {
                int lo = 0, hi = rows - 1;                 // the last column that starts at or before e
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (cpb[mid] <= e) lo = mid; else hi = mid - 1;
                }
                gap[lo] = 1;
            }
    }
}

// The class of point i of a range from what bs_table_passes left and its mark.  tot: the range's Float64 totals t_i as
// countstats_totals_kernel wrote them, read only if use_pc and the point is complete.  A point is held out if the raw floor holds it out,
// or if the floor per count is on, every value of the point is finite, t_i > 0 and (double)logdens_i < (double)min_pc * t_i.
__device__ __forceinline__ void cs_class(bool valid, bool nan_seen, float m, float s, unsigned gapped, int use_floor, float min_logdens, int use_pc, float min_pc,
                                         const double *tot, int64_t i, bool &scored, bool &held, bool &incomplete, bool &part) {
    scored = valid && !nan_seen && m > -INFINITY && m < INFINITY;
    held = scored && use_floor && score_logdens(m, s) < min_logdens;
    if (scored && !held && use_pc && gapped == 0) {
        const double t = tot[i];
        held = t > 0. && (double)score_logdens(m, s) < (double)min_pc * t;
    }
    incomplete = scored && !held && gapped != 0;
    part = scored && !held && !incomplete;
}

// t_i, the Float64 total of a point's values, for the floor per count (countstats.hip) and the binomial law of a feature
// (count_explain.hip): one wave per point.  Lane l adds entries l, l + 64, .. in order, then
// a fixed butterfly combines the lanes (every lane ends with the same sum): a function of the point alone, exact for integer data.
template <typename T>
__device__ __forceinline__ double cs_wave_total(const T *v, int64_t len, int lane) {
    double t = 0.;
    for (int64_t e = lane; e < len; e += 64) t += (double)v[e];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
    return t;
}

}  // namespace dpmm
