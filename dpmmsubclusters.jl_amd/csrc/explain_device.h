// explain_device.h -- the wave maximum and the selection of the top features of a point, as a function: the statements explain_kernel
// (explain.hip) was written with.  explain_gap_kernel (explain_gap.hip) takes them from here with GAPS = true.  explain_kernel keeps its own
// text: routed through this function (GAPS = false) it computes the same bits, but the compiler allocates and schedules the kernel
// differently, and the default path is to stay the code it was.
#pragma once
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "missing_device.h"

namespace dpmm {

__device__ __forceinline__ unsigned long long exp_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// The top features of a point (A.top = m > 0) from the lane's residuals e and z-scores tz: the rank of |t| is its bit pattern plus one, 0 for
// a NaN (it ranks last); ties go to the lower index.  m rounds of a wave maximum over 64-bit keys (rank << 32) | (0xFFFFFFFF - d), the
// winner masked out; lane j < m keeps entry j and writes it.  GAPS: nm holds the NaN ballots of the point's features (miss_read_point), and a
// selected feature that is missing is reported as -1.
template <int NT, bool GAPS>
__device__ __forceinline__ void exp_select_top(const ExplainArgs &A, int64_t row, const float (&e)[NT], const float (&tz)[NT], const unsigned long long *nm, int D,
                                               int lane) {
    unsigned long long key[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = 64 * t + lane;
        const unsigned rank = tz[t] == tz[t] ? __float_as_uint(fabsf(tz[t])) + 1u : 0u;
        key[t] = j < D ? ((unsigned long long)rank << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j) : 0ull;      // (0: not in the running)
    }
    float fe = NAN, ft = NAN;
    int ff = -1;
    for (int r = 0; r < A.top; ++r) {
        unsigned long long best = 0ull;
#pragma unroll
        for (int t = 0; t < NT; ++t) best = key[t] > best ? key[t] : best;
        best = exp_wave_max(best);
        const unsigned d = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull);      // (the same in every lane; top <= D: a feature is left)
        const int dl = __builtin_amdgcn_readfirstlane((int)(d & 63u)), dt = __builtin_amdgcn_readfirstlane((int)(d >> 6));
        float se = 0.f, st = 0.f;
        bool sm = false;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t == dt) {
                se = e[t];
                st = tz[t];
                if constexpr (GAPS) sm = (nm[t] >> dl) & 1ull;
                if (lane == dl) key[t] = 0ull;
            }
        }
        se = miss_rl_f(se, dl);
        st = miss_rl_f(st, dl);
        if (lane == r) {
            fe = se;
            ft = st;
            ff = sm ? -1 : (int)d;
        }
    }
    if (lane < A.top) {
        if (A.residual) A.residual[row + lane] = fe;
        if (A.zscore) A.zscore[row + lane] = ft;
        if (A.feature_tail) A.feature_tail[row + lane] = ft;
        if (A.features) A.features[row + lane] = ff;
    }
}

}  // namespace dpmm
