// explain_gap.hip -- the explanation of points with gaps (include/dpmm_hip_explain.h, "Points with gaps"; DPMM_OPT_TYPICALITY_GAPS): behind
// explain_kernel and explain_tail_kernel of a range (explain.hip, unchanged: they leave blank rows for these points), and only where the range
// has a list of points with NaN features (MissArgs::list of missing.hip, just made by the walk's missing-feature pass),
//   explain_gap_kernel    one wave per LISTED point,
//                         no workgroup barrier, wave-private LDS: the steps of typ_gap_kernel (typicality.hip) give y, t, L and q_o
//                         with the bits of `mahalanobis`; the residual y - C t is kept (Float64, miss_residual_vec of missing_device.h),
//                         rounded to Float32 and g' = R' res formed by miss_rty; then r more passes of miss_rty, over the columns c_a of
//                         R, give w_a = R' c_a, and every lane forward-substitutes L v = w for its own features in Float64 as the passes
//                         arrive, a' = A_dd - |v|^2 in Float64.  v (16 NT doubles per lane) lives in the wave's LDS next to L, word
//                         (a NT + t) 64 + lane: a lane reads only what it wrote itself, consecutive lanes hit consecutive banks, and the
//                         pass loop is an ordinary loop over a < r.  (Held in registers, v needs the 16 passes unrolled, and that kernel
//                         spilled up to 35 SGPRs.)  8 NT + 2 KB of LDS per wave, so a workgroup has 4 / 2 / 2 / 1 waves at
//                         NT = 1 / 2 / 3 / 4.  Per feature, in
//                         Float64 from the Float32 g', q_o, df and rounded once,
//                             e = g' / a',  s = g' g' / a',  h = df + max(q_o - s, 0),  t = g' sqrt((df + (D_o - 1)) / (a' h)),
//                         NaN on M.  Selection and layouts as explain_kernel; a selected feature of M gets -1 in `features`.  A listed
//                         point that is skipped, or has an observed feature that is not finite, is not touched.
//                         Where tails are asked for, lane 0 adds r << 24 to the point's class word (nobody else reads it any more).
//   explain_gap_tail_kernel   one lane per entry of a LISTED point's row, as explain_tail_kernel: the z-score explain_gap_kernel left in
//                         feature_tail becomes its tail (typ_tail at D = 1, df + D_o - 1 degrees of freedom, Float64 rounded once); r is
//                         read from the class word, 0 there meaning that the point was not scored.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "batchstats_device.h"
#include "missing_device.h"
#include "explain_device.h"
#include "typicality_math.h"

namespace dpmm {

constexpr int EXP_GAP_SHIFT = 24;  // explain_gap_kernel leaves r above this bit of a scored listed point's class word (K < 2^24)
// waves per workgroup (they share nothing but the workgroup's LDS allocation, which stays under 64 KB)
constexpr int exp_gap_waves(int nt) { return nt == 1 ? 4 : nt <= 3 ? 2 : 1; }

// The value of a wave-uniform word, opaque to the compiler: taken inside the loop over the wave's points, it keeps the lane masks and flags
// derived from the kernel's arguments (j < D per tile, top == 0, the null tests of the outputs) from being hoisted out of that loop, where
// they are live across everything and, at NT >= 2, no longer fit into the scalar registers.  An empty statement: nothing is executed.
__device__ __forceinline__ int exp_per_point(int v) {
    asm volatile("" : "+s"(v));
    return v;
}
template <class T>
__device__ __forceinline__ T *exp_per_point(T *p) {
    asm volatile("" : "+s"(p));
    return p;
}

template <int NT>
__global__ __launch_bounds__(64 * exp_gap_waves(NT)) void explain_gap_kernel(ExplainArgs A) {
    constexpr int W = exp_gap_waves(NT);
    __shared__ double sA[W][MISS_MAX * MISS_LDA];
    __shared__ double sV[W][MISS_MAX * NT * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *const Am = sA[wave];
    double *const Vm = sV[wave] + lane;
    constexpr int Dp = 64 * NT;
    // (the launcher admits a range of less than 2^31 points, so the list's length and le + nw fit into 32 bits)
    const unsigned total = (unsigned)A.list_cnt[0];
    const unsigned nw = gridDim.x * W;
    for (unsigned le = blockIdx.x * W + wave; le < total; le += nw) {
        const int64_t i = A.list[le];
        const int k = __builtin_amdgcn_readfirstlane(A.cls[i]);
        if (k < 0) continue;
        const int D = exp_per_point(A.D);
        float xv[NT];
        unsigned long long nm[NT];
        int myM;
        const int r = miss_read_point<NT>(A.X + i * A.ldx, D, lane, xv, nm, myM);
        if (!miss_observed_finite<NT>(xv, nm, D, lane)) continue;      // (it stays incomplete)
        const float *const Rtk = A.Rt + (int64_t)k * D * Dp;
        const float *const Rrk = A.Rr + (int64_t)k * D * Dp;
        float y[NT];
        double gl;
        miss_system<NT>(Rtk, A.mu + (int64_t)k * A.mu_step, xv, nm, myM, r, D, lane, Am, y, gl);
        double res[NT];
        const double q = (double)(float)miss_residual_vec<NT>(Rtk, y, gl, myM, r, lane, res);      // (the Float32 `mahalanobis`)
        float resf[NT], g[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) resf[t] = (float)res[t];
        miss_rty<NT>(Rrk, resf, D, lane, g);
        // L v = w, pass a: w_a = R' c_a, v_a = (w_a - sum_{b < a} L_ab v_b) / L_aa; sub gathers v_a^2
        double sub[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) sub[t] = 0.0;
        for (int a = 0; a < r; ++a) {
            const float *ca = Rtk + (int64_t)__builtin_amdgcn_readlane(myM, a) * Dp + lane;
            float c[NT], w[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) c[t] = ca[64 * t];
            miss_rty<NT>(Rrk, c, D, lane, w);
            double sv[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) sv[t] = (double)w[t];
            for (int b = 0; b < a; ++b) {
                const double lab = Am[a * MISS_LDA + b];
#pragma unroll
                for (int t = 0; t < NT; ++t) sv[t] -= lab * Vm[(b * NT + t) * 64];
            }
            const double laa = Am[a * MISS_LDA + a];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const double va = sv[t] / laa;
                Vm[(a * NT + t) * 64] = va;
                sub[t] += va * va;
            }
        }
        miss_lds_fence();      // (the next point overwrites A)
        const double df = A.cst[(int64_t)k * MISS_CST];
        const double c = df + (double)(D - r - 1);
        const float *const ak = A.a + (int64_t)k * Dp;
        float e[NT], tz[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = 64 * t + lane;
            const bool miss = (nm[t] >> lane) & 1ull;
            e[t] = tz[t] = NAN;
            if (j < D && !miss) {
                const double a = (double)ak[j] - sub[t], gd = (double)g[t];
                e[t] = (float)(gd / a);
                const double h = df + fmax(q - gd * gd / a, 0.0);
                tz[t] = (float)(gd * sqrt(c / (a * h)));
            }
        }
        const int64_t row = i * A.ld;
        ExplainArgs B = A;
        B.top = exp_per_point(A.top);
        B.residual = exp_per_point(A.residual);
        B.zscore = exp_per_point(A.zscore);
        B.feature_tail = exp_per_point(A.feature_tail);
        B.features = exp_per_point(A.features);
        if (B.feature_tail && lane == 0) A.cls[i] = k | (r << EXP_GAP_SHIFT);      // (for explain_gap_tail_kernel)
        if (B.top == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int j = 64 * t + lane;
                if (j < D) {
                    if (B.residual) B.residual[row + j] = e[t];
                    if (B.zscore) B.zscore[row + j] = tz[t];
                    if (B.feature_tail) B.feature_tail[row + j] = tz[t];      // (explain_gap_tail_kernel turns it into its tail)
                }
            }
            continue;
        }
        // a feature of M has a NaN z-score, ranks last and is reported as -1
        exp_select_top<NT, true>(B, row, e, tz, nm, D, lane);      // (explain_device.h)
    }
}

// One lane per entry of a listed point's row, in Float64, as explain_tail_kernel; r comes from the point's class word (explain_gap_kernel).
__global__ __launch_bounds__(256) void explain_gap_tail_kernel(ExplainArgs A) {
    const int width = A.top ? A.top : A.D;
    const unsigned long long total = A.list_cnt[0] * (unsigned long long)width;
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * 256) {
        const unsigned long long le = e / (unsigned)width;
        const int64_t i = A.list[le];
        const int cw = A.cls[i];
        const int r = cw < 0 ? 0 : cw >> EXP_GAP_SHIFT;      // (0: explain_gap_kernel left the point's blank row)
        float *const w = A.feature_tail + i * A.ld + (int64_t)(e - le * (unsigned)width);
        const float t = *w;
        if (r > 0 && t == t)
            *w = (float)typ_tail((double)t * (double)t, A.cst[(int64_t)(cw & ((1 << EXP_GAP_SHIFT) - 1)) * MISS_CST] + (double)(A.D - r - 1), 1, nullptr);
    }
}

hipError_t launch_explain_gap_range(const ExplainArgs &a, int max_grid, hipStream_t s) {
    if (a.n <= 0 || !a.list) return hipSuccess;
    const int cap = a.D < EXPLAIN_MAX_TOP ? a.D : EXPLAIN_MAX_TOP;
    if (a.K < 1 || a.D < 1 || a.D > 256 || a.ldx < a.D || a.top < 0 || a.top > cap || a.ld < (a.top ? a.top : a.D) || !a.X || !a.Rt || !a.Rr || !a.a || !a.mu ||
        !a.cst || !a.cls)
        return hipErrorInvalidValue;
    if (!a.residual && !a.zscore && !a.feature_tail && !(a.top && a.features)) return hipSuccess;
    // the list's length is on the device: a grid for a range full of gaps, as launch_miss_patch
    if (!a.list_cnt || a.n > (int64_t)0x7fffffffll || a.K >= (1 << EXP_GAP_SHIFT)) return hipErrorInvalidValue;
    const int nt = (a.D + 63) / 64, w = exp_gap_waves(nt);
    const int ggrid = (int)std::max<int64_t>(1, std::min<int64_t>((a.n + w - 1) / w, max_grid / w));
    if (nt == 1) DPMM_LAUNCH((explain_gap_kernel<1>), dim3(ggrid), dim3(64 * w), 0, s, a);
    else if (nt == 2) DPMM_LAUNCH((explain_gap_kernel<2>), dim3(ggrid), dim3(64 * w), 0, s, a);
    else if (nt == 3) DPMM_LAUNCH((explain_gap_kernel<3>), dim3(ggrid), dim3(64 * w), 0, s, a);
    else DPMM_LAUNCH((explain_gap_kernel<4>), dim3(ggrid), dim3(64 * w), 0, s, a);
    if (a.feature_tail) {
        const int64_t total = a.n * (a.top ? a.top : a.D);
        DPMM_LAUNCH(explain_gap_tail_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace dpmm
