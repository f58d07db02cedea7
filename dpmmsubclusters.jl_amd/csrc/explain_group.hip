// explain_group.hip -- which GROUP of features makes a point atypical (include/dpmm_hip_explain_groups.h, which states the definitions, the
// packing of the tables and the error bounds): behind the typicality pass of a range of the score table (typicality.hip), whose class words
// say which points are scored and under which cluster,
//   explain_group_kernel       one wave per point, no workgroup barrier, no atomics.  z, y, q and g = R' y are formed by the statements of
//                              explain_kernel (miss_rz, the FMA chain, the butterfly, miss_rty), so q has the bits of `mahalanobis`.  g goes
//                              to a strip of LDS that belongs to the wave (64 NT floats: typ_gap_kernel is the precedent), so that a
//                              group's entries can be gathered by index.  Per group of s features: lane l gathers g_c for c = l, l + 64, ..;
//                              v_r = sum_{c <= r} W_rc g_c as a chain of Float32 FMAs in increasing c, the lanes over r in tiles of 64 --
//                              column c of W is one coalesced row of the image, zero above the diagonal and in the pad, g_c goes round
//                              with v_readlane; q_G = sum_r v_r^2 by the lane's FMA chain and the butterfly; then in Float32
//                                  h = df + max(q - q_G, 0),  f = (q_G (df + (D - s))) / h
//                              with a correctly rounded division and no contraction (-ffp-contract=off: the only FMAs are the explicit
//                              ones).  Lane j keeps group j's pair and writes it: one writer per output word.
//   explain_group_tail_kernel  one lane per entry in Float64, as explain_tail_kernel: the f explain_group_kernel left in group_tail becomes
//                              typ_tail (typicality_math.h) at (f, df + D - s, s), rounded once.
// Skipped and incomplete points get NaN rows.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "batchstats_device.h"
#include "missing_device.h"
#include "typicality_math.h"

namespace dpmm {

constexpr int EXG_WAVES = 4;      // waves per workgroup (they share nothing): EXP_WAVES of explain.hip

__device__ __forceinline__ float exg_wave_sum(float v) {      // (exp_wave_sum of explain.hip: every lane ends with the same bits)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the rows of a point that is not scored
__device__ __forceinline__ void exg_blank(const ExplainGroupArgs &A, int64_t i, int lane) {
    if (lane < A.G) {
        if (A.group_q) A.group_q[i * A.ld + lane] = NAN;
        if (A.group_tail) A.group_tail[i * A.ld + lane] = NAN;
    }
}

template <int NT>
__global__ __launch_bounds__(64 * EXG_WAVES) void explain_group_kernel(ExplainGroupArgs A) {
    constexpr int Dp = 64 * NT;
    __shared__ float sG[EXG_WAVES][Dp];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *const gs = sG[wave];
    const int D = A.D;
    const int64_t nw = (int64_t)gridDim.x * EXG_WAVES;
    for (int64_t i = (int64_t)blockIdx.x * EXG_WAVES + wave; i < A.n; i += nw) {
        const int k = __builtin_amdgcn_readfirstlane(A.cls[i]);
        if (k < 0) {
            exg_blank(A, i, lane);
            continue;
        }
        const float *x = A.X + i * A.ldx;
        float xv[NT];
        bool fin = true;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = 64 * t + lane;
            xv[t] = j < D ? x[j] : 0.f;
            fin = fin && bs_finite(xv[t]);
        }
        if (__ballot(!fin)) {
            exg_blank(A, i, lane);
            continue;
        }
        // z, y, q, g: the statements of explain_kernel
        const float *const mk = A.mu + (int64_t)k * A.mu_step;
        float z[NT], y[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = 64 * t + lane;
            z[t] = j < D ? xv[t] - mk[j] : 0.f;
        }
        miss_rz<NT>(A.Rt + (int64_t)k * D * Dp, z, D, lane, y);
        float q = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) q = fmaf(y[t], y[t], q);
        q = exg_wave_sum(q);
        float g[NT];
        miss_rty<NT>(A.Rr + (int64_t)k * D * Dp, y, D, lane, g);
        const float df = (float)A.cst[(int64_t)k * MISS_CST];      // (the Float32 value, widened by the host: exact)
        miss_lds_fence();      // (the gathers of the wave's last point are behind it)
#pragma unroll
        for (int t = 0; t < NT; ++t) gs[64 * t + lane] = g[t];      // (all 64 NT words: the pad holds the zeros of miss_rty)
        miss_lds_fence();
        const float *const Wk = A.W + (int64_t)k * A.wstep;
        float oq = NAN, of = NAN;
        for (int j = 0; j < A.G; ++j) {
            const int o0 = __builtin_amdgcn_readfirstlane(A.goff[j]);
            const int s = __builtin_amdgcn_readfirstlane(A.goff[j + 1]) - o0;
            const int sp = explain_group_pitch(s);
            const float *const Wj = Wk + A.gw[j];
            float gg[NT], v[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int c = 64 * t + lane;
                gg[t] = c < s ? gs[A.gfeat[o0 + c]] : 0.f;
                v[t] = 0.f;
            }
#pragma unroll
            for (int tc = 0; tc < NT; ++tc) {
                const int cn = s - 64 * tc < 64 ? s - 64 * tc : 64;      // (<= 0: the group ends before this tile)
#pragma unroll 4
                for (int cc = 0; cc < cn; ++cc) {
                    const float gc = miss_rl_f(gg[tc], cc);
                    const float *col = Wj + (int64_t)(64 * tc + cc) * sp + lane;
#pragma unroll
                    for (int tr = tc; tr < NT; ++tr)      // (the row tiles above hold zeros of the triangle and are skipped)
                        if (64 * tr < s) v[tr] = fmaf(col[64 * tr], gc, v[tr]);
                }
            }
            float qg = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) qg = fmaf(v[t], v[t], qg);      // (a tile behind the group: v = 0, qg keeps its bits)
            qg = exg_wave_sum(qg);
            const float h = df + fmaxf(q - qg, 0.f);
            const float f = (qg * (df + (float)(D - s))) / h;
            if (lane == j) {
                oq = qg;
                of = f;
            }
        }
        if (lane < A.G) {
            if (A.group_q) A.group_q[i * A.ld + lane] = oq;
            if (A.group_tail) A.group_tail[i * A.ld + lane] = of;      // (explain_group_tail_kernel turns it into its tail)
        }
    }
}

// One lane per entry, in Float64: the f explain_group_kernel left in group_tail becomes the tail of F(s, df_k + D - s) at f / s, typ_tail
// (typicality_math.h) at (f, df_k + D - s, s), rounded once.  A NaN (a point that is not scored, or an f that is NaN) stays NaN.
__global__ __launch_bounds__(256) void explain_group_tail_kernel(ExplainGroupArgs A) {
    const int64_t total = A.n * A.G;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / A.G;
        const int j = (int)(e - i * A.G);
        float *const w = A.group_tail + i * A.ld + j;
        const float f = *w;
        const int k = A.cls[i];
        const int s = A.goff[j + 1] - A.goff[j];
        if (k >= 0 && f == f) *w = (float)typ_tail((double)f, A.cst[(int64_t)k * MISS_CST] + (double)(A.D - s), s, nullptr);
    }
}

hipError_t launch_explain_group_range(const ExplainGroupArgs &a, int max_grid, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.D < 1 || a.D > 256 || a.G < 1 || a.G > EXPLAIN_MAX_GROUPS || a.ldx < a.D || a.ld < a.G || a.wstep < 1 || !a.X || !a.Rt || !a.Rr || !a.mu ||
        !a.cst || !a.cls || !a.goff || !a.gfeat || !a.gw || !a.W)
        return hipErrorInvalidValue;
    if (!a.group_q && !a.group_tail) return hipSuccess;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((a.n + EXG_WAVES - 1) / EXG_WAVES, max_grid));
    const int nt = (a.D + 63) / 64;
    if (nt == 1) DPMM_LAUNCH((explain_group_kernel<1>), dim3(grid), dim3(64 * EXG_WAVES), 0, s, a);
    else if (nt == 2) DPMM_LAUNCH((explain_group_kernel<2>), dim3(grid), dim3(64 * EXG_WAVES), 0, s, a);
    else if (nt == 3) DPMM_LAUNCH((explain_group_kernel<3>), dim3(grid), dim3(64 * EXG_WAVES), 0, s, a);
    else DPMM_LAUNCH((explain_group_kernel<4>), dim3(grid), dim3(64 * EXG_WAVES), 0, s, a);
    if (a.group_tail) {
        const int64_t total = a.n * a.G;
        DPMM_LAUNCH(explain_group_tail_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace dpmm
