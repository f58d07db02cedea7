// explain.hip -- why a point is atypical (include/dpmm_hip_explain.h, which states the definitions): behind the typicality pass of a range of
// the score table (typicality.hip), whose class words say which points are scored and under which cluster,
//   explain_rows_kernel   Rr[k][r][d] = R_k[r][d] from the packed upper triangles of the parameter staging (the row-major sibling of
//   explain_diag_kernel   miss_transpose_kernel's Rt), and a[k][d] = sum_{r <= d} R_rd^2, summed in Float64 and rounded once; once per
//                         parameter set, by the first explain call that sees it.
//   explain_kernel        one wave per point, no workgroup barrier, no LDS: lane l carries features l, l + 64, .. as typ_q_kernel does.  z, y
//                         and q are formed by the statements of typ_q_kernel (miss_rz, the FMA chain, the butterfly), so q has the bits of
//                         `mahalanobis`; then g = R' y by miss_rty (missing_device.h) and, per feature, in Float32
//                             e = g / a,  s = g g / a,  h = df + max(q - s, 0),  t = g sqrt((df + (D - 1)) / (a h))
//                         with correctly rounded divisions and square roots and no contraction (-ffp-contract=off: the only FMAs are the
//                         explicit ones).  top == 0: every lane writes its features.  top == m: m rounds of a wave maximum over 64-bit
//                         keys (rank of |t|) << 32 | (0xFFFFFFFF - d), the winner masked out; lane j < m keeps entry j and writes it.
//                         One writer per output word, no atomics: skipped and incomplete points were counted by the typicality pass.
//   explain_tail_kernel   one lane per entry in Float64, as typ_tail_kernel: the z-score explain_kernel left in feature_tail becomes
//                         typ_tail (typicality_math.h) at D = 1 of its square, rounded once.
// Skipped and incomplete points get NaN rows and features = -1.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "batchstats_device.h"
#include "missing_device.h"
#include "typicality_math.h"

namespace dpmm {

constexpr int EXP_WAVES = 4;      // waves per workgroup (they share nothing): TYP_WAVES of typicality.hip

__global__ __launch_bounds__(256) void explain_rows_kernel(const float *__restrict__ Rpk, int64_t step, float *__restrict__ Rr, int K, int D, int Dp) {
    const int64_t total = (int64_t)K * D * Dp;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int d = (int)(e % Dp);
        const int r = (int)((e / Dp) % D);
        const int k = (int)(e / ((int64_t)Dp * D));
        // packed upper triangle: row r holds the columns r .. D - 1 from word r D - r (r - 1) / 2
        Rr[e] = (d >= r && d < D) ? Rpk[(int64_t)k * step + (int64_t)r * D - (int64_t)r * (r - 1) / 2 + (d - r)] : 0.f;
    }
}

__global__ __launch_bounds__(256) void explain_diag_kernel(const float *__restrict__ Rpk, int64_t step, float *__restrict__ a, int K, int D, int Dp) {
    const int64_t total = (int64_t)K * Dp;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int d = (int)(e % Dp);
        const int k = (int)(e / Dp);
        double s = 0.0;
        if (d < D)
            for (int r = 0; r <= d; ++r) {
                const double v = (double)Rpk[(int64_t)k * step + (int64_t)r * D - (int64_t)r * (r - 1) / 2 + (d - r)];
                s += v * v;
            }
        a[e] = (float)s;
    }
}

__device__ __forceinline__ float exp_wave_sum(float v) {      // (typ_wave_sum of typicality.hip: every lane ends with the same bits)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ unsigned long long exp_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// the rows of a point that is not scored
template <int NT>
__device__ __forceinline__ void exp_blank(const ExplainArgs &A, int64_t i, int lane) {
    const int64_t row = i * A.ld;
    if (A.top > 0) {
        if (lane < A.top) {
            if (A.residual) A.residual[row + lane] = NAN;
            if (A.zscore) A.zscore[row + lane] = NAN;
            if (A.feature_tail) A.feature_tail[row + lane] = NAN;
            if (A.features) A.features[row + lane] = -1;
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = 64 * t + lane;
        if (j < A.D) {
            if (A.residual) A.residual[row + j] = NAN;
            if (A.zscore) A.zscore[row + j] = NAN;
            if (A.feature_tail) A.feature_tail[row + j] = NAN;
        }
    }
}

template <int NT>
__global__ __launch_bounds__(64 * EXP_WAVES) void explain_kernel(ExplainArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = A.D;
    constexpr int Dp = 64 * NT;
    const int64_t nw = (int64_t)gridDim.x * EXP_WAVES;
    for (int64_t i = (int64_t)blockIdx.x * EXP_WAVES + wave; i < A.n; i += nw) {
        const int k = __builtin_amdgcn_readfirstlane(A.cls[i]);
        if (k < 0) {
            exp_blank<NT>(A, i, lane);
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
            exp_blank<NT>(A, i, lane);
            continue;
        }
        // z, y, q: the statements of typ_q_kernel
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
        q = exp_wave_sum(q);
        float g[NT];
        miss_rty<NT>(A.Rr + (int64_t)k * D * Dp, y, D, lane, g);
        const float df = (float)A.cst[(int64_t)k * MISS_CST];      // (the Float32 value, widened by the host: exact)
        const float c = df + (float)(D - 1);
        const float *const ak = A.a + (int64_t)k * Dp;
        float e[NT], tz[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = 64 * t + lane;
            e[t] = tz[t] = 0.f;
            if (j < D) {
                const float a = ak[j];
                e[t] = g[t] / a;
                const float s = g[t] * g[t] / a;
                const float h = df + fmaxf(q - s, 0.f);
                tz[t] = g[t] * sqrtf(c / (a * h));
            }
        }
        const int64_t row = i * A.ld;
        if (A.top == 0) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int j = 64 * t + lane;
                if (j < D) {
                    if (A.residual) A.residual[row + j] = e[t];
                    if (A.zscore) A.zscore[row + j] = tz[t];
                    if (A.feature_tail) A.feature_tail[row + j] = tz[t];      // (explain_tail_kernel turns it into its tail)
                }
            }
            continue;
        }
        // the top features: the rank of |t| is its bit pattern plus one, 0 for a NaN (it ranks last); ties go to the lower index
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
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t == dt) {
                    se = e[t];
                    st = tz[t];
                    if (lane == dl) key[t] = 0ull;
                }
            }
            se = miss_rl_f(se, dl);
            st = miss_rl_f(st, dl);
            if (lane == r) {
                fe = se;
                ft = st;
                ff = (int)d;
            }
        }
        if (lane < A.top) {
            if (A.residual) A.residual[row + lane] = fe;
            if (A.zscore) A.zscore[row + lane] = ft;
            if (A.feature_tail) A.feature_tail[row + lane] = ft;
            if (A.features) A.features[row + lane] = ff;
        }
    }
}

// One lane per entry, in Float64: the z-score explain_kernel left in feature_tail becomes its two-sided tail, typ_tail (typicality_math.h) at
// D = 1 with df_k + D - 1 degrees of freedom, rounded once.  A NaN (a point that is not scored, or a z-score that is NaN) stays NaN.
__global__ __launch_bounds__(256) void explain_tail_kernel(ExplainArgs A) {
    const int width = A.top ? A.top : A.D;
    const int64_t total = A.n * width;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t i = e / width;
        float *const w = A.feature_tail + i * A.ld + (e - i * width);
        const float t = *w;
        const int k = A.cls[i];
        if (k >= 0 && t == t) *w = (float)typ_tail((double)t * (double)t, A.cst[(int64_t)k * MISS_CST] + (double)(A.D - 1), 1, nullptr);
    }
}

hipError_t launch_explain_params(const float *Rpk, int64_t step, float *Rr, float *a, int K, int D, hipStream_t s) {
    if (K < 1 || D < 1 || D > 256 || !Rpk || !Rr || !a) return hipErrorInvalidValue;
    const int Dp = miss_pitch(D);
    const int64_t total = (int64_t)K * D * Dp;
    DPMM_LAUNCH(explain_rows_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, Rpk, step, Rr, K, D, Dp);
    DPMM_LAUNCH(explain_diag_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)K * Dp + 255) / 256, 4096)), dim3(256), 0, s, Rpk, step, a, K, D, Dp);
    return hipGetLastError();
}

hipError_t launch_explain_range(const ExplainArgs &a, int max_grid, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const int cap = a.D < EXPLAIN_MAX_TOP ? a.D : EXPLAIN_MAX_TOP;
    if (a.K < 1 || a.D < 1 || a.D > 256 || a.ldx < a.D || a.top < 0 || a.top > cap || a.ld < (a.top ? a.top : a.D) || !a.X || !a.Rt || !a.Rr || !a.a || !a.mu ||
        !a.cst || !a.cls)
        return hipErrorInvalidValue;
    if (!a.residual && !a.zscore && !a.feature_tail && !(a.top && a.features)) return hipSuccess;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((a.n + EXP_WAVES - 1) / EXP_WAVES, max_grid));
    const int nt = (a.D + 63) / 64;
    if (nt == 1) DPMM_LAUNCH((explain_kernel<1>), dim3(grid), dim3(64 * EXP_WAVES), 0, s, a);
    else if (nt == 2) DPMM_LAUNCH((explain_kernel<2>), dim3(grid), dim3(64 * EXP_WAVES), 0, s, a);
    else if (nt == 3) DPMM_LAUNCH((explain_kernel<3>), dim3(grid), dim3(64 * EXP_WAVES), 0, s, a);
    else DPMM_LAUNCH((explain_kernel<4>), dim3(grid), dim3(64 * EXP_WAVES), 0, s, a);
    if (a.feature_tail) {
        const int64_t total = a.n * (a.top ? a.top : a.D);
        DPMM_LAUNCH(explain_tail_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace dpmm
