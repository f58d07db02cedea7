// missing_device.h -- what the wave-per-point kernels of missing.hip, typicality.hip, explain.hip and explain_gap.hip have in common: lane l of
// a wave carries features / rows l, l + 64, .. of a point (NT = ceil(D / 64) of them), and y = R z is formed in Float32 from the transposed
// copy Rt of the clusters' triangular factors (MissArgs::Rt).  miss_read_point, miss_system, miss_residual and miss_lds_fence -- one
// cluster's small system of a point with NaN features -- are the statements missing.hip had them with: the gap kernels of typicality.hip
// and explain_gap.hip run them for the point's own cluster, with the bits of the patched table entry.
#pragma once
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "batchstats_device.h"

namespace dpmm {

__device__ __forceinline__ float miss_rl_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double miss_rl_d(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double miss_wave_sum(double v) {      // (a butterfly: every lane ends with the same bits)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// y = R z: column j of R (one coalesced row of Rk = Rt + k D Dp, zero below the diagonal and in the pad) scaled by z_j, j increasing; z_j
// goes round with v_readlane; rows above 64 (tj + 1) hold zeros of the triangle and are skipped.  z is 0 in the pad; y is overwritten.
template <int NT>
__device__ __forceinline__ void miss_rz(const float *Rk, const float (&z)[NT], int D, int lane, float (&y)[NT]) {
    constexpr int Dp = 64 * NT;
#pragma unroll
    for (int t = 0; t < NT; ++t) y[t] = 0.f;
#pragma unroll
    for (int tj = 0; tj < NT; ++tj) {
        const int jn = D - 64 * tj < 64 ? D - 64 * tj : 64;
#pragma unroll 4
        for (int jj = 0; jj < jn; ++jj) {
            const float zj = miss_rl_f(z[tj], jj);
            const float *c = Rk + (int64_t)(64 * tj + jj) * Dp + lane;
#pragma unroll
            for (int tr = 0; tr <= tj; ++tr) y[tr] = fmaf(c[64 * tr], zj, y[tr]);
        }
    }
}

// g = R' y, the sibling of miss_rz for the lower-triangular R': row r of R (one coalesced row of Rk = Rr + k D Dp of the row-major copy
// ExplainArgs::Rr, zero below the diagonal and in the pad) scaled by y_r, r increasing; y_r goes round with v_readlane; lane l accumulates
// g[64 t + l] = fma(Rr[r][64 t + l], y_r, g) for the tiles t >= r / 64 (the tiles below hold zeros of the triangle and are skipped).
// g is overwritten.
template <int NT>
__device__ __forceinline__ void miss_rty(const float *Rk, const float (&y)[NT], int D, int lane, float (&g)[NT]) {
    constexpr int Dp = 64 * NT;
#pragma unroll
    for (int t = 0; t < NT; ++t) g[t] = 0.f;
#pragma unroll
    for (int tr = 0; tr < NT; ++tr) {
        const int rn = D - 64 * tr < 64 ? D - 64 * tr : 64;
#pragma unroll 4
        for (int rr = 0; rr < rn; ++rr) {
            const float yr = miss_rl_f(y[tr], rr);
            const float *c = Rk + (int64_t)(64 * tr + rr) * Dp + lane;
#pragma unroll
            for (int t = tr; t < NT; ++t) g[t] = fmaf(c[64 * t], yr, g[t]);
        }
    }
}

constexpr int MISS_LDA = MISS_MAX + 1;         // doubles per row of a wave's A (odd: the lanes of a column fall into different banks)

__device__ __forceinline__ void miss_lds_fence() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// The range's point behind x: its values (0 in the pad), the NaN ballots per 64 features, M_a in lane a < r; returns r.
template <int NT>
__device__ __forceinline__ int miss_read_point(const float *x, int D, int lane, float (&xv)[NT], unsigned long long (&nm)[NT], int &myM) {
    int r = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = 64 * t + lane;
        xv[t] = j < D ? x[j] : 0.f;
        nm[t] = __ballot(xv[t] != xv[t]);
        r += __popcll(nm[t]);
    }
    // lane a < r learns M_a, the a-th missing feature
    myM = 0;
    int a = 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        unsigned long long mk = nm[t];
        while (mk) {
            const int b = __ffsll((long long)mk) - 1;
            mk &= mk - 1;
            if (lane == a) myM = 64 * t + b;
            ++a;
        }
    }
    return r;
}

// One cluster's small system of a listed point: y = R z, g = C'y, A = C'C = L L' and t = A^-1 g.  Leaves y, t_a in `gl` of lane a < r and L
// in the wave's LDS (the caller fences before A is overwritten); returns sum_j log L_jj = logdet A / 2.
template <int NT>
__device__ __forceinline__ double miss_system(const float *Rk, const float *mk, const float (&xv)[NT], const unsigned long long (&nm)[NT], int myM, int r,
                                              int D, int lane, double *Am, float (&y)[NT], double &gl) {
    constexpr int Dp = 64 * NT;
    float z[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = 64 * t + lane;
        const bool miss = (nm[t] >> lane) & 1ull;
        z[t] = (j < D && !miss) ? xv[t] - mk[j] : 0.f;
    }
    miss_rz<NT>(Rk, z, D, lane, y);      // ---- y = R z
    // ---- g = C'y into lane b, A = C'C (lower triangle) into the wave's LDS
    gl = 0.0;
    for (int b = 0; b < r; ++b) {
        const float *cb = Rk + (int64_t)__builtin_amdgcn_readlane(myM, b) * Dp + lane;
        float colb[NT];
        double p = 0.0;
#pragma unroll
        for (int t = 0; t < NT; ++t) { colb[t] = cb[64 * t]; p += (double)colb[t] * (double)y[t]; }
        p = miss_wave_sum(p);
        if (lane == b) gl = p;
        for (int a = 0; a <= b; ++a) {
            const float *ca = Rk + (int64_t)__builtin_amdgcn_readlane(myM, a) * Dp + lane;
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < NT; ++t) s += (double)ca[64 * t] * (double)colb[t];
            s = miss_wave_sum(s);
            if (lane == 0) Am[b * MISS_LDA + a] = s;
        }
    }
    miss_lds_fence();
    // ---- A = L L': lane a owns row a; column j is finished by the lanes j .. r - 1 at once
    double half_logdet = 0.0;
    for (int j = 0; j < r; ++j) {
        const bool act = lane >= j && lane < r;
        const int row = act ? lane : j;
        double s = Am[row * MISS_LDA + j];
        for (int t2 = 0; t2 < j; ++t2) s -= Am[row * MISS_LDA + t2] * Am[j * MISS_LDA + t2];
        const double dj = sqrt(miss_rl_d(s, j));
        half_logdet += log(dj);
        if (act) Am[lane * MISS_LDA + j] = (lane == j) ? dj : s / dj;
        miss_lds_fence();
    }
    // ---- t = A^-1 g: L u = g, then L't = u; lane a ends with t_a
    for (int j = 0; j < r; ++j) {
        if (lane == j) gl = gl / Am[j * MISS_LDA + j];
        const double uj = miss_rl_d(gl, j);
        if (lane > j && lane < r) gl -= Am[lane * MISS_LDA + j] * uj;
    }
    for (int j = r - 1; j >= 0; --j) {
        if (lane == j) gl = gl / Am[j * MISS_LDA + j];
        const double tj = miss_rl_d(gl, j);
        if (lane < j) gl -= Am[j * MISS_LDA + lane] * tj;
    }
    return half_logdet;
}

// res = y - C t in Float64 (t_a in `gl` of lane a < r), the lane's rows of it; returns q_o = |res|^2, every lane with the same bits
template <int NT>
__device__ __forceinline__ double miss_residual_vec(const float *Rk, const float (&y)[NT], double gl, int myM, int r, int lane, double (&res)[NT]) {
    constexpr int Dp = 64 * NT;
#pragma unroll
    for (int t = 0; t < NT; ++t) res[t] = (double)y[t];
    for (int a = 0; a < r; ++a) {
        const float *ca = Rk + (int64_t)__builtin_amdgcn_readlane(myM, a) * Dp + lane;
        const double ta = miss_rl_d(gl, a);
#pragma unroll
        for (int t = 0; t < NT; ++t) res[t] -= (double)ca[64 * t] * ta;
    }
    double q = 0.0;
#pragma unroll
    for (int t = 0; t < NT; ++t) q += res[t] * res[t];
    return miss_wave_sum(q);
}

// q_o = |y - C t|^2 alone
template <int NT>
__device__ __forceinline__ double miss_residual(const float *Rk, const float (&y)[NT], double gl, int myM, int r, int lane) {
    double res[NT];
    return miss_residual_vec<NT>(Rk, y, gl, myM, r, lane, res);
}

// true in every lane iff all the point's OBSERVED features (xv, nm of miss_read_point) are finite
template <int NT>
__device__ __forceinline__ bool miss_observed_finite(const float (&xv)[NT], const unsigned long long (&nm)[NT], int D, int lane) {
    bool fin = true;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const bool miss = (nm[t] >> lane) & 1ull;
        fin = fin && (64 * t + lane >= D || miss || bs_finite(xv[t]));
    }
    return __ballot(!fin) == 0ull;
}

}  // namespace dpmm
