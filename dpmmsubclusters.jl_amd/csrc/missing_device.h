// missing_device.h -- what the wave-per-point kernels of missing.hip and typicality.hip have in common: lane l of a wave carries features /
// rows l, l + 64, .. of a point (NT = ceil(D / 64) of them), and y = R z is formed in Float32 from the transposed copy Rt of the clusters'
// triangular factors (MissArgs::Rt).  The statements are those miss_system was written with, moved here unchanged.
#pragma once
#include "dpmm_device.h"

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

}  // namespace dpmm
