// regress.hip -- mixture regression behind the score table (include/dpmm_hip_regress.h): from a range of the table a_k(i) that the sweep
// kernels' table mode wrote (table[k * stride + i]) and the range's points to mean[i][d] = sum_k p_ik (c_k + B_k x_i)_d and, if asked,
// the standard deviation of the mixture of the conditional laws.
//
// The tile -- 32 points per workgroup, one wave per 32 targets, the staging, the table row, the Float32 chain of mu_ik = c_k + B_k x_i and
// the way out -- is regress_device.h's.  Here: the clusters in increasing k; a cluster whose p_ik is 0 for all 32 points is left out (a
// Float32 expf underflows to exactly 0 for far clusters); a lane adds p mu and p (s V + mu^2) of its 16 targets to its Float64 sums, a lane
// whose own p is 0 adding nothing: what a point gets does not depend on its neighbours in the tile.
#include "regress_device.h"      // rt_chain: the __builtin_amdgcn_mfma_f32_32x32x2f32 chain of every cluster
#include "score_device.h"        // score_e, score_p: p_ik

namespace dpmm {

template <bool STD>
__global__ __launch_bounds__(64 * RT_MAXW) void regress_kernel(RegressArgs A) {
    extern __shared__ float rg_smem[];
    __shared__ int bad[RT_PTS];
    const RegressTile &T = A.t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int pt = lane & 31, half = lane >> 5;
    const int D = T.D, K = T.K, Tp = T.Tp;
    float *const xs = rg_smem;
    float *const os = rg_smem + D * RT_XP + wave * (RT_PTS * RT_XP);
    const int64_t i0 = (int64_t)blockIdx.x * RT_PTS;
    const int npt = T.n - i0 < RT_PTS ? (int)(T.n - i0) : RT_PTS;
    rt_stage(T.X, T.ldx, i0, npt, D, xs, bad);
    const int64_t i = i0 + pt;
    const bool valid = pt < npt;
    const float *col = T.table + (valid ? i : 0);
    const int64_t rs = T.stride;
    const RtRow w = rt_row(col, rs, K, valid, bad[pt]);
    rt_row_out(T, i, valid, w, lane);
    const int t0 = (blockIdx.y * nw + wave) * 32;       // this wave's block of 32 targets
    if (t0 >= Tp) return;                               // (a whole wave; no barrier below)
    // ---- the clusters
    double sum1[16], sum2[STD ? 16 : 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) sum1[r] = 0.0;
    if constexpr (STD) {
#pragma unroll
        for (int r = 0; r < 16; ++r) sum2[r] = 0.0;
    }
    const double dDo = (double)D;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const float a = col[(int64_t)k * rs];
        const float p = w.part ? score_p(score_e(a, w.m), w.s) : 0.f;
        if (__ballot(p != 0.f) == 0) continue;
        const rt_f32x16 acc = rt_chain(rt_chain_start(T.c, k, Tp, t0, half), A.Bt + (int64_t)k * D * Tp + t0, (int64_t)Tp, xs, 0, D, pt, half);
        if (p != 0.f) {
            const double pd = (double)p;
            if constexpr (STD) {
                const double df = T.hd[2 * k + 1];
                const double sc = (df + rt_q(T.hd[2 * k], df, a, dDo)) / (df + dDo - 2.0);
                const float *vk = A.V + (int64_t)k * Tp + t0 + 4 * half;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 v4 = *reinterpret_cast<const float4 *>(vk + 8 * g);
                    const float vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double mu = (double)acc[4 * g + j];
                        sum1[4 * g + j] += pd * mu;
                        sum2[4 * g + j] += pd * (sc * (double)vv[j] + mu * mu);
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) sum1[r] += pd * (double)acc[r];
            }
        }
    }
    // ---- out
    const float fnan = __uint_as_float(0x7fc00000u);
    const int nt = T.Dt - t0 < 32 ? T.Dt - t0 : 32;    // targets of this block that exist
    for (int pass = 0; pass < (STD ? 2 : 1); ++pass) {
        float *const out = pass == 0 ? A.mean : A.std;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v;
            if (pass == 0) {
                v = (float)sum1[r];
            } else {
                const double var = sum2[STD ? r : 0] - sum1[r] * sum1[r];
                v = (float)sqrt(var > 0.0 ? var : 0.0);
            }
            rt_put(os, r, pt, half, w.part ? v : fnan);
        }
        rt_flush(out, i0, A.ld, os, npt, nt, t0, pt, half);
        if (t0 + 32 >= Tp) rt_zero_pad(out, i0, A.ld, npt, T.Dt, A.ld, lane);
    }
}

hipError_t launch_regress_range(const RegressArgs &a, hipStream_t s) {
    if (a.t.n <= 0) return hipSuccess;
    if (!regress_tile_ok(a.t, a.ld)) return hipErrorInvalidValue;
    const RtGrid g = rt_grid(a.t);
    const size_t lds = sizeof(float) * ((size_t)a.t.D * RT_XP + (size_t)g.nw * RT_PTS * RT_XP);
    if (a.std) DPMM_LAUNCH((regress_kernel<true>), g.grid, dim3(64 * g.nw), lds, s, a);
    else DPMM_LAUNCH((regress_kernel<false>), g.grid, dim3(64 * g.nw), lds, s, a);
    return hipGetLastError();
}

}  // namespace dpmm
