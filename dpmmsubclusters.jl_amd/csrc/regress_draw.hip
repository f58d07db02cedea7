// regress_draw.hip -- draws of the targets of a mixture regression (include/dpmm_hip_regress_draw.h states the law and the keying): from a
// range of the table a_k(i) and the range's points to x_M = c_k + B_k x_i + W_k (s n) with k ~ p_ik, for every draw asked for.
//
// Two kernels per range and batch of draws.
//   regress_draw_scale_kernel  one thread per point: it walks the point's row of the table ONCE with the functions of score_device.h (M, S,
//            hence p_ik with the bits `probs` holds) and forms, for every draw, the component (one 53-bit uniform against the Float64
//            cumulative sums of p_ik), g ~ chi^2(df + D_o) and the scale s = (float) sqrt((df + q) / g), into kc[jd][i] and sc[jd][i]; a row
//            with a NaN or without a finite entry gives component -1.  The Float64 library code of the chi^2 draw lives here, in a kernel of
//            its own: inlined into the chains' kernel it left 79 scalar registers spilled, and a point's scale was formed by all 8 threads
//            that serve it.
//   regress_draw_kernel        the tile of regress_device.h: a workgroup owns 32 points and a block of up to 4 x 32 targets, one wave
//            per 32 targets; the points are staged transposed in LDS (xs[e * 33 + p]) ONCE for the draws of the tile.  Per draw:
//     normals  the threads that serve point p share the Philox blocks of its normals (block b: thread (wave, half) takes b = 2 wave + half,
//              step 2 nw) and write s n into the second transposed image ns[a * 33 + p]; a workgroup barrier in front (the chains of the
//              draw before have read ns) and one behind;
//     clusters in increasing k, only those some point of the tile drew (one __ballot): (D_o + D_t - t0) / 2 v_mfma_f32_32x32x2_f32, A operand
//              the rows of the cluster's image Bw (B_k' on top of W_k', 128-byte lines), B operand xs and then ns from coordinate t0 on
//              (the coordinates below the wave's first target meet structural zeros of W), accumulator started from c_k: one Float32
//              fused-multiply-add chain per target.  A lane keeps the result where its own component is k;
//     write    through the wave-private 32 x 33 tile: the 32 targets of a point leave as one 128-byte segment.
// One writer per output word, no atomics; nothing a point gets depends on its neighbours in the tile.
#include "regress_device.h"      // rt_chain: the __builtin_amdgcn_mfma_f32_32x32x2f32 chain of every cluster
#include "score_device.h"        // score_e, score_p: p_ik
#include "sample_device.h"

namespace dpmm {

constexpr size_t RD_MAX_LDS = 65536;

__global__ __launch_bounds__(256) void regress_draw_scale_kernel(const float *table, int64_t rs, int64_t n, int K, double dDo, const double *hd, uint64_t seed,
                                                                 int64_t gi0, int64_t draw0, int ndraws, int32_t *kcs, float *scs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *col = table + i;
    const RtRow w = rt_row(col, rs, K, true, false);
    const float m = w.m, s = w.s;
    const bool part = w.part;
    const uint64_t gi = (uint64_t)(gi0 + i);
#pragma unroll 1
    for (int jd = 0; jd < ndraws; ++jd) {
        const uint32_t b0 = 64u * (uint32_t)(draw0 + jd);
        int kc = -1;
        float sc = 0.f;
        if (part) {
            const Philox4 rc = philox4x32_10(seed, gi, b0, STREAM_REGRESS_COMP);
            const double u = sample_u53(rc.v[0], rc.v[1]);
            double cum = 0.0;
            int klast = 0;
            for (int kk = 0; kk < K && kc < 0; ++kk) {
                const float pk = score_p(score_e(col[(int64_t)kk * rs], m), s);
                if (!(pk > 0.f)) continue;
                cum += (double)pk;
                klast = kk;
                if (u < cum) kc = kk;
            }
            if (kc < 0) kc = klast;
            const double df = hd[2 * kc + 1];
            const double q = rt_q(hd[2 * kc], df, col[(int64_t)kc * rs], dDo);
            const double g = sample_chi2(df + dDo, seed, gi, STREAM_REGRESS_CHI, b0);
            sc = (float)sqrt((df + q) / g);
        }
        kcs[(int64_t)jd * n + i] = kc;
        scs[(int64_t)jd * n + i] = sc;
    }
}

__global__ __launch_bounds__(64 * RT_MAXW) void regress_draw_kernel(RegressDrawArgs A) {
    extern __shared__ float rd_smem[];
    __shared__ int bad[RT_PTS];
    const RegressTile &T = A.t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int pt = lane & 31, half = lane >> 5;
    const int D = T.D, Dt = T.Dt, K = T.K, Tp = T.Tp;
    const int nb4 = (Dt + 3) >> 2;                       // Philox blocks of the normals of a draw
    float *const xs = rd_smem;
    float *const ns = rd_smem + D * RT_XP;
    float *const os = ns + 4 * nb4 * RT_XP + wave * (RT_PTS * RT_XP);
    const int64_t i0 = (int64_t)blockIdx.x * RT_PTS;
    const int npt = T.n - i0 < RT_PTS ? (int)(T.n - i0) : RT_PTS;
    rt_stage(T.X, T.ldx, i0, npt, D, xs, bad);
    const int64_t i = i0 + pt;
    const bool valid = pt < npt;
    const int64_t iv = valid ? i : 0;                   // (lanes past the end read point 0 and write nothing)
    const bool part = valid && A.kc[iv] >= 0 && !bad[pt];      // (the scale kernel has walked the row: it takes part in every draw or in none)
    const int t0 = (blockIdx.y * nw + wave) * 32;      // this wave's block of 32 targets
    const bool active = t0 < Tp;                        // (a wave without targets still serves the normals and the barriers)
    if (blockIdx.y == 0 && wave == 0 && T.skip) rt_count_skipped(T.skip, valid, part, lane);
    const uint64_t gi = (uint64_t)(A.i0 + i);
    const int b_lo = blockIdx.y * nw * 8;               // the first block of normals this workgroup's targets meet a non-zero of W in
    const float fnan = __uint_as_float(0x7fc00000u);
    const int nt = Dt - t0 < 32 ? Dt - t0 : 32;         // targets of this wave's block that exist
    const int ndraws = A.ndraws;
#pragma unroll 1
    for (int jd = 0; jd < ndraws; ++jd) {
        const uint32_t b0 = 64u * (uint32_t)(A.draw0 + jd);
        const int kc = part ? A.kc[(int64_t)jd * T.n + iv] : -1;
        const float sc = part ? A.sc[(int64_t)jd * T.n + iv] : 0.f;
        // ---- s n of this lane's point: coordinate a is word a & 3 of block a >> 2, Box-Muller as miss_draw_kernel
        __syncthreads();
        for (int b = b_lo + 2 * wave + half; b < nb4; b += 2 * nw) {
            const Philox4 rn = philox4x32_10(A.seed, gi, b0 + (uint32_t)b, STREAM_REGRESS_NORMAL);
            const float r0 = sqrtf(fmaxf(-2.0f * __logf(sample_u32(rn.v[0])), 0.0f)), r1 = sqrtf(fmaxf(-2.0f * __logf(sample_u32(rn.v[2])), 0.0f));
            const float th0 = 6.2831853071795865f * sample_u32(rn.v[1]), th1 = 6.2831853071795865f * sample_u32(rn.v[3]);
            float *const nb = ns + 4 * b * RT_XP + pt;
            nb[0] = sc * (r0 * __cosf(th0));
            nb[RT_XP] = sc * (r0 * __sinf(th0));
            nb[2 * RT_XP] = sc * (r1 * __cosf(th1));
            nb[3 * RT_XP] = sc * (r1 * __sinf(th1));
        }
        __syncthreads();
        if (active) {
            // ---- the clusters some point of the tile drew
            rt_f32x16 res;
#pragma unroll
            for (int r = 0; r < 16; ++r) res[r] = 0.f;
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                if (__ballot(kc == k) == 0) continue;
                const float *bk = A.Bw + (int64_t)k * (D + Dt) * Tp + t0;      // the cluster's image: B_k' on top of W_k'
                rt_f32x16 acc = rt_chain(rt_chain_start(T.c, k, Tp, t0, half), bk, Tp, xs, 0, D, pt, half);
                acc = rt_chain(acc, bk + (int64_t)D * Tp, Tp, ns, t0, Dt, pt, half);      // (W_k[d][a] = 0 for a < d, and d >= t0 here)
                if (kc == k) res = acc;
            }
            // ---- out
            const int64_t ld = A.ld, width = ld < A.draw_stride ? ld : A.draw_stride;
            float *const out = A.out + (int64_t)jd * A.draw_stride;
#pragma unroll
            for (int r = 0; r < 16; ++r) rt_put(os, r, pt, half, part ? res[r] : fnan);
            rt_flush(out, i0, ld, os, npt, nt, t0, pt, half);
            if (t0 + 32 >= Tp) rt_zero_pad(out, i0, ld, npt, Dt, width, lane);
        }
        if (A.comp && blockIdx.y == 0 && wave == 0 && half == 0 && valid) A.comp[(int64_t)jd * A.comp_stride + i] = kc;
    }
}

hipError_t launch_regress_draw_range(const RegressDrawArgs &a, hipStream_t s) {
    const RegressTile &t = a.t;
    if (t.n <= 0 || a.ndraws <= 0) return hipSuccess;
    if (!regress_tile_ok(t, a.ld < a.draw_stride ? a.ld : a.draw_stride) || t.Dt > REGRESS_MAX_TARGETS || t.Tp != regress_pitch(t.Dt) || !a.out || a.i0 < 0 ||
        a.draw0 < 0 || a.draw0 + a.ndraws > REGRESS_DRAW_MAX || !a.kc || !a.sc || t.n > t.stride)
        return hipErrorInvalidValue;
    const RtGrid g = rt_grid(t);
    const size_t lds = sizeof(float) * ((size_t)t.D * RT_XP + (size_t)4 * ((t.Dt + 3) / 4) * RT_XP + (size_t)g.nw * RT_PTS * RT_XP);
    if (lds > RD_MAX_LDS) return hipErrorInvalidValue;      // (dpmm_set_regression_factor refuses D_o + D_t > 256: at most 51 KiB)
    DPMM_LAUNCH(regress_draw_scale_kernel, dim3((unsigned)((t.n + 255) / 256)), dim3(256), 0, s, t.table, t.stride, t.n, t.K, (double)t.D, t.hd, a.seed,
                a.i0, a.draw0, a.ndraws, a.kc, a.sc);
    DPMM_LAUNCH(regress_draw_kernel, g.grid, dim3(64 * g.nw), lds, s, a);
    return hipGetLastError();
}

}  // namespace dpmm
