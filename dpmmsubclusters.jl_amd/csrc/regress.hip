// regress.hip -- mixture regression behind the score table (include/dpmm_hip_regress.h): from a range of the table a_k(i) that the sweep
// kernels' table mode wrote (table[k * stride + i]) and the range's points to mean[i][d] = sum_k p_ik (c_k + B_k x_i)_d and, if asked,
// the standard deviation of the mixture of the conditional laws.
//
// A workgroup owns RG_PTS = 32 points of the range and a block of up to 4 x 32 targets, one wave per 32 targets:
//   stage    the 32 points, transposed, into LDS (xs[e * 33 + p]: the read of X is coalesced along e, the odd pitch spreads the writes over
//            the banks); a point with a feature that is not finite is flagged;
//   row      lane l walks the table row of point p = l & 31 (both halves of the wave: the same statements on the same words) with the
//            functions of score_device.h: M, the label, S -- hence p_ik = e_k / S with the bits `probs` holds;
//   clusters in increasing k; a cluster whose p_ik is 0 for all 32 points is left out (a Float32 expf underflows to exactly 0 for far
//            clusters).  A cluster that stays costs D / 2 v_mfma_f32_32x32x2_f32: A operand B_k' (lane l: Bt[k][e + (l >> 5)][t0 + (l & 31)],
//            128-byte lines of the transposed table), B operand the points (xs[(e + (l >> 5)) * 33 + (l & 31)]), accumulator started
//            from c_k -- an exact Float32 fused-multiply-add chain in increasing e.  Lane l then holds mu for point l & 31 and the 16
//            targets 8 (r >> 2) + 4 (l >> 5) + (r & 3), and adds p mu and p (s V + mu^2) to its Float64 sums, a lane whose own p is 0
//            adding nothing: what a point gets does not depend on its neighbours in the tile;
//   write    through a wave-private LDS tile of 32 x 33 words, so that the 32 targets of a point leave as one 128-byte segment.
// One writer per output word, no atomics; the points that take no part are counted per tile, in a word only this workgroup's block 0
// writes (the host adds the words up).
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"

namespace dpmm {

typedef float rg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int RG_PTS = 32;               // points per workgroup
constexpr int RG_XP = 33;                // words per feature row of the staged points
constexpr int RG_MAXW = 4;               // waves per workgroup at most: 32 targets each

template <bool STD>
__global__ __launch_bounds__(64 * RG_MAXW) void regress_kernel(RegressArgs A) {
    extern __shared__ float rg_smem[];
    __shared__ int bad[RG_PTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int pt = lane & 31, half = lane >> 5;
    const int D = A.D, K = A.K, Tp = A.Tp;
    float *const xs = rg_smem;
    float *const os = rg_smem + D * RG_XP + wave * (RG_PTS * RG_XP);
    const int64_t i0 = (int64_t)blockIdx.x * RG_PTS;
    const int npt = A.n - i0 < RG_PTS ? (int)(A.n - i0) : RG_PTS;
    // ---- stage the points (rows past the end of the range: zeros)
    if (threadIdx.x < RG_PTS) bad[threadIdx.x] = 0;
    __syncthreads();
    for (int p = wave; p < RG_PTS; p += nw) {
        const float *row = A.X + (i0 + (p < npt ? p : 0)) * A.ldx;
        bool nf = false;
        for (int e = lane; e < D; e += 64) {
            const float v = p < npt ? row[e] : 0.f;
            nf = nf || !(fabsf(v) < INFINITY);
            xs[e * RG_XP + p] = v;
        }
        if (__ballot(nf) && lane == 0) bad[p] = 1;
    }
    __syncthreads();
    // ---- the point's row of the table: M, label, S (score_device.h)
    const int64_t i = i0 + pt;
    const bool valid = pt < npt;
    const float *col = A.table + (valid ? i : 0);      // (lanes past the end read point 0 and write nothing)
    const int64_t rs = A.stride;
    float m = -INFINITY;
    int best = 0;
    bool nan_seen = false;
    for (int k = 0; k < K; ++k) score_max_step(col[(int64_t)k * rs], k, m, best, nan_seen);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += score_e(col[(int64_t)k * rs], m);
    const bool part = valid && !nan_seen && m > -INFINITY && m < INFINITY && !bad[pt];
    const int tb = blockIdx.y * nw + wave;             // this wave's block of 32 targets
    if (blockIdx.y == 0 && wave == 0) {
        if (valid && half == 0 && A.labels) A.labels[i] = best + 1;
        const unsigned long long sm = __ballot(valid && half == 0 && !part);
        if (lane == 0) A.skip[blockIdx.x] += (unsigned)__popcll(sm);      // (this word has no other writer; launches of a stream are ordered)
    }
    if (tb * 32 >= Tp) return;                          // (a whole wave; no barrier below)
    const int t0 = tb * 32;
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
        const float p = part ? score_p(score_e(a, m), s) : 0.f;
        if (__ballot(p != 0.f) == 0) continue;
        const float *ck = A.c + (int64_t)k * Tp + t0 + 4 * half;
        rg_f32x16 acc;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 c4 = *reinterpret_cast<const float4 *>(ck + 8 * g);
            acc[4 * g] = c4.x; acc[4 * g + 1] = c4.y; acc[4 * g + 2] = c4.z; acc[4 * g + 3] = c4.w;
        }
        const float *bk = A.Bt + ((int64_t)k * D + half) * Tp + t0 + pt;
        const float *xk = xs + half * RG_XP + pt;
        int e = 0;
        for (; e + 8 <= D; e += 8) {                    // four steps at a time: the loads of all four in front of the first product
            const float b0 = bk[(int64_t)e * Tp], b1 = bk[(int64_t)(e + 2) * Tp], b2 = bk[(int64_t)(e + 4) * Tp], b3 = bk[(int64_t)(e + 6) * Tp];
            const float x0 = xk[e * RG_XP], x1 = xk[(e + 2) * RG_XP], x2 = xk[(e + 4) * RG_XP], x3 = xk[(e + 6) * RG_XP];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, x0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, x1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b2, x2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b3, x3, acc, 0, 0, 0);
        }
        for (; e < D; e += 2) {                         // the rest; an odd D: the second half's operands are zeros (feature D does not exist)
            const bool in = e + half < D;
            const float b = in ? bk[(int64_t)e * Tp] : 0.f;
            const float x = in ? xk[e * RG_XP] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b, x, acc, 0, 0, 0);
        }
        if (p != 0.f) {
            const double pd = (double)p;
            if constexpr (STD) {
                const double h = A.hd[2 * k], df = A.hd[2 * k + 1];
                double q = df * expm1(2.0 * (h - (double)a) / (df + dDo));
                q = q > 0.0 ? q : 0.0;
                const double sc = (df + q) / (df + dDo - 2.0);
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
    // ---- out through the wave's tile: word pt * 33 + target; then two points per trip, 32 consecutive targets each
    const float fnan = __uint_as_float(0x7fc00000u);
    const int nt = A.Dt - t0 < 32 ? A.Dt - t0 : 32;    // targets of this block that exist
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
            os[pt * RG_XP + 8 * (r >> 2) + 4 * half + (r & 3)] = part ? v : fnan;
        }
        __builtin_amdgcn_wave_barrier();               // (a wave's LDS instructions complete in order: the reads below see these writes)
        for (int p = half; p < npt; p += 2) {
            if (pt < nt) out[(i0 + p) * A.ld + t0 + pt] = os[p * RG_XP + pt];
        }
        __builtin_amdgcn_wave_barrier();
    }
    // ---- the padding columns [Dt, ld): zeros, by the wave that owns the last block of targets
    if (t0 + 32 >= Tp && A.ld > A.Dt) {
        const int64_t w = A.ld - A.Dt;
        for (int p = 0; p < npt; ++p)
            for (int64_t j = lane; j < w; j += 64) {
                A.mean[(i0 + p) * A.ld + A.Dt + j] = 0.f;
                if (STD) A.std[(i0 + p) * A.ld + A.Dt + j] = 0.f;
            }
    }
}

hipError_t launch_regress_range(const RegressArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.D < 1 || a.Dt < 1 || a.Tp % 32 || a.Tp < a.Dt || a.ld < a.Dt) return hipErrorInvalidValue;
    const int blocks = a.Tp / 32;
    const int nw = blocks < RG_MAXW ? blocks : RG_MAXW;
    const int64_t tiles = (a.n + RG_PTS - 1) / RG_PTS;
    if (tiles >> 31) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, (unsigned)((blocks + nw - 1) / nw));
    const size_t lds = sizeof(float) * ((size_t)a.D * RG_XP + (size_t)nw * RG_PTS * RG_XP);
    if (a.std) DPMM_LAUNCH((regress_kernel<true>), grid, dim3(64 * nw), lds, s, a);
    else DPMM_LAUNCH((regress_kernel<false>), grid, dim3(64 * nw), lds, s, a);
    return hipGetLastError();
}

}  // namespace dpmm
