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
//   regress_draw_kernel        the shape of regress.hip: a workgroup owns RD_PTS = 32 points and a block of up to 4 x 32 targets, one wave
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
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"
#include "sample_device.h"

namespace dpmm {

typedef float rd_f32x16 __attribute__((ext_vector_type(16)));

constexpr int RD_PTS = 32;               // points per workgroup
constexpr int RD_XP = 33;                // words per row of the staged images
constexpr int RD_MAXW = 4;               // waves per workgroup at most: 32 targets each
constexpr size_t RD_MAX_LDS = 65536;

__global__ __launch_bounds__(256) void regress_draw_scale_kernel(const float *table, int64_t rs, int64_t n, int K, double dDo, const double *hd, uint64_t seed,
                                                                 int64_t gi0, int64_t draw0, int ndraws, int32_t *kcs, float *scs) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *col = table + i;
    float m = -INFINITY;
    int best = 0;
    bool nan_seen = false;
    for (int k = 0; k < K; ++k) score_max_step(col[(int64_t)k * rs], k, m, best, nan_seen);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += score_e(col[(int64_t)k * rs], m);
    const bool part = !nan_seen && m > -INFINITY && m < INFINITY;
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
            const double h = hd[2 * kc], df = hd[2 * kc + 1];
            double q = df * expm1(2.0 * (h - (double)col[(int64_t)kc * rs]) / (df + dDo));
            q = q > 0.0 ? q : 0.0;
            const double g = sample_chi2(df + dDo, seed, gi, STREAM_REGRESS_CHI, b0);
            sc = (float)sqrt((df + q) / g);
        }
        kcs[(int64_t)jd * n + i] = kc;
        scs[(int64_t)jd * n + i] = sc;
    }
}

__global__ __launch_bounds__(64 * RD_MAXW) void regress_draw_kernel(RegressDrawArgs A) {
    extern __shared__ float rd_smem[];
    __shared__ int bad[RD_PTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int pt = lane & 31, half = lane >> 5;
    const int D = A.D, Dt = A.Dt, K = A.K, Tp = A.Tp;
    const int nb4 = (Dt + 3) >> 2;                       // Philox blocks of the normals of a draw
    float *const xs = rd_smem;
    float *const ns = rd_smem + D * RD_XP;
    float *const os = ns + 4 * nb4 * RD_XP + wave * (RD_PTS * RD_XP);
    const int64_t i0 = (int64_t)blockIdx.x * RD_PTS;
    const int npt = A.n - i0 < RD_PTS ? (int)(A.n - i0) : RD_PTS;
    // ---- stage the points (rows past the end of the range: zeros)
    if (threadIdx.x < RD_PTS) bad[threadIdx.x] = 0;
    __syncthreads();
    for (int p = wave; p < RD_PTS; p += nw) {
        const float *row = A.X + (i0 + (p < npt ? p : 0)) * A.ldx;
        bool nf = false;
        for (int e = lane; e < D; e += 64) {
            const float v = p < npt ? row[e] : 0.f;
            nf = nf || !(fabsf(v) < INFINITY);
            xs[e * RD_XP + p] = v;
        }
        if (__ballot(nf) && lane == 0) bad[p] = 1;
    }
    __syncthreads();
    const int64_t i = i0 + pt;
    const bool valid = pt < npt;
    const int64_t iv = valid ? i : 0;                   // (lanes past the end read point 0 and write nothing)
    const bool part = valid && A.kc[iv] >= 0 && !bad[pt];      // (a row of the table takes part in every draw or in none)
    const int tb = blockIdx.y * nw + wave;             // this wave's block of 32 targets
    const int t0 = tb * 32;
    const bool active = t0 < Tp;                        // (a wave without targets still serves the normals and the barriers)
    if (blockIdx.y == 0 && wave == 0 && A.skip) {
        const unsigned long long sm = __ballot(valid && half == 0 && !part);
        if (lane == 0) A.skip[blockIdx.x] += (unsigned)__popcll(sm);      // (this word has no other writer; launches of a stream are ordered)
    }
    const uint64_t gi = (uint64_t)(A.i0 + i);
    const int b_lo = blockIdx.y * nw * 8;               // the first block of normals this workgroup's targets meet a non-zero of W in
    const float fnan = __uint_as_float(0x7fc00000u);
    const int nt = Dt - t0 < 32 ? Dt - t0 : 32;         // targets of this wave's block that exist
    const int ndraws = A.ndraws;
#pragma unroll 1
    for (int jd = 0; jd < ndraws; ++jd) {
        const uint32_t b0 = 64u * (uint32_t)(A.draw0 + jd);
        const int kc = part ? A.kc[(int64_t)jd * A.n + iv] : -1;
        const float sc = part ? A.sc[(int64_t)jd * A.n + iv] : 0.f;
        // ---- s n of this lane's point: coordinate a is word a & 3 of block a >> 2, Box-Muller as miss_draw_kernel
        __syncthreads();
        for (int b = b_lo + 2 * wave + half; b < nb4; b += 2 * nw) {
            const Philox4 rn = philox4x32_10(A.seed, gi, b0 + (uint32_t)b, STREAM_REGRESS_NORMAL);
            const float r0 = sqrtf(fmaxf(-2.0f * __logf(sample_u32(rn.v[0])), 0.0f)), r1 = sqrtf(fmaxf(-2.0f * __logf(sample_u32(rn.v[2])), 0.0f));
            const float th0 = 6.2831853071795865f * sample_u32(rn.v[1]), th1 = 6.2831853071795865f * sample_u32(rn.v[3]);
            float *const nb = ns + 4 * b * RD_XP + pt;
            nb[0] = sc * (r0 * __cosf(th0));
            nb[RD_XP] = sc * (r0 * __sinf(th0));
            nb[2 * RD_XP] = sc * (r1 * __cosf(th1));
            nb[3 * RD_XP] = sc * (r1 * __sinf(th1));
        }
        __syncthreads();
        if (active) {
            // ---- the clusters some point of the tile drew
            rd_f32x16 res;
#pragma unroll
            for (int r = 0; r < 16; ++r) res[r] = 0.f;
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                if (__ballot(kc == k) == 0) continue;
                const float *ck = A.c + (int64_t)k * Tp + t0 + 4 * half;
                rd_f32x16 acc;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 c4 = *reinterpret_cast<const float4 *>(ck + 8 * g);
                    acc[4 * g] = c4.x; acc[4 * g + 1] = c4.y; acc[4 * g + 2] = c4.z; acc[4 * g + 3] = c4.w;
                }
                const float *bk = A.Bw + ((int64_t)k * (D + Dt) + half) * Tp + t0 + pt;
                const float *xk = xs + half * RD_XP + pt;
                int e = 0;
                for (; e + 8 <= D; e += 8) {                    // four steps at a time: the loads of all four in front of the first product
                    const float w0 = bk[e * Tp], w1 = bk[(e + 2) * Tp], w2 = bk[(e + 4) * Tp], w3 = bk[(e + 6) * Tp];
                    const float x0 = xk[e * RD_XP], x1 = xk[(e + 2) * RD_XP], x2 = xk[(e + 4) * RD_XP], x3 = xk[(e + 6) * RD_XP];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, x0, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, x1, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w2, x2, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w3, x3, acc, 0, 0, 0);
                }
                for (; e < D; e += 2) {                         // the rest; an odd D: the second half's operands are zeros (feature D does not exist)
                    const bool in = e + half < D;
                    const float w = in ? bk[e * Tp] : 0.f;
                    const float x = in ? xk[e * RD_XP] : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w, x, acc, 0, 0, 0);
                }
                const float *wk = bk + D * Tp;         // the rows of W': coordinate a at wk[a * Tp]
                const float *nk = ns + half * RD_XP + pt;
                int a = t0;                                     // (W_k[d][a] = 0 for a < d, and d >= t0 here)
                for (; a + 8 <= Dt; a += 8) {
                    const float w0 = wk[a * Tp], w1 = wk[(a + 2) * Tp], w2 = wk[(a + 4) * Tp], w3 = wk[(a + 6) * Tp];
                    const float x0 = nk[a * RD_XP], x1 = nk[(a + 2) * RD_XP], x2 = nk[(a + 4) * RD_XP], x3 = nk[(a + 6) * RD_XP];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, x0, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, x1, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w2, x2, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w3, x3, acc, 0, 0, 0);
                }
                for (; a < Dt; a += 2) {
                    const bool in = a + half < Dt;
                    const float w = in ? wk[a * Tp] : 0.f;
                    const float x = in ? nk[a * RD_XP] : 0.f;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w, x, acc, 0, 0, 0);
                }
                if (kc == k) res = acc;
            }
            // ---- out through the wave's tile: word pt * 33 + target; then two points per trip, 32 consecutive targets each
            const int64_t ld = A.ld, width = ld < A.draw_stride ? ld : A.draw_stride;
            float *const out = A.out + (int64_t)jd * A.draw_stride;
#pragma unroll
            for (int r = 0; r < 16; ++r) os[pt * RD_XP + 8 * (r >> 2) + 4 * half + (r & 3)] = part ? res[r] : fnan;
            __builtin_amdgcn_wave_barrier();               // (a wave's LDS instructions complete in order: the reads below see these writes)
            for (int p = half; p < npt; p += 2) {
                if (pt < nt) out[(i0 + p) * ld + t0 + pt] = os[p * RD_XP + pt];
            }
            __builtin_amdgcn_wave_barrier();
            // ---- the padding columns [Dt, width): zeros, by the wave that owns the last block of targets
            if (t0 + 32 >= Tp && width > Dt) {
                const int64_t w = width - Dt;
                for (int p = 0; p < npt; ++p)
                    for (int64_t j = lane; j < w; j += 64) out[(i0 + p) * ld + Dt + j] = 0.f;
            }
        }
        if (A.comp && blockIdx.y == 0 && wave == 0 && half == 0 && valid) A.comp[(int64_t)jd * A.comp_stride + i] = kc;
    }
}

hipError_t launch_regress_draw_range(const RegressDrawArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.ndraws <= 0) return hipSuccess;
    const int64_t width = a.ld < a.draw_stride ? a.ld : a.draw_stride;
    if (a.K < 1 || a.D < 1 || a.Dt < 1 || a.Dt > REGRESS_MAX_TARGETS || a.Tp != regress_pitch(a.Dt) || !a.out || width < a.Dt || a.i0 < 0 || a.draw0 < 0 ||
        a.draw0 + a.ndraws > REGRESS_DRAW_MAX || !a.kc || !a.sc || a.n > a.stride)
        return hipErrorInvalidValue;
    const int blocks = a.Tp / 32;
    const int nw = blocks < RD_MAXW ? blocks : RD_MAXW;
    const int64_t tiles = (a.n + RD_PTS - 1) / RD_PTS;
    if (tiles >> 31) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, (unsigned)((blocks + nw - 1) / nw));
    const size_t lds = sizeof(float) * ((size_t)a.D * RD_XP + (size_t)4 * ((a.Dt + 3) / 4) * RD_XP + (size_t)nw * RD_PTS * RD_XP);
    if (lds > RD_MAX_LDS) return hipErrorInvalidValue;      // (dpmm_set_regression_factor refuses D_o + D_t > 256: at most 51 KiB)
    DPMM_LAUNCH(regress_draw_scale_kernel, dim3((unsigned)((a.n + 255) / 256)), dim3(256), 0, s, a.table, a.stride, a.n, a.K, (double)a.D, a.hd, a.seed,
                a.i0, a.draw0, a.ndraws, a.kc, a.sc);
    DPMM_LAUNCH(regress_draw_kernel, grid, dim3(64 * nw), lds, s, a);
    return hipGetLastError();
}

}  // namespace dpmm
