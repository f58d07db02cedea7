// typicality.hip -- calibrated outlier scores (include/dpmm_hip_typicality.h, which states the definitions): behind the evaluation of a range
// of the score table (and the patch of missing.hip, if the ctx marginalises),
//   typ_class_kernel   lanes along i over the table: pass 1 of score_finish_kernel (batchstats_device.h) -- the label, NaN seen, M.  Writes
//                      the label and the point's class word: its 0-based cluster, or -1 for a skipped point (a NaN in its row or M not
//                      finite, the rule of overlap.hip); counts the skipped points, one integer atomic per wave.
//   typ_q_kernel       one wave per point, no workgroup barrier: lane l carries features / rows l, l + 64, .. as the kernels of missing.hip
//                      do.  A feature that is not finite makes the point incomplete (counted per wave, one integer atomic when the wave
//                      leaves).  Else z = x - m_k, y = R_k z by miss_rz (missing_device.h: the columns of R_k are coalesced rows of the
//                      transposed copy, Float32 FMAs in increasing column order), q = sum y^2: an FMA chain over the lane's NT values,
//                      then a butterfly over the wave.  Lane 0 writes q: one writer per point, and every operation on the point is fixed
//                      by the point and its cluster alone, so the bits do not depend on ranges, capacities or the grid.
//   typ_tail_kernel    one lane per point in Float64: typ_tail (typicality_math.h) of the Float32 q just written and df_k; rounded once.
//   typ_gap_kernel     (DPMM_OPT_TYPICALITY_GAPS, behind the three above, only where the range has a list of points with gaps) one wave per
//                      LISTED point, no workgroup barrier, r x r doubles of wave-private LDS as miss_patch_kernel: for the point's own
//                      cluster alone miss_system and miss_residual (missing_device.h) -- q_o = |y - C t|^2 with the bits that went into the
//                      patched table entry --, rounded once.  A listed point that is skipped, or has an observed feature that is not
//                      finite, is not touched.  Lane 0 overwrites the NaN words the passes above left (in `tail` it leaves D - r for the
//                      pass below); the wave counts its points, one integer atomic when it leaves.
//   typ_gap_tail_kernel   one lane per LISTED point in Float64, as typ_tail_kernel: typ_tail of the Float32 q_o at the D - r degrees of
//                      freedom typ_gap_kernel left in the word; rounded once.
// Skipped and incomplete points get q = tail = NaN.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"
#include "batchstats_device.h"
#include "missing_device.h"
#include "typicality_math.h"

namespace dpmm {

constexpr int TYP_WAVES = 4;      // waves per workgroup of the q kernel (they share nothing)

__global__ __launch_bounds__(256) void typ_class_kernel(TypicalityArgs A) {
    const int lane = threadIdx.x & 63;
    // (the 64 points of a trip belong to one wave: its trip count is uniform, the ballot sees whole waves)
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); base < A.n; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + lane;
        const bool valid = i < A.n;
        const float *col = A.table + (valid ? i : 0);      // (lanes past the end read point 0 and write nothing)
        float m, s;
        int best;
        bool nan_seen;
        bs_table_passes(col, A.stride, A.K, m, best, nan_seen, s);
        const bool scored = !nan_seen && m > -INFINITY && m < INFINITY;
        if (valid) {
            A.cls[i] = scored ? best : -1;
            if (A.labels) A.labels[i] = (int64_t)best + 1;
        }
        const unsigned long long sm = __ballot(valid && !scored);
        if (sm && lane == 0) atomicAdd(&A.cnt[0], (unsigned long long)__popcll(sm));
    }
}

__device__ __forceinline__ float typ_wave_sum(float v) {      // (a butterfly: every lane ends with the same bits)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

template <int NT>
__global__ __launch_bounds__(64 * TYP_WAVES) void typ_q_kernel(TypicalityArgs A) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = A.D;
    constexpr int Dp = 64 * NT;
    const int64_t nw = (int64_t)gridDim.x * TYP_WAVES;
    unsigned incomplete = 0;
    for (int64_t i = (int64_t)blockIdx.x * TYP_WAVES + wave; i < A.n; i += nw) {
        const int k = __builtin_amdgcn_readfirstlane(A.cls[i]);
        if (k < 0) {
            if (lane == 0) A.q[i] = NAN;
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
            if (lane == 0) A.q[i] = NAN;
            incomplete += 1;
            continue;
        }
        const float *const mk = A.mu + (int64_t)k * A.mu_step;
        float z[NT], y[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int j = 64 * t + lane;
            z[t] = j < D ? xv[t] - mk[j] : 0.f;
        }
        miss_rz<NT>(A.Rt + (int64_t)k * D * Dp, z, D, lane, y);
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) s = fmaf(y[t], y[t], s);
        s = typ_wave_sum(s);
        if (lane == 0) A.q[i] = s;
    }
    if (lane == 0 && incomplete) atomicAdd(&A.cnt[1], (unsigned long long)incomplete);
}

__global__ __launch_bounds__(256) void typ_tail_kernel(TypicalityArgs A) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < A.n; i += (int64_t)gridDim.x * 256) {
        const int k = A.cls[i];
        const float q = A.q[i];
        float t = NAN;
        if (k >= 0 && q == q) t = (float)typ_tail((double)q, A.cst[(int64_t)k * MISS_CST], A.D, nullptr);
        A.tail[i] = t;
    }
}

template <int NT>
__global__ __launch_bounds__(64 * TYP_WAVES) void typ_gap_kernel(TypicalityArgs A) {
    __shared__ double sA[TYP_WAVES][MISS_MAX * MISS_LDA];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *const Am = sA[wave];
    const int D = A.D;
    constexpr int Dp = 64 * NT;
    const unsigned long long total = A.list_cnt[0];
    const unsigned long long nw = (unsigned long long)gridDim.x * TYP_WAVES;
    unsigned scored = 0;
    for (unsigned long long e = (unsigned long long)blockIdx.x * TYP_WAVES + wave; e < total; e += nw) {
        const int64_t i = A.list[e];
        const int k = __builtin_amdgcn_readfirstlane(A.cls[i]);
        if (k < 0) continue;
        float xv[NT];
        unsigned long long nm[NT];
        int myM;
        const int r = miss_read_point<NT>(A.X + i * A.ldx, D, lane, xv, nm, myM);
        if (!miss_observed_finite<NT>(xv, nm, D, lane)) continue;      // (it stays incomplete)
        const float *const Rk = A.Rt + (int64_t)k * D * Dp;
        float y[NT];
        double gl;
        miss_system<NT>(Rk, A.mu + (int64_t)k * A.mu_step, xv, nm, myM, r, D, lane, Am, y, gl);
        miss_lds_fence();      // (the next point overwrites A)
        const float q = (float)miss_residual<NT>(Rk, y, gl, myM, r, lane);
        if (lane == 0) {
            A.q[i] = q;
            if (A.tail) A.tail[i] = q == q ? (float)(D - r) : NAN;      // (typ_gap_tail_kernel turns it into the tail)
        }
        scored += 1;
    }
    if (lane == 0 && scored) atomicAdd(&A.cnt[2], (unsigned long long)scored);
}

// A listed point that typ_gap_kernel did not score has a NaN in `tail` (typ_tail_kernel's) and keeps it.
__global__ __launch_bounds__(256) void typ_gap_tail_kernel(TypicalityArgs A) {
    const unsigned long long total = A.list_cnt[0];
    for (unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (unsigned long long)gridDim.x * 256) {
        const int64_t i = A.list[e];
        const int k = A.cls[i];
        const float d = A.tail[i];
        if (k >= 0 && d == d) A.tail[i] = (float)typ_tail((double)A.q[i], A.cst[(int64_t)k * MISS_CST], (int)d, nullptr);
    }
}

hipError_t launch_typicality_range(const TypicalityArgs &a, int max_grid, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.D < 1 || a.D > 256 || a.n > a.stride || a.ldx < a.D || !a.table || !a.X || !a.Rt || !a.mu || !a.cst || !a.cls || !a.q || !a.cnt)
        return hipErrorInvalidValue;
    DPMM_LAUNCH(typ_class_kernel, dim3((unsigned)std::min<int64_t>((a.n + 255) / 256, 4096)), dim3(256), 0, s, a);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((a.n + TYP_WAVES - 1) / TYP_WAVES, max_grid));
    const int nt = (a.D + 63) / 64;
    if (nt == 1) DPMM_LAUNCH((typ_q_kernel<1>), dim3(grid), dim3(64 * TYP_WAVES), 0, s, a);
    else if (nt == 2) DPMM_LAUNCH((typ_q_kernel<2>), dim3(grid), dim3(64 * TYP_WAVES), 0, s, a);
    else if (nt == 3) DPMM_LAUNCH((typ_q_kernel<3>), dim3(grid), dim3(64 * TYP_WAVES), 0, s, a);
    else DPMM_LAUNCH((typ_q_kernel<4>), dim3(grid), dim3(64 * TYP_WAVES), 0, s, a);
    if (a.tail) DPMM_LAUNCH(typ_tail_kernel, dim3((unsigned)std::min<int64_t>((a.n + 255) / 256, 4096)), dim3(256), 0, s, a);
    if (a.list) {      // the list's length is on the device: a grid for a range full of gaps, as launch_miss_patch
        if (!a.list_cnt || a.n > (int64_t)0xffffffffll) return hipErrorInvalidValue;
        const int ggrid = (int)std::max<int64_t>(1, std::min<int64_t>((a.n + TYP_WAVES - 1) / TYP_WAVES, max_grid / 4));
        if (nt == 1) DPMM_LAUNCH((typ_gap_kernel<1>), dim3(ggrid), dim3(64 * TYP_WAVES), 0, s, a);
        else if (nt == 2) DPMM_LAUNCH((typ_gap_kernel<2>), dim3(ggrid), dim3(64 * TYP_WAVES), 0, s, a);
        else if (nt == 3) DPMM_LAUNCH((typ_gap_kernel<3>), dim3(ggrid), dim3(64 * TYP_WAVES), 0, s, a);
        else DPMM_LAUNCH((typ_gap_kernel<4>), dim3(ggrid), dim3(64 * TYP_WAVES), 0, s, a);
        if (a.tail) DPMM_LAUNCH(typ_gap_tail_kernel, dim3((unsigned)std::min<int64_t>((a.n + 255) / 256, 4096)), dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace dpmm
