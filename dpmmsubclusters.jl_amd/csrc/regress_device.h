// regress_device.h -- the tile the kernels of regress.hip and regress_draw.hip share.  (regress_cdf.hip keeps its own copy of these statements,
// rc_stage .. rc_flush: its two kernels sit at the register limit, and moving them onto this header cost the quantile kernel scalar spills
// and both kernels 0.2 to 0.65 % of their time.)
//
// A workgroup owns RT_PTS = 32 points of the range and a block of up to 4 x 32 targets, one wave per 32 targets:
//   stage    the 32 points, transposed, into LDS (xs[e * 33 + p]: the read of X is coalesced along e, the odd pitch spreads the writes over
//            the banks); a point with a feature that is not finite is flagged;
//   row      lane l walks the table row of point p = l & 31 (both halves of the wave: the same statements on the same words) with the
//            functions of score_device.h: M, the label, S -- hence p_ik = e_k / S with the bits `probs` holds;
//   chain    a cluster costs one v_mfma_f32_32x32x2_f32 per two rows of its transposed matrix: A operand the matrix (lane l: row
//            e + (l >> 5), column t0 + (l & 31), 128-byte lines), B operand an LDS image (word (e + (l >> 5)) * 33 + (l & 31)), accumulator
//            started from c_k -- an exact Float32 fused-multiply-add chain in increasing e.  Lane l then holds the result for point l & 31
//            and the 16 targets t0 + rt_target(r, l >> 5);
//   flush    through a wave-private LDS tile of 32 x 33 words, so that the 32 targets of a point leave as one 128-byte segment; the padding
//            columns behind the targets are zeroed by the wave that owns the last block of targets.
// One writer per output word, no atomics; the points that take no part are counted per tile, in a word only this workgroup's block 0
// writes (the host adds the words up).
#pragma once
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"

namespace dpmm {

typedef float rt_f32x16 __attribute__((ext_vector_type(16)));

constexpr int RT_PTS = 32;               // points per workgroup
constexpr int RT_XP = 33;                // words per row of a staged image and of a wave's output tile
constexpr int RT_MAXW = 4;               // waves per workgroup at most: 32 targets each

// the target, from the wave's first, that element r of a lane's accumulator belongs to
__device__ __forceinline__ int rt_target(int r, int half) { return 8 * (r >> 2) + 4 * half + (r & 3); }

// the staged points: xs[e * 33 + p], zeros past the end of the range; bad[p]: a feature of point p is not finite.  Ends with a barrier.
__device__ __forceinline__ void rt_stage(const float *X, int64_t ldx, int64_t i0, int npt, int D, float *xs, int *bad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (threadIdx.x < RT_PTS) bad[threadIdx.x] = 0;
    __syncthreads();
    for (int p = wave; p < RT_PTS; p += nw) {
        const float *row = X + (i0 + (p < npt ? p : 0)) * ldx;
        bool nf = false;
        for (int e = lane; e < D; e += 64) {
            const float v = p < npt ? row[e] : 0.f;
            nf = nf || !(fabsf(v) < INFINITY);
            xs[e * RT_XP + p] = v;
        }
        if (__ballot(nf) && lane == 0) bad[p] = 1;
    }
    __syncthreads();
}

// The table row of the lane's point (col: its first entry; lanes past the end of the range read point 0 and write nothing): M, the label, S
struct RtRow {
    float m, s;
    int best;
    bool part;           // the point takes part: a row without NaN and with a finite entry, finite features
};
__device__ __forceinline__ RtRow rt_row(const float *col, int64_t rs, int K, bool valid, bool bad) {
    RtRow w;
    w.m = -INFINITY;
    w.best = 0;
    bool nan_seen = false;
    for (int k = 0; k < K; ++k) score_max_step(col[(int64_t)k * rs], k, w.m, w.best, nan_seen);
    w.s = 0.f;
    for (int k = 0; k < K; ++k) w.s += score_e(col[(int64_t)k * rs], w.m);
    w.part = valid && !nan_seen && w.m > -INFINITY && w.m < INFINITY && !bad;
    return w;
}

// the points of the tile that take no part, added to the tile's word: by wave 0 of the workgroups with blockIdx.y == 0 (the word has no
// other writer; launches of a stream are ordered)
__device__ __forceinline__ void rt_count_skipped(unsigned *skip, bool valid, bool part, int lane) {
    const unsigned long long sm = __ballot(valid && lane < 32 && !part);
    if (lane == 0) skip[blockIdx.x] += (unsigned)__popcll(sm);
}

// what the row gives beside the targets, by the same wave: the label of point i, and the count
__device__ __forceinline__ void rt_row_out(const RegressTile &T, int64_t i, bool valid, const RtRow &w, int lane) {
    if (blockIdx.y != 0 || threadIdx.x >= 64) return;
    if (valid && lane < 32 && T.labels) T.labels[i] = w.best + 1;
    rt_count_skipped(T.skip, valid, w.part, lane);
}

// c_k as the accumulator of the lane: the 16 targets t0 + rt_target(r, half)
__device__ __forceinline__ rt_f32x16 rt_chain_start(const float *c, int k, int Tp, int t0, int half) {
    const float *ck = c + (int64_t)k * Tp + t0 + 4 * half;
    rt_f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 c4 = *reinterpret_cast<const float4 *>(ck + 8 * g);
        acc[4 * g] = c4.x; acc[4 * g + 1] = c4.y; acc[4 * g + 2] = c4.z; acc[4 * g + 3] = c4.w;
    }
    return acc;
}

// acc continued over the rows [from, to) of a transposed matrix (mt: row 0, Tp floats a row, at the wave's first target) against the LDS
// image img (row e at img[e * 33]), in increasing row: four steps at a time, the loads of all four in front of the first product, then
// the rest two rows at a time; a row `to` that does not exist meets zero operands.  The offset of a row is formed in the type Tp comes in
// (a cluster's matrix is below 2^17 floats): int64_t in regress.hip, int in regress_draw.hip, each as its chains had it -- with 64-bit
// offsets the draws' kernel needs 110 vector registers for 73 and loses a wave per SIMD, with int ones regress_kernel is other code.
template <class Index>
__device__ __forceinline__ rt_f32x16 rt_chain(rt_f32x16 acc, const float *mt, Index Tp, const float *img, int from, int to, int pt, int half) {
    const float *bk = mt + half * Tp + pt;
    const float *xk = img + half * RT_XP + pt;
    int e = from;
    for (; e + 8 <= to; e += 8) {
        const float b0 = bk[e * Tp], b1 = bk[(e + 2) * Tp], b2 = bk[(e + 4) * Tp], b3 = bk[(e + 6) * Tp];
        const float x0 = xk[e * RT_XP], x1 = xk[(e + 2) * RT_XP], x2 = xk[(e + 4) * RT_XP], x3 = xk[(e + 6) * RT_XP];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, x0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, x1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b2, x2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b3, x3, acc, 0, 0, 0);
    }
    for (; e < to; e += 2) {
        const bool in = e + half < to;
        const float b = in ? bk[e * Tp] : 0.f;
        const float x = in ? xk[e * RT_XP] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b, x, acc, 0, 0, 0);
    }
    return acc;
}

// q_ik, the squared distance of the given features, recovered from the table entry a of a cluster with the constants h and df
__device__ __forceinline__ double rt_q(double h, double df, float a, double dDo) {
    const double q = df * expm1(2.0 * (h - (double)a) / (df + dDo));
    return q > 0.0 ? q : 0.0;
}

// element r of the lane into the wave's tile os (word point * 33 + target)
__device__ __forceinline__ void rt_put(float *os, int r, int pt, int half, float v) { os[pt * RT_XP + rt_target(r, half)] = v; }

// rows of `out` for the points of the tile from the wave's tile, two points per trip, 32 consecutive targets each (a wave's LDS
// instructions complete in order: the reads see the writes in front of the barrier)
__device__ __forceinline__ void rt_flush(float *out, int64_t row0, int64_t ld, const float *os, int npt, int nt, int t0, int pt, int half) {
    __builtin_amdgcn_wave_barrier();
    for (int p = half; p < npt; p += 2)
        if (pt < nt) out[(row0 + p) * ld + t0 + pt] = os[p * RT_XP + pt];
    __builtin_amdgcn_wave_barrier();
}

// the padding columns [Dt, width) of the tile's rows: zeros, by the wave that owns the last block of targets
__device__ __forceinline__ void rt_zero_pad(float *out, int64_t row0, int64_t ld, int npt, int Dt, int64_t width, int lane) {
    for (int p = 0; p < npt; ++p)
        for (int64_t j = Dt + lane; j < width; j += 64) out[(row0 + p) * ld + j] = 0.f;
}

// the grid of a launch: x tiles of points, y blocks of up to RT_MAXW x 32 targets, nw waves per workgroup
struct RtGrid {
    dim3 grid;
    int nw;
};
inline RtGrid rt_grid(const RegressTile &t) {
    const int blocks = t.Tp / 32;
    const int nw = blocks < RT_MAXW ? blocks : RT_MAXW;
    return {dim3((unsigned)((t.n + RT_PTS - 1) / RT_PTS), (unsigned)((blocks + nw - 1) / nw)), nw};
}

}  // namespace dpmm
