// score.hip -- the fused finish of scoring new points (include/dpmm_hip_score.h): from a slab of the table a_k(i) that the sweep kernels'
// table mode wrote (table[k * rstep * stride + i], i < n points of the slab) to labels, mixture log-density, the best m clusters and
// the probability matrix, whichever of them the call asked for.
//
// One thread per point, lanes along i: every read of table[k][i .. i + 63] is one coalesced 256-byte line, as in predict_finish_kernel
// (labels.hip), whose operations -- and therefore bits -- labels and probs repeat:
//   pass 1   M = max_k a_k (NaN skipped) and the label by Julia's argmax (the first NaN wins, else the first maximum);
//   pass 2   only if something beyond the labels is asked for: e_k = expf(a_k - M) (NaN -> -Inf first), S = sum in increasing k;
//            logdens = M + logf(S);
//   top m    a third walk over k with p_k = e_k / S -- the value probs holds -- inserted into m sorted registers.  MT (1, 2, 4, 8, 16)
//            is a template parameter and the insertion a fully unrolled chain of selects: an array indexed at run time would live
//            in scratch memory.  A slot is one 64-bit key ordered like (value descending, index ascending): equal values keep index order;
//   writes   probs[i][k] and top_*[i][j] are row-major in i: written straight from the lanes they would be K (m) elements apart.
//            They go through a wave-private LDS tile of 64 points x 64 clusters and leave it in the order of the output: the wave's
//            64 rows are one contiguous range (K <= 64), else 256-byte row segments.  A tile row has c | 1 words for c columns in
//            use (65 for 64 clusters -- tensor_io.hip's feature-major tile -- K | 1 for fewer, MT | 1 for the top m, MT / 2 < m <= MT).  Write side:
//            lane i writes word (c | 1) i + k, an odd stride, so the 64 lanes fall into 64 banks.  Read side: element f of the
//            output sits at word f (c odd) or f + f / c (c even): the lanes read consecutive words with a one-word step every c
//            lanes, 64 + 64 / c words in all (the top m: fewer than 128), so a bank is met twice at most -- with 65-word rows whatever c is, K = 5 read five
//            rows through one bank.  The division by S happens at that read (same operands, same bits; sS[r] is one word per
//            row, broadcast to the lanes of the row); the row / column of a lane advance incrementally, one integer division
//            per 64 clusters.
// The slab was written by the launch in front on the same stream and is read two to four times: it is sized (DPMM_OPT_SCORE_TABLE_MB)
// to stay in the last-level cache between the passes.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"

namespace dpmm {

constexpr int SC_WAVES = 2;              // waves per workgroup: 2 x 64 x 65 words of LDS = 33 KB, four workgroups per CU
constexpr int SC_ROW = 65;               // words per tile row at most (64 clusters | 1)
constexpr int SC_TOPI = 64 * 17;         // first word of the top-m indices (rows of at most 16 | 1 words in front)

template <int MT, bool PROBS>
__global__ __launch_bounds__(64 * SC_WAVES) void score_finish_kernel(ScoreArgs A) {
    constexpr bool LDS = PROBS || MT > 0;
    __shared__ float tile[LDS ? SC_WAVES * 64 * SC_ROW : 1];
    __shared__ float sums[LDS ? SC_WAVES * 64 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *const tw = tile + (LDS ? wave * 64 * SC_ROW : 0);
    float *const sS = sums + (LDS ? wave * 64 : 0);
    const int K = A.K;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    const bool pass2 = LDS || A.logdens != nullptr;
    // (the trip count is the same for every thread of the workgroup: the barriers below are uniform)
    for (int64_t base = (int64_t)blockIdx.x * (64 * SC_WAVES); base < A.n; base += (int64_t)gridDim.x * (64 * SC_WAVES)) {
        const int64_t i0 = base + (int64_t)wave * 64;
        const int64_t i = i0 + lane;
        const bool valid = i < A.n;
        const int npt = i0 < A.n ? (int)(A.n - i0 < 64 ? A.n - i0 : 64) : 0;      // points of this wave
        const float *col = A.table + (valid ? i : 0);                              // (lanes past the end read point 0 and write nothing)
        // ---- pass 1: maximum and label
        float m = -INFINITY;
        int best = 0;
        bool nan_seen = false;
        for (int k = 0; k < K; ++k) {
            const float a = col[(int64_t)k * rs];
            if (a != a) {
                if (!nan_seen) { nan_seen = true; best = k; }
            } else if (a > m) {
                m = a;
                if (!nan_seen) best = k;
            }
        }
        if (valid && A.labels) A.labels[i] = best + 1;
        if (!pass2) continue;
        // ---- pass 2: e_k and their sum (K <= 64 with probs: the e_k go to the tile on the way)
        float s = 0.f;
        for (int k = 0; k < K; ++k) {
            const float e = score_e(col[(int64_t)k * rs], m);
            if (PROBS && K <= 64) tw[lane * (K | 1) + k] = e;
            s += e;
        }
        if (valid && A.logdens) A.logdens[i] = (m == -INFINITY) ? -INFINITY : m + logf(s);
        // ---- the best MT probabilities, in registers
        // key of a probability p >= 0 of cluster k: (bits(p) + 1) << 32 | ~k -- as unsigned integers the keys order like (p descending, k
        // ascending); an empty slot j is 0 << 32 | ~j, below every real key.  One register pair per slot, max / min instead of flags.
        unsigned long long tk[MT > 0 ? MT : 1];
        float tv[MT > 0 ? MT : 1];
        if constexpr (MT > 0) {
#pragma unroll
            for (int j = 0; j < MT; ++j) tk[j] = (unsigned long long)(~(unsigned)j);
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const float p = score_p(score_e(col[(int64_t)k * rs], m), s);
                // (a NaN -- the whole row is then NaN -- is never inserted: key 0 ranks below every slot)
                unsigned long long key = (p == p) ? (((unsigned long long)(__float_as_uint(p) + 1u) << 32) | (unsigned long long)(~(unsigned)k)) : 0ull;
#pragma unroll
                for (int j = 0; j < MT; ++j) {      // the carried key moves in where it ranks higher; the displaced one is carried on
                    const unsigned long long t = tk[j];
                    tk[j] = key > t ? key : t;
                    key = key > t ? t : key;
                }
            }
#pragma unroll
            for (int j = 0; j < MT; ++j) tv[j] = __uint_as_float((unsigned)(tk[j] >> 32) - 1u);
            if (s != s) {      // no finite entry: every probability is NaN and none was inserted -- indices 0 .. m - 1 with the NaNs probs holds
#pragma unroll 1
                for (int k = 0; k < K && k < MT; ++k) {      // (a rolled loop: sixteen unrolled row offsets cost the kernel its scalar registers)
                    const float p = score_p(score_e(col[(int64_t)k * rs], m), s);
#pragma unroll
                    for (int j = 0; j < MT; ++j) tv[j] = (j == k) ? p : tv[j];
                }
            }
        }
        // ---- probs: 64 clusters at a time through the tile
        if constexpr (PROBS) {
            sS[lane] = s;
            for (int k0 = 0; k0 < K; k0 += 64) {
                const int kc = K - k0 < 64 ? K - k0 : 64;
                const int sr = kc | 1;                     // words per tile row: odd (lanes writing column kk of their rows meet in no bank) and as
                                                           // close to kc as that allows, so that the read below walks consecutive words
                if (K > 64) {
                    __syncthreads();                       // the previous 64 clusters have left the tile
                    for (int kk = 0; kk < kc; ++kk) {
                        tw[lane * sr + kk] = score_e(col[(int64_t)(k0 + kk) * rs], m);
                    }
                }
                __syncthreads();
                // element f of the wave's npt x kc block: row r = f / kc, cluster kk = f % kc; f advances by 64 per trip
                int r = lane / kc, kk = lane - r * kc;
                const int dr = 64 / kc, dk = 64 - dr * kc;
                const int total = npt * kc;
                for (int f = lane; f < total; f += 64) {
                    A.probs[(i0 + r) * (int64_t)K + k0 + kk] = score_p(tw[r * sr + kk], sS[r]);
                    r += dr; kk += dk;
                    if (kk >= kc) { kk -= kc; ++r; }
                }
            }
        }
        // ---- top m: the values in rows of MT | 1 words from word 0, the indices in rows of the same length from word SC_TOPI
        if constexpr (MT > 0) {
            if (PROBS) __syncthreads();                    // the probabilities have left the tile
            const int mm = A.m;                            // MT / 2 < mm <= MT
            constexpr int sr = MT | 1;                     // (the rows are MT | 1 words, not m | 1: a guard per slot costs the widest kernel its scalar registers)
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                tw[lane * sr + j] = tv[j];
                tw[SC_TOPI + lane * sr + j] = __uint_as_float(~(unsigned)tk[j]);
            }
            __syncthreads();
            int r = lane / mm, j = lane - r * mm;
            const int dr = 64 / mm, dj = 64 - dr * mm;
            const int total = npt * mm;
            for (int f = lane; f < total; f += 64) {
                const int64_t o = (i0 + r) * (int64_t)mm + j;
                if (A.top_prob) A.top_prob[o] = tw[r * sr + j];
                if (A.top_idx) A.top_idx[o] = (int64_t)__float_as_int(tw[SC_TOPI + r * sr + j]) + 1;
                r += dr; j += dj;
                if (j >= mm) { j -= mm; ++r; }
            }
        }
        if constexpr (LDS) __syncthreads();                // the tile is refilled by the next trip
    }
}

template <int MT>
static void launch_mt(const ScoreArgs &a, int grid, hipStream_t s) {
    if (a.probs) DPMM_LAUNCH((score_finish_kernel<MT, true>), dim3(grid), dim3(64 * SC_WAVES), 0, s, a);
    else DPMM_LAUNCH((score_finish_kernel<MT, false>), dim3(grid), dim3(64 * SC_WAVES), 0, s, a);
}

hipError_t launch_score_finish(const ScoreArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.m < 0 || a.m > 16 || a.K < 1) return hipErrorInvalidValue;
    int64_t g = (a.n + 64 * SC_WAVES - 1) / (64 * SC_WAVES);
    if (g > 2048) g = 2048;
    const int grid = (int)g;
    if (a.m == 0) launch_mt<0>(a, grid, s);
    else if (a.m == 1) launch_mt<1>(a, grid, s);
    else if (a.m == 2) launch_mt<2>(a, grid, s);
    else if (a.m <= 4) launch_mt<4>(a, grid, s);
    else if (a.m <= 8) launch_mt<8>(a, grid, s);
    else launch_mt<16>(a, grid, s);
    return hipGetLastError();
}

}  // namespace dpmm
