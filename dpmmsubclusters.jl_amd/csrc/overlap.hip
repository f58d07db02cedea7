// overlap.hip -- the posterior overlap of the clusters (include/dpmm_hip_overlap.h): O[k][j] = sum_i p_ik p_ij, mass[k] = sum_i p_ik,
// count and skipped, from a range of the table a_k(i) that the sweep kernels' table mode wrote (table[k * rstep * stride + i], as
// score.hip reads it).  p_ik is the Float32 probability score.hip writes, formed with the same functions (score_device.h), widened to
// Float64; the sums are Float64 on the matrix pipe (v_mfma_f64_16x16x4_f64, operand layout as in suffstats.hip).
//
// Three launches per range, nothing in them waits for another workgroup:
//   prep      one thread per point, lanes along i (every read of table[k][i .. i + 63] is one coalesced 256-byte line): passes 1 and 2 of
//             score_finish_kernel -- M, the label, NaN seen, S -- written as one float2 per point, S = 0 for a point that takes no part
//             (S >= 1 for one that does: the entry at the maximum adds expf(0)).  count and skipped are integer adds in LDS, flushed to
//             one of RANK_REPL replicas of the global counters: sums of integers, order-free.
//   contract  the range is cut into nchunk chunks of whole 64-point batches, the rows into blocks of 64; a workgroup of four waves owns
//             (chunk, pair of row blocks ba >= bb) and writes its 64 x 64 block of partial sums -- one writer, no atomics.  Per batch of 64
//             points: lane = point, wave w converts rows w, w + 4, .. of both blocks to p (rows beyond K and points that take no part or lie
//             beyond the range: 0, from clamped addresses, never an out-of-bounds read) and stores them as Float32 to LDS, row-major
//             with 68 words per row; then wave w accumulates the four 16 x 16 tiles of tile row w over the batch's 16 k-steps of 4 points.
//             Operands of a k-step s: lane (i = lane & 15, g = lane >> 4) supplies A[row i][k = g] = p[16 w + i][4 s + g] and
//             B[k = g][col i] = p[16 tb + i][4 s + g], element r of the result is row g + 4 r, column i.  A lane reads word
//             68 (16 t + i) + 4 s + g: bank 4 i + g (mod 64), the 64 lanes in 64 banks; a wave writes 64 consecutive words.  The
//             widening to Float64 happens at that read (5 conversions per 4 or 5 matrix instructions).  On a diagonal pair the tiles
//             above the diagonal are left out and one more instruction per k-step, against a column of ones, gives the row sums: mass.
//   reduce    one thread per entry of the lower triangle: the chunks' partials added in increasing chunk order, then added to the
//             accumulator and the sum written to [k][j] and [j][k] -- symmetric bit for bit.  The mass rows likewise.
// nchunk depends on the range's length and K alone (overlap_chunks), so the order of every addition is fixed by the call sequence.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"

namespace dpmm {

typedef double ov_f64x4 __attribute__((ext_vector_type(4)));

constexpr int OV_THREADS = 256;
constexpr int OV_PITCH = 68;             // words per LDS row of 64 points: = 4 (mod 64)

__global__ __launch_bounds__(OV_THREADS) void overlap_prep_kernel(OverlapArgs A) {
    __shared__ unsigned cnt[DPMM_MAX_CLUSTERS_K];
    __shared__ unsigned skipped;
    const int K = A.K, tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < K; k += OV_THREADS) cnt[k] = 0;
    if (tid == 0) skipped = 0;
    __syncthreads();
    const int64_t rs = (int64_t)A.rstep * A.stride;
    // (the trip count is the same for every thread of the workgroup: the ballots below see whole waves)
    for (int64_t base = (int64_t)blockIdx.x * OV_THREADS; base < A.n; base += (int64_t)gridDim.x * OV_THREADS) {
        const int64_t i = base + tid;
        const bool valid = i < A.n;
        const float *col = A.table + (valid ? i : 0);      // (lanes past the end read point 0 and contribute nothing)
        float m = -INFINITY;
        int best = 0;
        bool nan_seen = false;
        for (int k = 0; k < K; ++k) score_max_step(col[(int64_t)k * rs], k, m, best, nan_seen);
        float s = 0.f;
        for (int k = 0; k < K; ++k) s += score_e(col[(int64_t)k * rs], m);
        const bool part = valid && !nan_seen && m > -INFINITY && m < INFINITY;
        if (valid) A.ms[i] = part ? make_float2(m, s) : make_float2(0.f, 0.f);
        // ---- count and skipped (as rank_filter_kernel)
        const unsigned long long pm = __ballot(part);
        if (pm) {
            const int first = __ffsll((long long)pm) - 1;
            const int k0 = __shfl(best, first);
            if (__ballot(part && best != k0) == 0) {
                if (lane == first) atomicAdd(&cnt[k0], (unsigned)__popcll(pm));
            } else if (part) {
                atomicAdd(&cnt[best], 1u);
            }
        }
        const unsigned long long sm = __ballot(valid && !part);
        if (sm && lane == 0) atomicAdd(&skipped, (unsigned)__popcll(sm));
    }
    __syncthreads();
    unsigned long long *count = A.count + (int64_t)(blockIdx.x % RANK_REPL) * (K + 1);
    for (int k = tid; k < K; k += OV_THREADS)
        if (cnt[k]) atomicAdd(&count[k], (unsigned long long)cnt[k]);
    if (tid == 0 && skipped) atomicAdd(&count[K], (unsigned long long)skipped);
}

// pair p of the lower block triangle, p = ba (ba + 1) / 2 + bb, ba >= bb
__device__ __forceinline__ void overlap_pair(int p, int &ba, int &bb) {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= p) ++a;      // (at most DPMM_MAX_CLUSTERS_K / 64 trips)
    ba = a;
    bb = p - a * (a + 1) / 2;
}

// rows w, w + 4, .. of the block from row0, one batch: lane = point
__device__ __forceinline__ void overlap_stage(float *__restrict__ dst, const float *__restrict__ col, int64_t rs, int row0, int K, int w, int lane,
                                              float M, float S, bool on) {
    float a[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = row0 + w + 4 * j;
        a[j] = col[(int64_t)(k < K ? k : K - 1) * rs];      // unconditional, clamped: rows beyond K are zeroed below
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int k = row0 + w + 4 * j;
        const float p = score_p(score_e(a[j], M), S);
        dst[(w + 4 * j) * OV_PITCH + lane] = (on && k < K) ? p : 0.f;
    }
}

__global__ __launch_bounds__(OV_THREADS) void overlap_contract_kernel(OverlapArgs A) {
    __shared__ float la[64 * OV_PITCH];
    __shared__ float lb[64 * OV_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int K = A.K, pair = blockIdx.x, chunk = blockIdx.y;
    int ba, bb;
    overlap_pair(pair, ba, bb);
    const bool diag = ba == bb;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    const int64_t c0 = (int64_t)chunk * A.chunk;
    const int64_t c1 = c0 + A.chunk < A.n ? c0 + A.chunk : A.n;
    const bool wave_on = 64 * ba + 16 * w < K;               // a tile row beyond K holds zeros and is never read
    ov_f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (ov_f64x4){0., 0., 0., 0.};
    ov_f64x4 accm = (ov_f64x4){0., 0., 0., 0.};
    const float *const pb = diag ? la : lb;
    for (int64_t b0 = c0; b0 < c1; b0 += 64) {               // (uniform over the workgroup: the barriers below are met by all)
        const int64_t pt = b0 + lane;
        const bool in = pt < c1;
        const float2 ms = A.ms[in ? pt : c0];                 // (c0 < c1 <= n inside the loop)
        const bool on = in && ms.y > 0.f;
        const float *col = A.table + (in ? pt : c0);
        __syncthreads();                                      // the previous batch has been read
        overlap_stage(la, col, rs, 64 * ba, K, w, lane, ms.x, ms.y, on);
        if (!diag) overlap_stage(lb, col, rs, 64 * bb, K, w, lane, ms.x, ms.y, on);
        __syncthreads();
        if (!wave_on) continue;
        const float *ra = la + (16 * w + i) * OV_PITCH + g;
        const float *rb = pb + i * OV_PITCH + g;
        if (diag) {
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const double a = (double)ra[4 * s];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t <= w) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)rb[16 * t * OV_PITCH + 4 * s], acc[t], 0, 0, 0);
                accm = __builtin_amdgcn_mfma_f64_16x16x4f64(a, 1.0, accm, 0, 0, 0);
            }
        } else {
#pragma unroll 4
            for (int s = 0; s < 16; ++s) {
                const double a = (double)ra[4 * s];
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)rb[16 * t * OV_PITCH + 4 * s], acc[t], 0, 0, 0);
            }
        }
    }
    if (!wave_on) return;
    // block [chunk][pair][64][64]: element r of tile t is row 16 w + g + 4 r, column 16 t + i
    double *out = A.part + ((int64_t)chunk * gridDim.x + pair) * 4096;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(16 * w + g + 4 * r) * 64 + 16 * t + i] = acc[t][r];
    if (diag && i == 0) {
        double *mo = A.mpart + (int64_t)chunk * A.nb * 64 + 64 * ba + 16 * w + g;
#pragma unroll
        for (int r = 0; r < 4; ++r) mo[4 * r] = accm[r];
    }
}

__global__ __launch_bounds__(OV_THREADS) void overlap_reduce_kernel(OverlapArgs A) {
    const int K = A.K, npairs = A.nb * (A.nb + 1) / 2;
    const int64_t t = (int64_t)blockIdx.x * OV_THREADS + threadIdx.x;
    if (t < (int64_t)npairs * 4096) {
        const int pair = (int)(t >> 12), e = (int)(t & 4095), r = e >> 6, c = e & 63;
        int ba, bb;
        overlap_pair(pair, ba, bb);
        const int row = 64 * ba + r, col = 64 * bb + c;
        if (row >= K || col >= K || (ba == bb && r < c)) return;
        double v = 0.;
        for (int ch = 0; ch < A.nchunk; ++ch) v += A.part[((int64_t)ch * npairs + pair) * 4096 + e];
        const double x = A.acc[(int64_t)row * K + col] + v;
        A.acc[(int64_t)row * K + col] = x;
        if (row != col) A.acc[(int64_t)col * K + row] = x;
    } else {
        const int64_t k = t - (int64_t)npairs * 4096;
        if (k >= K) return;
        double v = 0.;
        for (int ch = 0; ch < A.nchunk; ++ch) v += A.mpart[(int64_t)ch * A.nb * 64 + k];
        A.acc[(int64_t)K * K + k] += v;
    }
}

// chunks of a range of n points: a function of n and K alone; nchunk * npairs <= OVERLAP_PARTIAL_BLOCKS, a chunk is whole 64-point batches
void overlap_chunks(int64_t n, int K, int *nchunk, int64_t *chunk) {
    const int nb = (K + 63) / 64, npairs = nb * (nb + 1) / 2;
    int64_t nc = (n + 255) / 256;
    const int64_t most = OVERLAP_PARTIAL_BLOCKS / npairs > 1 ? OVERLAP_PARTIAL_BLOCKS / npairs : 1;
    if (nc > most) nc = most;
    if (nc < 1) nc = 1;
    int64_t len = ((n + nc - 1) / nc + 63) / 64 * 64;
    if (len < 64) len = 64;
    *nchunk = (int)((n + len - 1) / len > 0 ? (n + len - 1) / len : 1);
    *chunk = len;
}

hipError_t launch_overlap_range(const OverlapArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.nb != (a.K + 63) / 64 || a.nchunk < 1 || a.chunk < 64 || (a.chunk & 63) || (int64_t)a.nchunk * a.chunk < a.n)
        return hipErrorInvalidValue;
    const int npairs = a.nb * (a.nb + 1) / 2;
    if ((int64_t)a.nchunk * npairs > (int64_t)OVERLAP_PARTIAL_BLOCKS && a.nchunk > 1) return hipErrorInvalidValue;
    int64_t g = (a.n + OV_THREADS - 1) / OV_THREADS;
    if (g > 2048) g = 2048;
    DPMM_LAUNCH(overlap_prep_kernel, dim3((int)g), dim3(OV_THREADS), 0, s, a);
    DPMM_LAUNCH(overlap_contract_kernel, dim3(npairs, a.nchunk), dim3(OV_THREADS), 0, s, a);
    const int64_t work = (int64_t)npairs * 4096 + a.K;
    DPMM_LAUNCH(overlap_reduce_kernel, dim3((int)((work + OV_THREADS - 1) / OV_THREADS)), dim3(OV_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace dpmm
