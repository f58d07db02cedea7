// batchstats.hip -- per-cluster sufficient statistics of a batch under the served model (include/dpmm_hip_batchstats.h):
// N[k] = sum_i w_ik, sums[k] = sum_i w_ik x_i, S[k] = sum_i w_ik x_i x_i' and the four counters, from a range of the table a_k(i) that the
// sweep kernels' table mode wrote (table[k * rstep * stride + i], as score.hip reads it) and the range's rows of the point-major Float32
// matrix X.  w_ik is 1 for the point's label or the Float32 probability score.hip writes, formed with the same functions
// (score_device.h) and widened to Float64; the sums are Float64 on the matrix pipe (v_mfma_f64_16x16x4_f64, operands as in overlap.hip).
//
// Launches per range, nothing in them waits for another workgroup:
//   prep      a workgroup per 256 points.  Lanes along i over the table: passes 1 and 2 of score_finish_kernel -- M, the label, NaN seen,
//             S, logdens.  The workgroup's 256 rows of X are one contiguous piece of memory: it is read flat, lanes along the words, and a
//             word that is not finite (features d < D only) marks its row in LDS.  With dpmm_batchstats_set_min_tail a complete point is
//             also held out when its tail -- one float per point of the range, written by typicality.hip in front of this kernel --
//             lies below the floor; without it that buffer does not exist and is not read.  The class of the point follows, and one float2 per
//             point: (M, S) in SOFT mode, (label, 1) in HARD mode, (0, 0) for a point that takes no part.  The counters are integer
//             adds in LDS, flushed to one of RANK_REPL replicas of the global counters: sums of integers, order-free.
//   contract  the range is cut into nchunk chunks, the features into blocks of 64; a workgroup of four waves owns (chunk, cluster k,
//             pair of feature blocks ba >= bb) and writes its 64 x 64 block of partial sums -- one writer, no atomics.  It walks its chunk
//             256 points at a time, thread = point, and appends the points with w_ik != 0 -- (index, w) -- to a ring in LDS in
//             increasing i (ballot, prefix inside the wave, the waves' counts through LDS).  HARD: those are the points labelled k, so the
//             matrix work is n D^2, not n K D^2; SOFT: p_ik > 0, and a far cluster's probability underflows to an exact 0.  Whenever
//             the ring holds 64 points (and once more for the rest of the chunk) they are staged: wave w loads slots 16 w .. 16 w + 15,
//             lane = feature, one coalesced 256-byte read per point and block, from clamped addresses (features beyond D and empty slots:
//             0, never an out-of-bounds read), to LDS point-major with 80 words per point; then wave w accumulates the four 16 x 16
//             tiles of tile row w over the batch's k-steps of 4 points.  Operands of k-step s: lane (i = lane & 15, g = lane >> 4)
//             supplies A[row i][k = g] = (double)w[4 s + g] * (double)x[4 s + g][16 w + i] -- exact -- and B[k = g][col i] =
//             x[4 s + g][16 t + i]; element r of the result is row g + 4 r, column i.  A lane reads word 80 (4 s + g) + 16 t + i: bank
//             16 g + i (mod 64), the 64 lanes in 64 banks; a wave writes 64 consecutive words.  On a diagonal pair the tiles above the
//             diagonal are left out and one more instruction per k-step, against a column of ones, gives the row sums: `sums`; pair 0,
//             wave 0 adds one with A = w: `N`.  Tile rows and tiles beyond D are neither computed nor read.
//   reduce    one thread per entry of the lower triangle of a cluster: the chunks' partials added in increasing chunk order, then added
//             to the accumulator and the sum written to [d][e] and [e][d] -- symmetric bit for bit.  sums and N likewise.
// contract and reduce run once per group of kgroup clusters, so that the partials stay inside BATCHSTATS_PARTIAL_BLOCKS blocks.  kgroup
// and nchunk depend on the range's length, K and D alone (batchstats_chunks), so the order of every addition is fixed by the call sequence.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"
#include "batchstats_device.h"

namespace dpmm {

typedef double bs_f64x4 __attribute__((ext_vector_type(4)));

constexpr int BS_THREADS = 256;
constexpr int BS_PITCH = 80;             // words per staged point: 64 features, = 16 (mod 64)
constexpr int BS_RING = 512;             // slots of the ring: at most 63 points left over + 256 new ones
constexpr int BS_CHUNK_MIN = 2048;       // points per chunk at least (unless the range is shorter)

__global__ __launch_bounds__(BS_THREADS) void batchstats_prep_kernel(BatchStatsArgs A) {
    __shared__ unsigned cnt[DPMM_MAX_CLUSTERS_K + BATCHSTATS_COUNTERS];
    __shared__ unsigned gap[BS_THREADS];
    const int K = A.K, D = A.D, tid = threadIdx.x, lane = tid & 63;
    const int ldx = (int)A.ldx;
    for (int k = tid; k < K + BATCHSTATS_COUNTERS; k += BS_THREADS) cnt[k] = 0;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    // (the trip count is the same for every thread of the workgroup: the barriers and ballots below see whole workgroups)
    for (int64_t base = (int64_t)blockIdx.x * BS_THREADS; base < A.n; base += (int64_t)gridDim.x * BS_THREADS) {
        __syncthreads();                                       // cnt is cleared / the previous trip's marks have been read
        gap[tid] = 0;
        __syncthreads();
        // ---- rows base .. base + 255 of X, flat: word f is feature f % ldx of row f / ldx
        const int rows = (int)(A.n - base < BS_THREADS ? A.n - base : BS_THREADS);
        const float *xr = A.X + base * A.ldx;
        bs_mark_gaps(gap, xr, rows, ldx, D, tid, BS_THREADS);
        // ---- the table: passes 1 and 2 of score_finish_kernel
        const int64_t i = base + tid;
        const bool valid = i < A.n;
        const float *col = A.table + (valid ? i : 0);      // (lanes past the end read point 0 and contribute nothing)
        float m, s;
        int best;
        bool nan_seen;
        bs_table_passes(col, rs, K, m, best, nan_seen, s);
        __syncthreads();
        // ---- the class: skipped, else held out, else incomplete, else it takes part (bs_class, batchstats_device.h)
        bool scored, held, incomplete, part;
        bs_class(valid, nan_seen, m, s, gap[tid], A.use_floor, A.min_logdens, A.use_tail, A.min_tail, A.tail, i, scored, held, incomplete, part);
        if (valid) A.ms[i] = !part ? make_float2(0.f, 0.f) : A.soft ? make_float2(m, s) : make_float2((float)best, 1.f);
        // ---- the counters (as overlap_prep_kernel)
        bs_count(cnt, K, lane, valid, scored, held, incomplete, part, best);
    }
    __syncthreads();
    bs_flush(cnt, A.count, K, tid, BS_THREADS);
}

// pair p of the lower block triangle, p = ba (ba + 1) / 2 + bb, ba >= bb
__device__ __forceinline__ void bs_pair(int p, int &ba, int &bb) {
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= p) ++a;      // (at most 4 trips: D <= 256)
    ba = a;
    bb = p - a * (a + 1) / 2;
}

// slots 16 w .. 16 w + 15 of a batch of nv points from ring slot h, features 64 blk + lane: lane = feature
__device__ __forceinline__ void bs_stage(float *__restrict__ dst, const float *__restrict__ X, int64_t ldx, const int *q_i, int h, int nv, int blk, int D,
                                         int w, int lane) {
    const int d = 64 * blk + lane;
    const bool din = d < D;
    const float *src = X + (din ? d : 0);
    float x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int slot = 16 * w + j;
        const int idx = slot < nv ? q_i[(h + slot) & (BS_RING - 1)] : 0;      // unconditional, clamped: empty slots are zeroed below
        x[j] = src[(int64_t)idx * ldx];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int slot = 16 * w + j;
        dst[slot * BS_PITCH + lane] = (din && slot < nv) ? x[j] : 0.f;
    }
}

template <bool SOFT>
__global__ __launch_bounds__(BS_THREADS) void batchstats_contract_kernel(BatchStatsArgs A) {
    __shared__ float xa[64 * BS_PITCH];
    __shared__ float xb[64 * BS_PITCH];
    __shared__ int q_i[BS_RING];
    __shared__ float q_w[BS_RING];
    __shared__ float wb[64];
    __shared__ int wcnt[BS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int D = A.D, pair = blockIdx.x, kk = blockIdx.y, chunk = blockIdx.z, k = A.k0 + kk;
    int ba, bb;
    bs_pair(pair, ba, bb);
    const bool diag = ba == bb, first = pair == 0 && w == 0;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    const int64_t c0 = (int64_t)chunk * A.chunk;
    const int64_t c1 = c0 + A.chunk < A.n ? c0 + A.chunk : A.n;
    const bool wave_on = 64 * ba + 16 * w < D;               // a tile row beyond D holds zeros and is never read
    const int nt = D - 64 * bb >= 64 ? 4 : (D - 64 * bb + 15) >> 4;      // tiles of block bb that hold features
    bs_f64x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = (bs_f64x4){0., 0., 0., 0.};
    bs_f64x4 accs = (bs_f64x4){0., 0., 0., 0.}, accn = (bs_f64x4){0., 0., 0., 0.};
    const float *const tcol = A.table + (int64_t)k * rs;
    const float *const pb = diag ? xa : xb;

    // one batch: nv <= 64 points from ring slot h (uniform over the workgroup: the barriers are met by all)
    auto batch = [&](int h, int nv) {
        __syncthreads();                                      // the previous batch has been read; the ring's new entries are written
        bs_stage(xa, A.X, A.ldx, q_i, h, nv, ba, D, w, lane);
        if (!diag) bs_stage(xb, A.X, A.ldx, q_i, h, nv, bb, D, w, lane);
        if (tid < 64) wb[tid] = tid < nv ? q_w[(h + tid) & (BS_RING - 1)] : 0.f;
        __syncthreads();
        if (!wave_on) return;
        const float *ra = xa + g * BS_PITCH + 16 * w + i;
        const float *rb = pb + g * BS_PITCH + i;
        const int ns = (nv + 3) >> 2;
        for (int s = 0; s < ns; ++s) {
            const double wv = (double)wb[4 * s + g];
            const double a = wv * (double)ra[4 * s * BS_PITCH];      // Float32 x Float32 in Float64: exact
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (t < nt && (!diag || t <= w)) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)rb[4 * s * BS_PITCH + 16 * t], acc[t], 0, 0, 0);
            if (diag) accs = __builtin_amdgcn_mfma_f64_16x16x4f64(a, 1.0, accs, 0, 0, 0);
            if (first) accn = __builtin_amdgcn_mfma_f64_16x16x4f64(wv, 1.0, accn, 0, 0, 0);
        }
    };

    int head = 0, qn = 0;                                     // the ring: qn points from slot head, the same in every thread
    for (int64_t b0 = c0; b0 < c1; b0 += BS_THREADS) {
        const int64_t pt = b0 + tid;
        float wt = 0.f;
        if (pt < c1) {
            const float2 ms = A.ms[pt];
            if (ms.y > 0.f) wt = SOFT ? score_p(score_e(tcol[pt], ms.x), ms.y) : ((int)ms.x == k ? 1.f : 0.f);
        }
        const bool take = wt > 0.f;
        const unsigned long long bm = __ballot(take);
        if (lane == 0) wcnt[w] = __popcll(bm);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int v = 0; v < BS_THREADS / 64; ++v) {
            const int c = wcnt[v];
            off += v < w ? c : 0;
            tot += c;
        }
        if (take) {
            const int slot = (head + qn + off + __popcll(bm & ((1ull << lane) - 1ull))) & (BS_RING - 1);
            q_i[slot] = (int)pt;
            q_w[slot] = wt;
        }
        qn += tot;
        __syncthreads();                                      // wcnt has been read
        while (qn >= 64) {
            batch(head, 64);
            head = (head + 64) & (BS_RING - 1);
            qn -= 64;
        }
    }
    if (qn > 0) batch(head, qn);
    if (!wave_on) return;
    // block [chunk][kk][pair][64][64]: element r of tile t is row 16 w + g + 4 r, column 16 t + i
    const int64_t ck = (int64_t)chunk * gridDim.y + kk;
    double *out = A.part + (ck * gridDim.x + pair) * 4096;
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (t < nt && (!diag || t <= w)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(16 * w + g + 4 * r) * 64 + 16 * t + i] = acc[t][r];
        }
    if (diag && i == 0) {
        double *so = A.spart + ck * A.nb * 64 + 64 * ba + 16 * w + g;
#pragma unroll
        for (int r = 0; r < 4; ++r) so[4 * r] = accs[r];
    }
    if (first && lane == 0) A.npart[ck] = accn[0];
}

__global__ __launch_bounds__(BS_THREADS) void batchstats_reduce_kernel(BatchStatsArgs A) {
    const int K = A.K, D = A.D, nb = A.nb, npairs = nb * (nb + 1) / 2, kc = A.kcount;
    const int64_t t = (int64_t)blockIdx.x * BS_THREADS + threadIdx.x;
    const int64_t nS = (int64_t)kc * npairs * 4096, ns = (int64_t)kc * nb * 64;
    double *const N = A.acc, *const sums = A.acc + K, *const S = A.acc + K + (int64_t)K * D;
    if (t < nS) {
        const int kk = (int)(t / ((int64_t)npairs * 4096));
        const int rem = (int)(t - (int64_t)kk * npairs * 4096);
        const int pair = rem >> 12, e = rem & 4095, r = e >> 6, c = e & 63;
        int ba, bb;
        bs_pair(pair, ba, bb);
        const int row = 64 * ba + r, col = 64 * bb + c;
        if (row >= D || col >= D || (ba == bb && r < c)) return;
        double v = 0.;
        for (int ch = 0; ch < A.nchunk; ++ch) v += A.part[(((int64_t)ch * kc + kk) * npairs + pair) * 4096 + e];
        double *Sk = S + (int64_t)(A.k0 + kk) * D * D;
        const double x = Sk[(int64_t)row * D + col] + v;
        Sk[(int64_t)row * D + col] = x;
        if (row != col) Sk[(int64_t)col * D + row] = x;
    } else if (t < nS + ns) {
        const int kk = (int)((t - nS) / (nb * 64)), d = (int)((t - nS) - (int64_t)kk * nb * 64);
        if (d >= D) return;
        double v = 0.;
        for (int ch = 0; ch < A.nchunk; ++ch) v += A.spart[((int64_t)ch * kc + kk) * nb * 64 + d];
        sums[(int64_t)(A.k0 + kk) * D + d] += v;
    } else if (t < nS + ns + kc) {
        const int kk = (int)(t - nS - ns);
        double v = 0.;
        for (int ch = 0; ch < A.nchunk; ++ch) v += A.npart[(int64_t)ch * kc + kk];
        N[A.k0 + kk] += v;
    }
}

// clusters per launch and chunks of a range of n points: functions of n, K and D alone; nchunk * kgroup * npairs <= BATCHSTATS_PARTIAL_BLOCKS,
// a chunk is whole 64-point batches and at least BS_CHUNK_MIN points unless the range is shorter
void batchstats_chunks(int64_t n, int K, int D, int *kgroup, int *nchunk, int64_t *chunk) {
    const int nb = (D + 63) / 64, npairs = nb * (nb + 1) / 2;
    const int kg = K < BATCHSTATS_PARTIAL_BLOCKS / npairs ? K : BATCHSTATS_PARTIAL_BLOCKS / npairs;
    const int64_t most = BATCHSTATS_PARTIAL_BLOCKS / (kg * npairs) > 1 ? BATCHSTATS_PARTIAL_BLOCKS / (kg * npairs) : 1;
    int64_t nc = (n + BS_CHUNK_MIN - 1) / BS_CHUNK_MIN;
    if (nc > most) nc = most;
    if (nc < 1) nc = 1;
    int64_t len = ((n + nc - 1) / nc + 63) / 64 * 64;
    if (len < 64) len = 64;
    *kgroup = kg;
    *nchunk = (int)((n + len - 1) / len > 0 ? (n + len - 1) / len : 1);
    *chunk = len;
}

hipError_t launch_batchstats_range(const BatchStatsArgs &a0, hipStream_t s) {
    BatchStatsArgs a = a0;
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.D < 1 || a.D > 256 || a.ldx < a.D || a.ldx > 1024 || a.nb != (a.D + 63) / 64 || a.n >> 31 || a.kgroup < 1 ||
        a.nchunk < 1 || a.chunk < 64 || (a.chunk & 63) || (int64_t)a.nchunk * a.chunk < a.n || a.nchunk > 65535)
        return hipErrorInvalidValue;
    const int npairs = a.nb * (a.nb + 1) / 2;
    if ((int64_t)a.nchunk * std::min(a.kgroup, a.K) * npairs > (int64_t)BATCHSTATS_PARTIAL_BLOCKS) return hipErrorInvalidValue;
    int64_t g = (a.n + BS_THREADS - 1) / BS_THREADS;
    if (g > 8192) g = 8192;
    DPMM_LAUNCH(batchstats_prep_kernel, dim3((int)g), dim3(BS_THREADS), 0, s, a);
    for (int k0 = 0; k0 < a.K; k0 += a.kgroup) {
        a.k0 = k0;
        a.kcount = std::min(a.kgroup, a.K - k0);
        const dim3 grid(npairs, a.kcount, a.nchunk);
        if (a.soft) DPMM_LAUNCH(batchstats_contract_kernel<true>, grid, dim3(BS_THREADS), 0, s, a);
        else DPMM_LAUNCH(batchstats_contract_kernel<false>, grid, dim3(BS_THREADS), 0, s, a);
        const int64_t work = (int64_t)a.kcount * ((int64_t)npairs * 4096 + a.nb * 64 + 1);
        DPMM_LAUNCH(batchstats_reduce_kernel, dim3((int)((work + BS_THREADS - 1) / BS_THREADS)), dim3(BS_THREADS), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace dpmm
