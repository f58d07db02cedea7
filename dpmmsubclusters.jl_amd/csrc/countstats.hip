// countstats.hip -- per-cluster count statistics of a batch under the served Multinomial model (include/dpmm_hip_countstats.h):
// N[k] = sum_i w_ik, sums[k][d] = sum_i w_ik x_id and the four counters, from a range of the table a_k(i) that the Multinomial kernels' table
// mode wrote (table[k * rstep * stride + i], rstep = 3, as score.hip reads it) and the range's points in whichever store is live: the
// point-major Float32 matrix, its lossless byte copy, or compressed sparse columns.  w_ik is 1 for the point's label or the Float32
// probability score.hip writes, formed with the same functions (score_device.h) and widened to Float64; w x is formed in Float64.
//
// Launches per range, nothing in them waits for another workgroup:
//   totals    only with the floor per count (dpmm_countstats_set_per_count), in front of prep by the caller: t_i, the Float64 total of every
//             point's values, one wave per point, lanes strided over the entries and a fixed butterfly -- a function of the point alone.
//   prep      the classification of countstats_device.h (cs_mark_gaps, cs_class -- shared with holdout.hip), a workgroup per 256 points,
//             one float2 per point: (M, S) in SOFT mode, (label, 1) in HARD mode, (0, 0) for a point that takes no part.  The scan for a
//             value that is not finite goes over the live store: the workgroup's rows of X read flat; nothing for bytes; for sparse points
//             the workgroup's entries cp[base] .. cp[base + rows] read flat, and the (rare) offender's column found by bisection in cp.
//   contract, dense and byte stores: W' X on the Float64 matrix pipe (v_mfma_f64_16x16x4_f64, operands as in overlap.hip / batchstats.hip).
//             The range is cut into nchunk chunks, the clusters into groups of 16, the features into blocks of 256; a workgroup of four
//             waves owns (chunk, group, block) and writes its 16 x 256 partial sums -- one writer, no atomics.  It walks its chunk 256
//             points at a time, thread = point, and appends the points with a non-zero weight in the group -- index and the 16 weights
//             (HARD: the index of the one cluster) -- to a ring in LDS in increasing i (ballot, prefix inside the wave, the waves' counts
//             through LDS).  HARD: every point is staged by one group, the matrix work is n 16 D; SOFT: a far cluster's probability is an
//             exact 0.  Whenever the ring holds 64 points (and once more for the rest) they are staged one 64-feature block after the
//             other: wave w loads slots 16 w .. 16 w + 15, lane = feature, coalesced along the row (Float32, or bytes widened on the way),
//             from clamped addresses (features beyond D and empty slots: 0, never an out-of-bounds read), to LDS point-major with 80
//             words per point; then wave w accumulates the 16 x 16 tile (clusters x features 16 w ..) over the k-steps of 4 points:
//             lane (i = lane & 15, g = lane >> 4) supplies A[cluster i][k = g] = (double)w and B[k = g][feature i] = (double)x; element r
//             of the result is cluster g + 4 r, feature i.  Block 0, wave 0 adds one instruction against a column of ones: `N`.
//   contract, sparse store: work proportional to the stored entries of the points with weight.  A workgroup owns (chunk, cluster k, range of
//             7168 features), wave w the 1792 features from 1792 w of it and as many doubles of LDS.  The chunk is walked 256 points at a
//             time; the points with w_ik != 0 are listed in LDS (offset, length, w) in increasing i, and every wave takes the list point
//             by point: the lanes spread over the point's entries -- from the start of the column when it has at most 128 entries,
//             else from the first entry of the wave's range, found by bisection in ri (rows are strictly increasing) -- and add
//             (double)w * (double)val to acc[ri - r0]: a column holds a row once, so no two lanes meet, and the wave's LDS operations are
//             in order from one point to the next.  No atomics; an empty column adds to N alone.  N is summed per thread, then over the
//             256 threads in index order, by the workgroups of range 0.
//   reduce    one thread per (cluster, feature): the chunks' partials added in increasing chunk order, then added to the accumulator.
// contract and reduce run once per group of kgroup clusters, so that the partials stay inside COUNTSTATS_PARTIAL_BYTES.  kgroup and nchunk
// depend on the range's length, K, D and the kind of store alone (countstats_chunks): the order of every addition is fixed by the call sequence.
#include <algorithm>
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"
#include "batchstats_device.h"
#include "countstats_device.h"

namespace dpmm {

typedef double cs_f64x4 __attribute__((ext_vector_type(4)));

constexpr int CS_THREADS = 256;
constexpr int CS_PITCH = 80;             // words per staged point: 64 features, = 16 (mod 64)
constexpr int CS_RING = 512;             // slots of the ring: at most 63 points left over + 256 new ones
constexpr int CS_CHUNK_MIN = 2048;       // points per chunk at least (unless the range is shorter)
constexpr int CS_G = 16;                 // clusters of a group: the rows of the matrix instruction
constexpr int CS_XB = 4;                 // 64-feature blocks of a dense workgroup
constexpr int CS_SP_WAVE = 1792;         // features (doubles of LDS) of a wave of the sparse kernel
constexpr int CS_SP_WG = 4 * CS_SP_WAVE; // ... of its workgroup: 56 KB
constexpr int CS_SP_SCAN = 128;          // columns up to this length are scanned from their start, longer ones bisected

// (t_i, the Float64 total of a point's values: cs_wave_total of countstats_device.h)
__global__ __launch_bounds__(CS_THREADS) void countstats_totals_kernel(CountTotalsArgs A) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    constexpr int WAVES = CS_THREADS / 64;
    // (the trip count is the same for every lane of a wave: the shuffles see whole waves)
    for (int64_t i = (int64_t)blockIdx.x * WAVES + w; i < A.n; i += (int64_t)gridDim.x * WAVES) {
        double t;
        if (A.store == COUNTSTATS_F32) t = cs_wave_total(A.X + i * A.ldx, A.D, lane);
        else if (A.store == COUNTSTATS_U8) t = cs_wave_total(A.X8 + i * A.ld8, A.D, lane);
        else { const int64_t lo = A.cp[i]; t = cs_wave_total(A.val + lo, A.cp[i + 1] - lo, lane); }
        if (lane == 0) A.tot[i] = t;
    }
}

hipError_t launch_countstats_totals(const CountTotalsArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.n >> 31 || a.D < 1 || !a.tot) return hipErrorInvalidValue;
    if (a.store == COUNTSTATS_F32) { if (!a.X || a.ldx < a.D) return hipErrorInvalidValue; }
    else if (a.store == COUNTSTATS_U8) { if (!a.X8 || a.ld8 < a.D) return hipErrorInvalidValue; }
    else if (a.store == COUNTSTATS_SPARSE) { if (!a.cp) return hipErrorInvalidValue; }      // (val is read only where a column has entries)
    else return hipErrorInvalidValue;
    const int64_t g = std::min<int64_t>((a.n + CS_THREADS / 64 - 1) / (CS_THREADS / 64), (int64_t)1 << 20);
    DPMM_LAUNCH(countstats_totals_kernel, dim3((unsigned)g), dim3(CS_THREADS), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(CS_THREADS) void countstats_prep_kernel(CountStatsArgs A) {
    __shared__ unsigned cnt[DPMM_MAX_CLUSTERS_K + BATCHSTATS_COUNTERS];
    __shared__ unsigned gap[CS_THREADS];
    const int K = A.K, D = A.D, tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < K + BATCHSTATS_COUNTERS; k += CS_THREADS) cnt[k] = 0;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    // (the trip count is the same for every thread of the workgroup: the barriers and ballots below see whole workgroups)
    for (int64_t base = (int64_t)blockIdx.x * CS_THREADS; base < A.n; base += (int64_t)gridDim.x * CS_THREADS) {
        __syncthreads();                                       // cnt is cleared / the previous trip's marks have been read
        gap[tid] = 0;
        __syncthreads();
        const int rows = (int)(A.n - base < CS_THREADS ? A.n - base : CS_THREADS);
        // a value that is not finite, over the live store (countstats_device.h): the rows of X flat; the entries of the columns flat; a byte is finite
        cs_mark_gaps(gap, A.store, A.store == COUNTSTATS_F32 ? A.X + base * A.ldx : nullptr, (int)A.ldx, A.store == COUNTSTATS_SPARSE ? A.cp + base : nullptr, A.val, rows, D,
                     tid, CS_THREADS);
        const int64_t i = base + tid;
        const bool valid = i < A.n;
        const float *col = A.table + (valid ? i : 0);      // (lanes past the end read point 0 and contribute nothing)
        float m, s;
        int best;
        bool nan_seen;
        bs_table_passes(col, rs, K, m, best, nan_seen, s);
        __syncthreads();
        // ---- the class: skipped, else held out, else incomplete, else it takes part
        bool scored, held, incomplete, part;
        cs_class(valid, nan_seen, m, s, gap[tid], A.use_floor, A.min_logdens, A.use_pc, A.min_pc, A.tot, i, scored, held, incomplete, part);
        if (valid) A.ms[i] = !part ? make_float2(0.f, 0.f) : A.soft ? make_float2(m, s) : make_float2((float)best, 1.f);
        bs_count(cnt, K, lane, valid, scored, held, incomplete, part, best);
    }
    __syncthreads();
    bs_flush(cnt, A.count, K, tid, CS_THREADS);
}

// slots 16 w .. 16 w + 15 of a batch of nv points from ring slot h, features fb + lane: lane = feature
template <typename T>
__device__ __forceinline__ void cs_stage(float *__restrict__ dst, const T *__restrict__ X, int64_t ld, const int *q_i, int h, int nv, int fb, int D, int w, int lane) {
    const int d = fb + lane;
    const bool din = d < D;
    const T *src = X + (din ? d : 0);
    float x[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int slot = 16 * w + j;
        const int idx = slot < nv ? q_i[(h + slot) & (CS_RING - 1)] : 0;      // unconditional, clamped: empty slots are zeroed below
        x[j] = (float)src[(int64_t)idx * ld];
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int slot = 16 * w + j;
        dst[slot * CS_PITCH + lane] = (din && slot < nv) ? x[j] : 0.f;
    }
}

template <bool SOFT, typename T>
__global__ __launch_bounds__(CS_THREADS) void countstats_dense_kernel(CountStatsArgs A, const T *__restrict__ X, int64_t ld) {
    __shared__ float xa[64 * CS_PITCH];
    __shared__ int q_i[CS_RING];
    __shared__ float q_w[SOFT ? CS_RING * CS_G : CS_RING];      // SOFT: the group's 16 weights of the point; HARD: its cluster inside the group
    __shared__ int wcnt[CS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int i = lane & 15, g = lane >> 4;
    const int D = A.D, bx = blockIdx.x, cg = blockIdx.y, chunk = blockIdx.z;
    const int kg0 = A.k0 + CS_G * cg;                            // the group's first cluster
    const int kin = A.K - kg0 < CS_G ? A.K - kg0 : CS_G;         // its clusters that exist (>= 1)
    const int f0 = 64 * CS_XB * bx;
    const int nfb = D - f0 >= 64 * CS_XB ? CS_XB : (D - f0 + 63) >> 6;      // 64-feature blocks that hold features (>= 1)
    const bool first = bx == 0 && w == 0;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    const int64_t c0 = (int64_t)chunk * A.chunk;
    const int64_t c1 = c0 + A.chunk < A.n ? c0 + A.chunk : A.n;
    cs_f64x4 acc[CS_XB];
#pragma unroll
    for (int t = 0; t < CS_XB; ++t) acc[t] = (cs_f64x4){0., 0., 0., 0.};
    cs_f64x4 accn = (cs_f64x4){0., 0., 0., 0.};
    const float *const tcol = A.table + (int64_t)kg0 * rs;

    // one batch: nv <= 64 points from ring slot h (uniform over the workgroup: the barriers are met by all)
    auto batch = [&](int h, int nv) {
        const int ns = (nv + 3) >> 2;
#pragma unroll
        for (int t = 0; t < CS_XB; ++t) {
            if (t >= nfb) break;
            __syncthreads();                                  // the previous block has been read; the ring's new entries are written
            cs_stage<T>(xa, X, ld, q_i, h, nv, f0 + 64 * t, D, w, lane);
            __syncthreads();
            if (f0 + 64 * t + 16 * w >= D) continue;          // a tile beyond D holds zeros and is never read
            const float *rb = xa + g * CS_PITCH + 16 * w + i;
            for (int s = 0; s < ns; ++s) {
                const int slot = 4 * s + g;
                double wv = 0.;
                if (slot < nv) {
                    const int q = (h + slot) & (CS_RING - 1);
                    if constexpr (SOFT) wv = (double)q_w[q * CS_G + i];
                    else wv = q_w[q] == (float)i ? 1. : 0.;
                }
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv, (double)rb[4 * s * CS_PITCH], acc[t], 0, 0, 0);      // Float32 x Float32 in Float64: exact
                if (first && t == 0) accn = __builtin_amdgcn_mfma_f64_16x16x4f64(wv, 1.0, accn, 0, 0, 0);
            }
        }
    };

    int head = 0, qn = 0;                                     // the ring: qn points from slot head, the same in every thread
    for (int64_t b0 = c0; b0 < c1; b0 += CS_THREADS) {
        const int64_t pt = b0 + tid;
        float wl[SOFT ? CS_G : 1];
        int lab = -1;
        bool take = false;
        if (pt < c1) {
            const float2 ms = A.ms[pt];
            if (ms.y > 0.f) {
                if constexpr (SOFT) {
#pragma unroll
                    for (int j = 0; j < CS_G; ++j) {
                        const float p = score_p(score_e(tcol[(int64_t)(j < kin ? j : kin - 1) * rs + pt], ms.x), ms.y);
                        wl[j] = j < kin ? p : 0.f;
                        take = take || wl[j] > 0.f;
                    }
                } else {
                    lab = (int)ms.x - kg0;
                    take = lab >= 0 && lab < CS_G;
                }
            }
        }
        const unsigned long long bm = __ballot(take);
        if (lane == 0) wcnt[w] = __popcll(bm);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int v = 0; v < CS_THREADS / 64; ++v) {
            const int c = wcnt[v];
            off += v < w ? c : 0;
            tot += c;
        }
        if (take) {
            const int slot = (head + qn + off + __popcll(bm & ((1ull << lane) - 1ull))) & (CS_RING - 1);
            q_i[slot] = (int)pt;
            if constexpr (SOFT) {
#pragma unroll
                for (int j = 0; j < CS_G; ++j) q_w[slot * CS_G + j] = wl[j];
            } else {
                q_w[slot] = (float)lab;
            }
        }
        qn += tot;
        __syncthreads();                                      // wcnt has been read
        while (qn >= 64) {
            batch(head, 64);
            head = (head + 64) & (CS_RING - 1);
            qn -= 64;
        }
    }
    if (qn > 0) batch(head, qn);
    // rows [chunk][16 cg + cluster][dp]: element r of tile t is cluster g + 4 r, feature f0 + 64 t + 16 w + i
    const int64_t row0 = (int64_t)chunk * A.krows + CS_G * cg;
#pragma unroll
    for (int t = 0; t < CS_XB; ++t)
        if (t < nfb && f0 + 64 * t + 16 * w < D) {
#pragma unroll
            for (int r = 0; r < 4; ++r) A.part[(row0 + g + 4 * r) * A.dp + f0 + 64 * t + 16 * w + i] = acc[t][r];
        }
    if (first && i == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) A.npart[row0 + g + 4 * r] = accn[r];
    }
}

template <bool SOFT>
__global__ __launch_bounds__(CS_THREADS) void countstats_sparse_kernel(CountStatsArgs A) {
    __shared__ double acc[CS_SP_WG];
    __shared__ double nred[CS_THREADS];
    __shared__ int64_t q_lo[CS_THREADS];
    __shared__ int q_len[CS_THREADS];
    __shared__ float q_w[CS_THREADS];
    __shared__ int wcnt[CS_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int D = A.D, bx = blockIdx.x, kk = blockIdx.y, chunk = blockIdx.z, k = A.k0 + kk;
    const int r0 = CS_SP_WG * bx + CS_SP_WAVE * w;             // the wave's features r0 .. r1 - 1 (none when r0 >= D)
    const int r1 = r0 + CS_SP_WAVE < D ? r0 + CS_SP_WAVE : D;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    const int64_t c0 = (int64_t)chunk * A.chunk;
    const int64_t c1 = c0 + A.chunk < A.n ? c0 + A.chunk : A.n;
    const float *const tcol = A.table + (int64_t)k * rs;
    double *const my = acc + CS_SP_WAVE * w;
    for (int j = tid; j < CS_SP_WG; j += CS_THREADS) acc[j] = 0.;
    double nsum = 0.;
    for (int64_t b0 = c0; b0 < c1; b0 += CS_THREADS) {
        const int64_t pt = b0 + tid;
        float wt = 0.f;
        if (pt < c1) {
            const float2 ms = A.ms[pt];
            if (ms.y > 0.f) wt = SOFT ? score_p(score_e(tcol[pt], ms.x), ms.y) : ((int)ms.x == k ? 1.f : 0.f);
        }
        const bool take = wt > 0.f;
        nsum += (double)wt;
        const unsigned long long bm = __ballot(take);
        if (lane == 0) wcnt[w] = __popcll(bm);
        __syncthreads();                                      // acc is cleared; the previous list has been walked by every wave
        int off = 0, tot = 0;
#pragma unroll
        for (int v = 0; v < CS_THREADS / 64; ++v) {
            const int c = wcnt[v];
            off += v < w ? c : 0;
            tot += c;
        }
        if (take) {
            const int slot = off + __popcll(bm & ((1ull << lane) - 1ull));
            const int64_t lo = A.cp[pt];
            q_lo[slot] = lo;
            q_len[slot] = (int)(A.cp[pt + 1] - lo);
            q_w[slot] = wt;
        }
        __syncthreads();
        if (r0 >= D) continue;                                // (the wave still meets the barriers)
        for (int q = 0; q < tot; ++q) {
            const int len = q_len[q];
            if (len == 0) continue;
            const int64_t lo = q_lo[q], e1 = lo + len;
            const double wv = (double)q_w[q];
            int64_t e0 = lo;
            if (len > CS_SP_SCAN) {                           // the first entry with ri >= r0 (the same in every lane)
                int a = 0, b = len;
                while (a < b) {
                    const int mid = (a + b) >> 1;
                    if ((int)A.ri[lo + mid] < r0) a = mid + 1; else b = mid;
                }
                e0 = lo + a;
            }
            for (int64_t eb = e0; eb < e1; eb += 64) {
                const int64_t e = eb + lane;
                const int d = e < e1 ? (int)A.ri[e] : 0x7fffffff;
                if (d >= r0 && d < r1) my[d - r0] = my[d - r0] + wv * (double)A.val[e];      // Float32 x Float32 in Float64: exact
                if (__ballot(d >= r1) != 0) break;            // rows increase: nothing of the range lies further on
            }
            __threadfence_block();                            // the next point may hold the same features on other lanes
        }
    }
    __syncthreads();
    const int64_t row = (int64_t)chunk * A.krows + kk;
    for (int j = lane; j < r1 - r0; j += 64) A.part[row * A.dp + r0 + j] = my[j];
    if (bx == 0) {                                            // N: per thread in increasing i, then the threads in index order
        nred[tid] = nsum;
        __syncthreads();
        if (tid == 0) {
            double v = 0.;
            for (int j = 0; j < CS_THREADS; ++j) v += nred[j];
            A.npart[row] = v;
        }
    }
}

__global__ __launch_bounds__(CS_THREADS) void countstats_reduce_kernel(CountStatsArgs A) {
    const int K = A.K, D = A.D, kc = A.kcount;
    const int64_t t = (int64_t)blockIdx.x * CS_THREADS + threadIdx.x;
    const int64_t ns = (int64_t)kc * D;
    double *const N = A.acc, *const sums = A.acc + K;
    if (t < ns) {
        const int kk = (int)(t / D), d = (int)(t - (int64_t)kk * D);
        double v = 0.;
        for (int ch = 0; ch < A.nchunk; ++ch) v += A.part[((int64_t)ch * A.krows + kk) * A.dp + d];
        sums[(int64_t)(A.k0 + kk) * D + d] += v;
    } else if (t < ns + kc) {
        const int kk = (int)(t - ns);
        double v = 0.;
        for (int ch = 0; ch < A.nchunk; ++ch) v += A.npart[(int64_t)ch * A.krows + kk];
        N[A.k0 + kk] += v;
    }
}

// clusters per launch, chunks of a range of n points and the pitch of a partial row: functions of n, K, D and the kind of store alone;
// nchunk * kgroup * dp doubles stay inside COUNTSTATS_PARTIAL_BYTES (dp <= 65536 doubles: at least 128 rows fit), a chunk is whole 64-point
// batches and at least CS_CHUNK_MIN points unless the range is shorter
void countstats_chunks(int64_t n, int K, int D, int sparse, int *kgroup, int *nchunk, int64_t *chunk, int64_t *dp) {
    const int64_t pitch = sparse ? D : (int64_t)(D + 64 * CS_XB - 1) / (64 * CS_XB) * (64 * CS_XB);
    const int64_t rows = std::max<int64_t>(CS_G, COUNTSTATS_PARTIAL_BYTES / 8 / pitch);
    const int64_t kp = sparse ? K : (int64_t)(K + CS_G - 1) / CS_G * CS_G;
    const int64_t kg = std::min<int64_t>(kp, sparse ? rows : rows / CS_G * CS_G);
    const int64_t most = std::min<int64_t>(65535, std::max<int64_t>(1, rows / kg));
    int64_t nc = (n + CS_CHUNK_MIN - 1) / CS_CHUNK_MIN;
    if (nc > most) nc = most;
    if (nc < 1) nc = 1;
    int64_t len = ((n + nc - 1) / nc + 63) / 64 * 64;
    if (len < 64) len = 64;
    *kgroup = (int)kg;
    *nchunk = (int)((n + len - 1) / len > 0 ? (n + len - 1) / len : 1);
    *chunk = len;
    *dp = pitch;
}

hipError_t launch_countstats_range(const CountStatsArgs &a0, hipStream_t s) {
    CountStatsArgs a = a0;
    if (a.n <= 0) return hipSuccess;
    const bool sparse = a.store == COUNTSTATS_SPARSE;
    if (a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.D < 1 || a.D > (1 << 20) || a.n >> 31 || a.kgroup < 1 || a.nchunk < 1 || a.chunk < 64 || (a.chunk & 63) ||
        (int64_t)a.nchunk * a.chunk < a.n || a.nchunk > 65535 || a.dp < a.D || !a.table || !a.ms || !a.count || !a.part || !a.npart || !a.acc ||
        (a.use_pc && !a.tot))
        return hipErrorInvalidValue;
    if (a.store == COUNTSTATS_F32) { if (!a.X || a.ldx < a.D || a.ldx > (1 << 22)) return hipErrorInvalidValue; }
    else if (a.store == COUNTSTATS_U8) { if (!a.X8 || a.ld8 < a.D) return hipErrorInvalidValue; }
    else if (sparse) { if (!a.cp || !a.ri || !a.val || a.D > 65536) return hipErrorInvalidValue; }
    else return hipErrorInvalidValue;
    if (!sparse && ((a.kgroup % CS_G) || (a.dp % (64 * CS_XB)))) return hipErrorInvalidValue;
    if ((int64_t)a.nchunk * a.kgroup * a.dp * 8 > std::max<int64_t>(COUNTSTATS_PARTIAL_BYTES, (int64_t)CS_G * a.dp * 8)) return hipErrorInvalidValue;
    int64_t g = (a.n + CS_THREADS - 1) / CS_THREADS;
    if (g > 8192) g = 8192;
    DPMM_LAUNCH(countstats_prep_kernel, dim3((int)g), dim3(CS_THREADS), 0, s, a);
    double *const part0 = a.part;
    for (int k0 = 0; k0 < a.K; k0 += a.kgroup) {
        a.k0 = k0;
        a.kcount = std::min(a.kgroup, a.K - k0);
        a.krows = sparse ? a.kcount : (a.kcount + CS_G - 1) / CS_G * CS_G;
        a.part = part0;
        if (sparse) {
            const dim3 grid((a.D + CS_SP_WG - 1) / CS_SP_WG, a.kcount, a.nchunk);
            if (a.soft) DPMM_LAUNCH(countstats_sparse_kernel<true>, grid, dim3(CS_THREADS), 0, s, a);
            else DPMM_LAUNCH(countstats_sparse_kernel<false>, grid, dim3(CS_THREADS), 0, s, a);
        } else {
            const dim3 grid((a.D + 64 * CS_XB - 1) / (64 * CS_XB), a.krows / CS_G, a.nchunk);
            if (a.store == COUNTSTATS_U8) {
                if (a.soft) DPMM_LAUNCH((countstats_dense_kernel<true, uint8_t>), grid, dim3(CS_THREADS), 0, s, a, a.X8, a.ld8);
                else DPMM_LAUNCH((countstats_dense_kernel<false, uint8_t>), grid, dim3(CS_THREADS), 0, s, a, a.X8, a.ld8);
            } else {
                if (a.soft) DPMM_LAUNCH((countstats_dense_kernel<true, float>), grid, dim3(CS_THREADS), 0, s, a, a.X, a.ldx);
                else DPMM_LAUNCH((countstats_dense_kernel<false, float>), grid, dim3(CS_THREADS), 0, s, a, a.X, a.ldx);
            }
        }
        const int64_t work = (int64_t)a.kcount * ((int64_t)a.D + 1);
        DPMM_LAUNCH(countstats_reduce_kernel, dim3((unsigned)((work + CS_THREADS - 1) / CS_THREADS)), dim3(CS_THREADS), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace dpmm
