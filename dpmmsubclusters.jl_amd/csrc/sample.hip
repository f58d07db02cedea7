// sample.hip -- drawing new points from a fitted model (include/dpmm_hip_sample.h, which states the laws and the keying of every random
// word: Philox4x32-10, key = seed, counter = (global sample index, block number, stream)).  The value of a sample depends on
// (seed, its global index, its cluster, the model) alone; how a draw is cut into calls, tiles and workgroups decides nothing.
//
//   sample_niw_kernel          x = m_k + sqrt(df_k / g) A_k z.  A workgroup (4 waves) walks a contiguous range of 64-point tiles; a tile lies
//       inside one cluster (tstart [K + 1]: first tile of every cluster, cstart [K + 1]: first point, both relative to the call).  Per tile:
//       wave 0 draws the 64 chi^2 values (Float64 Marsaglia-Tsang, at most 8 rounds), all waves the D x 64 normals into the LDS tile
//       zs[b][i] (feature major: lanes along i write 64 banks); then thread (feature a, 16 points) accumulates sum_{b >= a0} A[a][b] z[b][i]
//       with plain fmaf: A is read TRANSPOSED (At[b][a]: lanes along a read one line, every cluster's matrix stays in L2), z as broadcast
//       ds_read_b128 (the 64 lanes of a wave share the 16 points when D > 32).  b starts at the wave's first feature a0: the 64 x 64
//       blocks below the diagonal are skipped, the zeros below it inside a diagonal block are multiplied.  Rows leave coalesced: lanes
//       along a, 256 bytes per point and wave.  Lanes of points past a short tile's end compute on whatever the tile holds and store nothing.
//   sample_mult_dense_kernel   one wave (a workgroup of 64) per point: the D counters in LDS (D <= SM_HIST) or, zeroed first, in the
//       point's own output row as integers (atomics at device scope, converted in place); every lane draws pairs of trials from one
//       Philox block through the alias table.
//   sample_mult_sparse_kernel  one wave per point, twice: the draws go to LDS, a bitonic sort orders them, the starts of the runs of equal
//       categories are counted (pass 1: cnt[i]; the offsets are csc_io.hip's scan) or listed and written out run-length encoded
//       (pass 2: row indices strictly increasing, counts >= 1).  Both passes redo the same counter-based draws.
// Vector stores only; every LDS word a result depends on is written in front of its read within the same tile / point.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "sample_device.h"

namespace dpmm {

// ---- cluster of a position: the largest k < K with start[k] <= v (start non-decreasing, start[0] <= v): empty clusters are skipped
template <typename T>
__device__ __forceinline__ int sample_find(const T *__restrict__ start, int K, T v) {
    int lo = 0, hi = K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- NIW -----------------------------------------------------------------------------------------------------------------------
constexpr int SN_THREADS = 256;
constexpr int SN_PPT = 16;               // points per thread of the product: four groups per 64-point tile

template <int DPMAX>                     // rows of the z tile: 64 (D <= 64) or 256
__global__ __launch_bounds__(SN_THREADS) void sample_niw_kernel(SampleArgs A, int ntiles, int chunk, int FW) {
    __shared__ __attribute__((aligned(16))) float zs[DPMAX * 64];
    __shared__ float sc[64];
    const int D = A.D, K = A.K;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nb4 = (D + 3) >> 2;
    // product roles: FW feature lanes (a power of two <= 64), 64 / FW point groups side by side in a wave
    const int fl = lane & (FW - 1), pgl = lane / FW, PGW = 64 / FW;
    const int NPB = PGW >= 4 ? 1 : 4 / PGW;                 // passes over the four point groups
    const int NFC = (D + FW - 1) / FW;                      // feature chunks
    const int t_end = min(ntiles, (int)(blockIdx.x + 1) * chunk);
    for (int tile = blockIdx.x * chunk; tile < t_end; ++tile) {
        const int k = sample_find<int32_t>(A.tstart, K, tile);
        const int64_t j0 = A.cstart[k] + (int64_t)(tile - A.tstart[k]) * 64;          // first point of the tile, relative to the call
        const int64_t left = A.cstart[k + 1] - j0;
        const int cnt = left < 64 ? (int)left : 64;
        __syncthreads();                                    // the previous tile's product has read zs and sc
        if (wave == 0 && lane < cnt) {
            const double df = (double)A.df[k];
            sc[lane] = (float)sqrt(df / sample_chi2(df, A.seed, (uint64_t)(A.i0 + j0 + lane)));
            if (A.labels) A.labels[j0 + lane] = (int64_t)k + 1;
        }
        if (lane < cnt) {
            const uint64_t gi = (uint64_t)(A.i0 + j0 + lane);
            for (int j = wave; j < nb4; j += SN_THREADS / 64) {
                const Philox4 r = philox4x32_10(A.seed, gi, (uint32_t)j, STREAM_SAMPLE_NORMAL);
                const float r0 = sqrtf(fmaxf(-2.0f * __logf(sample_u32(r.v[0])), 0.0f)), t0 = 6.2831853071795865f * sample_u32(r.v[1]);
                const float r1 = sqrtf(fmaxf(-2.0f * __logf(sample_u32(r.v[2])), 0.0f)), t1 = 6.2831853071795865f * sample_u32(r.v[3]);
                float *z = zs + (4 * j) * 64 + lane;
                z[0] = r0 * __cosf(t0);
                z[64] = r0 * __sinf(t0);
                z[128] = r1 * __cosf(t1);
                z[192] = r1 * __sinf(t1);
            }
        }
        __syncthreads();
        const float *At = A.At + (int64_t)k * D * D;
        for (int item = wave; item < NFC * NPB; item += SN_THREADS / 64) {
            const int fc = item / NPB, pg = (item - fc * NPB) * PGW + pgl;
            const int a0 = fc * FW, a = a0 + fl;
            if (pg >= 4) continue;                          // (FW < 16: more lane slots than point groups)
            const bool fa = a < D;
            const int ac = fa ? a : 0;
            float acc[SN_PPT];
#pragma unroll
            for (int p = 0; p < SN_PPT; ++p) acc[p] = 0.f;
            const float4 *zrow = reinterpret_cast<const float4 *>(zs + pg * SN_PPT);
#pragma unroll 4
            for (int b = a0; b < D; ++b) {
                const float av = At[(int64_t)b * D + ac];
#pragma unroll
                for (int q = 0; q < SN_PPT / 4; ++q) {
                    const float4 zv = zrow[b * 16 + q];
                    acc[4 * q + 0] = __builtin_fmaf(av, zv.x, acc[4 * q + 0]);
                    acc[4 * q + 1] = __builtin_fmaf(av, zv.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = __builtin_fmaf(av, zv.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = __builtin_fmaf(av, zv.w, acc[4 * q + 3]);
                }
            }
            if (fa) {
                const float mk = A.m[(int64_t)k * D + a];
                float *xo = A.x + (j0 + pg * SN_PPT) * A.ld + a;
#pragma unroll
                for (int p = 0; p < SN_PPT; ++p)
                    if (pg * SN_PPT + p < cnt) xo[(int64_t)p * A.ld] = __builtin_fmaf(sc[pg * SN_PPT + p], acc[p], mk);
            }
        }
    }
}

hipError_t launch_sample_niw(const SampleArgs &a, int ntiles, int cus, hipStream_t s) {
    if (ntiles <= 0) return hipSuccess;
    if (a.D < 1 || a.D > 256 || a.K < 1) return hipErrorInvalidValue;
    int FW = 1;
    while (FW < a.D && FW < 64) FW <<= 1;
    const int want = cus * (a.D <= 64 ? 8 : 2);              // resident workgroups: 16 KB / 64 KB of LDS each
    const int chunk = (ntiles + want - 1) / want;
    const int grid = (ntiles + chunk - 1) / chunk;
    if (a.D <= 64) DPMM_LAUNCH((sample_niw_kernel<64>), dim3(grid), dim3(SN_THREADS), 0, s, a, ntiles, chunk, FW);
    else DPMM_LAUNCH((sample_niw_kernel<256>), dim3(grid), dim3(SN_THREADS), 0, s, a, ntiles, chunk, FW);
    return hipGetLastError();
}

// ---- Multinomial ---------------------------------------------------------------------------------------------------------------
// one trial: bucket j = (r0 * D) >> 32, category j if r1 < thr[j] else alias[j].  Integers only: a numpy restatement gives the same bits.
__device__ __forceinline__ uint32_t sample_alias(const uint32_t *__restrict__ thr, const int32_t *__restrict__ alias, uint32_t D, uint32_t r0, uint32_t r1) {
    const uint32_t j = __umulhi(r0, D);
    return r1 < thr[j] ? j : (uint32_t)alias[j];
}

constexpr int SM_HIST = 4096;            // counters of a point held in LDS (16 KB); more features count in the output row itself
constexpr int SM_SORT = 4096;            // == DPMM_SAMPLE_MAX_TRIALS_SPARSE: one point's draws in LDS

template <bool LDSH>
__global__ __launch_bounds__(64) void sample_mult_dense_kernel(SampleArgs A) {
    __shared__ uint32_t h[LDSH ? SM_HIST : 1];
    const int lane = threadIdx.x;
    const int D = A.D;
    const uint32_t nblk = (uint32_t)((A.trials + 1) >> 1);
    for (int64_t j = blockIdx.x; j < A.n; j += gridDim.x) {
        const int k = sample_find<int64_t>(A.cstart, A.K, j);
        const uint32_t *thr = A.thr + (int64_t)k * D;
        const int32_t *alias = A.alias + (int64_t)k * D;
        float *row = A.x + j * A.ld;
        uint32_t *cnt = LDSH ? h : reinterpret_cast<uint32_t *>(row);
        for (int d = lane; d < D; d += 64) cnt[d] = 0u;
        if (!LDSH) __threadfence();                         // the zeros are in memory in front of the atomics of the other lanes
        __syncthreads();
        const uint64_t gi = (uint64_t)(A.i0 + j);
        for (uint32_t b = lane; b < nblk; b += 64) {
            const Philox4 r = philox4x32_10(A.seed, gi, b, STREAM_SAMPLE_MULT);
            atomicAdd(&cnt[sample_alias(thr, alias, (uint32_t)D, r.v[0], r.v[1])], 1u);
            if (2 * (int64_t)b + 1 < A.trials) atomicAdd(&cnt[sample_alias(thr, alias, (uint32_t)D, r.v[2], r.v[3])], 1u);
        }
        if (!LDSH) __threadfence();
        __syncthreads();
        if (LDSH) {
            for (int d = lane; d < D; d += 64) row[d] = (float)h[d];
        } else {
            for (int d = lane; d < D; d += 64)
                row[d] = (float)__hip_atomic_load(&cnt[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (A.labels && lane == 0) A.labels[j] = (int64_t)k + 1;
        __syncthreads();                                    // the counters are read in front of the next point's zeros
    }
}

template <bool FILL>
__global__ __launch_bounds__(64) void sample_mult_sparse_kernel(SampleArgs A) {
    __shared__ uint32_t sv[SM_SORT];
    __shared__ uint32_t st[FILL ? SM_SORT : 1];
    const int lane = threadIdx.x;
    const int D = A.D;
    const int trials = (int)A.trials;                       // <= SM_SORT (the launcher refuses more)
    const uint32_t nblk = (uint32_t)((trials + 1) >> 1);
    int P = 2;
    while (P < trials) P <<= 1;                             // <= SM_SORT
    for (int64_t j = blockIdx.x; j < A.n; j += gridDim.x) {
        const int k = sample_find<int64_t>(A.cstart, A.K, j);
        const uint32_t *thr = A.thr + (int64_t)k * D;
        const int32_t *alias = A.alias + (int64_t)k * D;
        const uint64_t gi = (uint64_t)(A.i0 + j);
        for (uint32_t b = lane; b < nblk; b += 64) {
            const Philox4 r = philox4x32_10(A.seed, gi, b, STREAM_SAMPLE_MULT);
            sv[2 * b] = sample_alias(thr, alias, (uint32_t)D, r.v[0], r.v[1]);
            if (2 * (int)b + 1 < trials) sv[2 * b + 1] = sample_alias(thr, alias, (uint32_t)D, r.v[2], r.v[3]);
        }
        for (int t = trials + lane; t < P; t += 64) sv[t] = 0xFFFFFFFFu;      // behind every category
        __syncthreads();
        for (int kk = 2; kk <= P; kk <<= 1) {
            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                for (int t = lane; t < P; t += 64) {
                    const int o = t ^ jj;
                    if (o > t) {
                        const uint32_t x0 = sv[t], x1 = sv[o];
                        if ((x0 > x1) == ((t & kk) == 0)) { sv[t] = x1; sv[o] = x0; }
                    }
                }
                __syncthreads();
            }
        }
        // the starts of the runs of equal categories, in order
        int nd = 0;
        for (int t0 = 0; t0 < trials; t0 += 64) {
            const int t = t0 + lane;
            const bool first = t < trials && (t == 0 || sv[t] != sv[t - 1]);
            const unsigned long long mask = __ballot(first);
            if (FILL && first) st[nd + __popcll(mask & ((1ull << lane) - 1ull))] = (uint32_t)t;
            nd += __popcll(mask);
        }
        if (!FILL) {
            if (lane == 0) A.cnt[j] = nd;
        } else {
            __syncthreads();
            const int64_t off = A.colptr[j];
            for (int r = lane; r < nd; r += 64) {
                const uint32_t t = st[r], e = r + 1 < nd ? st[r + 1] : (uint32_t)trials;
                const int64_t o = off + r;
                if (o >= 0 && o < A.extent) {               // (offsets that are not the first pass's address nothing outside the arrays)
                    A.rowval[o] = (int64_t)sv[t];
                    A.nzval[o] = (float)(e - t);
                }
            }
        }
        __syncthreads();                                    // sv / st are read in front of the next point's draws
    }
}

__global__ __launch_bounds__(256) void sample_add_i64_kernel(int64_t *__restrict__ p, int64_t n, int64_t v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] += v;
}

static int sample_grid(int64_t n) { return (int)(n < 16384 ? n : 16384); }

hipError_t launch_sample_mult_dense(const SampleArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.D < 1 || a.K < 1 || a.trials < 1 || a.trials > (1 << 24)) return hipErrorInvalidValue;
    if (a.D <= SM_HIST) DPMM_LAUNCH((sample_mult_dense_kernel<true>), dim3(sample_grid(a.n)), dim3(64), 0, s, a);
    else DPMM_LAUNCH((sample_mult_dense_kernel<false>), dim3(sample_grid(a.n)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sample_mult_sparse(const SampleArgs &a, bool fill, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.D < 1 || a.K < 1 || a.trials < 1 || a.trials > SM_SORT) return hipErrorInvalidValue;
    if (fill) DPMM_LAUNCH((sample_mult_sparse_kernel<true>), dim3(sample_grid(a.n)), dim3(64), 0, s, a);
    else DPMM_LAUNCH((sample_mult_sparse_kernel<false>), dim3(sample_grid(a.n)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sample_add_i64(int64_t *p, int64_t n, int64_t v, hipStream_t s) {
    if (n <= 0 || v == 0) return hipSuccess;
    const int64_t g = (n + 255) / 256;
    DPMM_LAUNCH(sample_add_i64_kernel, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(256), 0, s, p, n, v);
    return hipGetLastError();
}

}  // namespace dpmm
