// csc_io.hip -- sparse points (compressed sparse columns, one column = one point) out of caller-owned DEVICE memory into the storage
// mult_sparse.hip reads (include/dpmm_hip_csc.h): offsets Int32 / Int64, rows of the same type, values of any of the eight element
// types, read in place; cp [n + 1] Int64, ri UInt16, val Float32 written.  Three phases, nothing but two 8-byte words crosses to the host:
//
//   csc_dev_check_kernel<I, V>    A WAVE owns a run of CSC_RUN consecutive points, hence one contiguous run of entries.  It validates the
//                                 run's offsets FIRST (inside [0, extent], non-decreasing, at most D entries), keeps them in its slice of
//                                 LDS, and then streams the entries of the points in front of the first bad offset only -- 64 consecutive
//                                 entries per load instruction, CSC_U loads in flight per lane -- so no entry is addressed through an
//                                 offset that was not checked.  The column of an entry is found by bisection in the LDS offsets; per entry:
//                                 row in [0, D), and greater than its predecessor unless it is the first of its column; per point:
//                                 cnt[i] = values that are not zero after rounding to Float32 (a segmented wave ballot, one LDS update per
//                                 column and load).  The first offender goes to bad[0] by atomicMin of
//                                     point << 20 | (position in the column + 1) << 3 | reason       (position 0: the point's offsets)
//                                 which orders the defects of a point as csc_check_kernel (mult_sparse.hip) decides them: that kernel, too,
//                                 reports a column of more than D entries as "not strictly increasing" from its offsets, WITHOUT walking
//                                 it, and otherwise the first defective entry of its walk, range before order.
//   csc_scan_*_kernel             exclusive scan of cnt (Int32) into cp_out (Int64) in three passes: totals of tiles of CSC_SCAN_TILE
//                                 points, a one-workgroup scan of those totals, the offsets.  No workgroup waits for another.
//   csc_dev_compact_kernel<I, V>  the same runs: entry order is kept and a run's output starts at cp_out[first point], so an entry goes to
//                                 that base + the kept entries in front of it in the run: a ballot prefix plus a running base.  Reads
//                                 and writes are consecutive along the lanes.
//
// Waves take their runs in a grid-stride loop; a column of 65536 entries is 256 rounds of one wave.  Values are rounded by the to_f32 of
// tensor_elem.h, the code the dense ingest uses.  Index arithmetic is Int64 throughout.
#include <algorithm>
#include "dpmm_kernels.h"
#include "tensor_elem.h"

namespace dpmm {

constexpr int CSC_BLOCK = 256;                 // four waves, each with runs of its own: no barrier in the check and compact kernels
constexpr int CSC_WAVES = CSC_BLOCK / 64;
constexpr int CSC_RUN = 64;                    // points per run: lane l holds the offsets of the run's point l
constexpr int CSC_U = 4;                       // loads of 64 consecutive entries in flight per wave
constexpr int CSC_MAX_GRID = 2048;

__device__ __forceinline__ unsigned long long csc_bad_key(int64_t point, int64_t pos1, int reason) {
    return ((unsigned long long)point << 20) | ((unsigned long long)pos1 << 3) | (unsigned)reason;
}

template <typename I, typename V>
__global__ __launch_bounds__(CSC_BLOCK) void csc_dev_check_kernel(const I *__restrict__ cp, const I *__restrict__ rv, const V *__restrict__ nz, int64_t n,
                                                                  int64_t extent, int D, int base, int32_t *__restrict__ cnt,
                                                                  unsigned long long *__restrict__ bad) {
    __shared__ int64_t s_off[CSC_WAVES][CSC_RUN + 1];
    __shared__ int32_t s_cnt[CSC_WAVES][CSC_RUN];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t *off = s_off[wave];
    int32_t *kc = s_cnt[wave];
    const int64_t nruns = (n + CSC_RUN - 1) / CSC_RUN;
    for (int64_t r = (int64_t)blockIdx.x * CSC_WAVES + wave; r < nruns; r += (int64_t)gridDim.x * CSC_WAVES) {
        const int64_t p0 = r * CSC_RUN;
        const int npt = (int)min((int64_t)CSC_RUN, n - p0);
        const bool valid = lane < npt;
        // ---- the offsets of my point, before anything is read through them
        const int64_t lo = valid ? (int64_t)cp[p0 + lane] - base : 0;
        const int64_t hi = valid ? (int64_t)cp[p0 + lane + 1] - base : 0;
        int reason = 0;
        if (valid) {
            if (lo < 0 || lo > extent || hi < 0 || hi > extent) reason = CSC_BAD_OUTSIDE;
            else if (hi < lo) reason = CSC_BAD_DECREASES;
            else if (hi - lo > D) reason = CSC_BAD_ORDER;             // (more entries than features: some index repeats -- decided here, before any
                                                                      // entry, as csc_check_kernel does; it also keeps position + 1 <= D inside 17 bits)
        }
        const unsigned long long badmask = __ballot(reason != 0);
        const int nproc = badmask ? (int)__builtin_ctzll(badmask) : npt;      // the points in front of the first bad offset: their entries
        if (reason && lane == nproc) atomicMin(bad, csc_bad_key(p0 + lane, 0, reason));      // are one run inside [0, extent]
        if (valid) off[lane] = lo;
        if (lane == npt - 1) off[npt] = hi;
        kc[lane] = 0;
        __threadfence_block();
        const int64_t e_begin = off[0], e_end = nproc > 0 ? off[nproc] : e_begin;
        // ---- the entries
        for (int64_t b = e_begin; b < e_end; b += 64 * CSC_U) {
            I row[CSC_U];
            V raw[CSC_U];
#pragma unroll
            for (int u = 0; u < CSC_U; ++u) {
                const int64_t e = b + 64 * u + lane;
                row[u] = e < e_end ? rv[e] : I{};
                raw[u] = e < e_end ? nz[e] : V{};
            }
#pragma unroll
            for (int u = 0; u < CSC_U; ++u) {
                const int64_t e = b + 64 * u + lane;
                const bool act = e < e_end;
                int p = 0;                                             // the last point whose first entry is not behind e
                if (act) {
                    int len = nproc;
                    while (len > 1) {
                        const int half = len >> 1;
                        if (off[p + half] <= e) { p += half; len -= half; } else len = half;
                    }
                }
                const int64_t d = (int64_t)row[u] - base;
                const int64_t first_e = act ? off[p] : 0;
                int64_t pd = __shfl_up(d, 1);
                if (lane == 0 && act && e > first_e) pd = (int64_t)rv[e - 1] - base;     // (the lane in front belongs to the load before)
                if (act) {
                    int rs = 0;
                    if (d < 0 || d >= D) rs = CSC_BAD_RANGE;
                    else if (e > first_e && d <= pd) rs = CSC_BAD_ORDER;
                    if (rs) atomicMin(bad, csc_bad_key(p0 + p, e - first_e + 1, rs));
                }
                // kept values per column: the lanes of one column are consecutive
                const bool kept = act && to_f32(raw[u]) != 0.f;
                const int pp = __shfl_up(p, 1);
                const bool head = act && (lane == 0 || p != pp);
                const unsigned long long hm = __ballot(head), km = __ballot(kept);
                if (head) {
                    const unsigned long long above = lane == 63 ? 0ull : hm >> (lane + 1);
                    const int next = above ? lane + 1 + (int)__builtin_ctzll(above) : 64;
                    const unsigned long long upto = next == 64 ? ~0ull : (1ull << next) - 1ull;
                    // Plain read-modify-write of LDS, no atomic: only THIS wave touches kc[], a column has one head lane per load (its
                    // lanes are consecutive), and the DS operations of one wave are issued in order, so the updates of successive loads
                    // to the same kc[p] follow each other.  A run shared by several waves would need atomicAdd here and barriers around off[].
                    kc[p] += __popcll(km & upto & ~((1ull << lane) - 1ull));
                }
            }
        }
        __threadfence_block();
        if (valid) cnt[p0 + lane] = kc[lane];
        __threadfence_block();                  // the slice is reused by this wave's next run
    }
}

template <typename I, typename V>
__global__ __launch_bounds__(CSC_BLOCK) void csc_dev_compact_kernel(const I *__restrict__ cp, const I *__restrict__ rv, const V *__restrict__ nz, int64_t n,
                                                                    int base, const int64_t *__restrict__ cp_out, uint16_t *__restrict__ ri,
                                                                    float *__restrict__ val) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nruns = (n + CSC_RUN - 1) / CSC_RUN;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int64_t r = (int64_t)blockIdx.x * CSC_WAVES + wave; r < nruns; r += (int64_t)gridDim.x * CSC_WAVES) {
        const int64_t p0 = r * CSC_RUN;
        const int64_t p1 = min(p0 + CSC_RUN, n);
        const int64_t e_end = (int64_t)cp[p1] - base;
        int64_t o = cp_out[p0];
        for (int64_t b = (int64_t)cp[p0] - base; b < e_end; b += 64 * CSC_U) {
            I row[CSC_U];
            V raw[CSC_U];
#pragma unroll
            for (int u = 0; u < CSC_U; ++u) {
                const int64_t e = b + 64 * u + lane;
                row[u] = e < e_end ? rv[e] : I{};
                raw[u] = e < e_end ? nz[e] : V{};
            }
#pragma unroll
            for (int u = 0; u < CSC_U; ++u) {
                const float v = to_f32(raw[u]);
                const bool kept = b + 64 * u + lane < e_end && v != 0.f;
                const unsigned long long km = __ballot(kept);
                if (kept) {
                    const int64_t at = o + __popcll(km & below);
                    ri[at] = (uint16_t)((int64_t)row[u] - base);
                    val[at] = v;
                }
                o += __popcll(km);
            }
        }
    }
}

// ---- cnt [n] Int32 -> cp_out [n + 1] Int64, exclusive.  A thread holds CSC_SCAN_PER consecutive elements of its tile.
constexpr int CSC_SCAN_PER = CSC_SCAN_TILE / CSC_BLOCK;

// exclusive prefix of v over the workgroup and the workgroup's total; ws: CSC_WAVES words of LDS (synchronised here for reuse)
__device__ __forceinline__ int64_t csc_block_scan(int64_t v, int64_t *ws, int64_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t incl = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int64_t t = __shfl_up(incl, s);
        if (lane >= s) incl += t;
    }
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    int64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CSC_WAVES; ++w) {
        const int64_t t = ws[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

__global__ __launch_bounds__(CSC_BLOCK) void csc_scan_totals_kernel(const int32_t *__restrict__ cnt, int64_t n, int64_t ntiles, int64_t *__restrict__ bt) {
    __shared__ int64_t ws[CSC_WAVES];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t i0 = t * CSC_SCAN_TILE + (int64_t)threadIdx.x * CSC_SCAN_PER;
        int64_t s = 0, total;
#pragma unroll
        for (int j = 0; j < CSC_SCAN_PER; ++j) s += i0 + j < n ? cnt[i0 + j] : 0;
        csc_block_scan(s, ws, &total);
        if (threadIdx.x == 0) bt[t] = total;
    }
}

// one workgroup: bt [ntiles] totals -> exclusive offsets in place, bt[ntiles] = the sum of all
__global__ __launch_bounds__(CSC_BLOCK) void csc_scan_top_kernel(int64_t *__restrict__ bt, int64_t ntiles) {
    __shared__ int64_t ws[CSC_WAVES];
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < ntiles; c0 += CSC_BLOCK) {
        const int64_t i = c0 + threadIdx.x;
        const int64_t v = i < ntiles ? bt[i] : 0;
        int64_t total;
        const int64_t ex = csc_block_scan(v, ws, &total);
        if (i < ntiles) bt[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) bt[ntiles] = carry;
}

__global__ __launch_bounds__(CSC_BLOCK) void csc_scan_final_kernel(const int32_t *__restrict__ cnt, int64_t n, int64_t ntiles, const int64_t *__restrict__ bt,
                                                                   int64_t *__restrict__ cp_out) {
    __shared__ int64_t ws[CSC_WAVES];
    if (blockIdx.x == 0 && threadIdx.x == 0) cp_out[n] = bt[ntiles];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t i0 = t * CSC_SCAN_TILE + (int64_t)threadIdx.x * CSC_SCAN_PER;
        int32_t c[CSC_SCAN_PER];
        int64_t s = 0, total;
#pragma unroll
        for (int j = 0; j < CSC_SCAN_PER; ++j) { c[j] = i0 + j < n ? cnt[i0 + j] : 0; s += c[j]; }
        int64_t o = bt[t] + csc_block_scan(s, ws, &total);
#pragma unroll
        for (int j = 0; j < CSC_SCAN_PER; ++j) {
            if (i0 + j < n) cp_out[i0 + j] = o;
            o += c[j];
        }
    }
}

// ---- launchers
static inline int csc_grid(int64_t n) {
    const int64_t nruns = (n + CSC_RUN - 1) / CSC_RUN;
    return (int)std::max<int64_t>(1, std::min<int64_t>(CSC_MAX_GRID, (nruns + CSC_WAVES - 1) / CSC_WAVES));
}

template <typename I, typename V>
static hipError_t launch_check_t(const void *cp, const void *rv, const void *nz, int64_t n, int64_t extent, int D, int base, int32_t *cnt,
                                 unsigned long long *bad, hipStream_t s) {
    DPMM_LAUNCH((csc_dev_check_kernel<I, V>), dim3(csc_grid(n)), dim3(CSC_BLOCK), 0, s, static_cast<const I *>(cp), static_cast<const I *>(rv),
                static_cast<const V *>(nz), n, extent, D, base, cnt, bad);
    return hipGetLastError();
}

template <typename I, typename V>
static hipError_t launch_compact_t(const void *cp, const void *rv, const void *nz, int64_t n, int base, const int64_t *cp_out, uint16_t *ri, float *val,
                                   hipStream_t s) {
    DPMM_LAUNCH((csc_dev_compact_kernel<I, V>), dim3(csc_grid(n)), dim3(CSC_BLOCK), 0, s, static_cast<const I *>(cp), static_cast<const I *>(rv),
                static_cast<const V *>(nz), n, base, cp_out, ri, val);
    return hipGetLastError();
}

#define CSC_BY_VALUE_TYPE(I, FN, ...)                                   \
    switch (value_dtype) {                                              \
        case 0: return FN<I, f16_bits>(__VA_ARGS__);                    \
        case 1: return FN<I, bf16_bits>(__VA_ARGS__);                   \
        case 2: return FN<I, float>(__VA_ARGS__);                       \
        case 3: return FN<I, double>(__VA_ARGS__);                      \
        case 4: return FN<I, uint8_t>(__VA_ARGS__);                     \
        case 5: return FN<I, int16_t>(__VA_ARGS__);                     \
        case 6: return FN<I, int32_t>(__VA_ARGS__);                     \
        case 7: return FN<I, int64_t>(__VA_ARGS__);                     \
        default: return hipErrorInvalidValue;                           \
    }

hipError_t launch_csc_dev_check(const void *cp, const void *rv, const void *nz, int index_i64, int value_dtype, int64_t n, int64_t extent, int D, int base,
                                int32_t *cnt, unsigned long long *bad, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (index_i64) { CSC_BY_VALUE_TYPE(int64_t, launch_check_t, cp, rv, nz, n, extent, D, base, cnt, bad, s) }
    CSC_BY_VALUE_TYPE(int32_t, launch_check_t, cp, rv, nz, n, extent, D, base, cnt, bad, s)
}

hipError_t launch_csc_dev_compact(const void *cp, const void *rv, const void *nz, int index_i64, int value_dtype, int64_t n, int base, const int64_t *cp_out,
                                  uint16_t *ri, float *val, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (index_i64) { CSC_BY_VALUE_TYPE(int64_t, launch_compact_t, cp, rv, nz, n, base, cp_out, ri, val, s) }
    CSC_BY_VALUE_TYPE(int32_t, launch_compact_t, cp, rv, nz, n, base, cp_out, ri, val, s)
}

// bt: csc_scan_tiles(n) + 1 words; afterwards bt[csc_scan_tiles(n)] == cp_out[n], the number of entries kept
hipError_t launch_csc_scan(const int32_t *cnt, int64_t n, int64_t *bt, int64_t *cp_out, hipStream_t s) {
    const int64_t ntiles = csc_scan_tiles(n);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(CSC_MAX_GRID, ntiles));
    DPMM_LAUNCH(csc_scan_totals_kernel, dim3(grid), dim3(CSC_BLOCK), 0, s, cnt, n, ntiles, bt);
    DPMM_LAUNCH(csc_scan_top_kernel, dim3(1), dim3(CSC_BLOCK), 0, s, bt, ntiles);
    DPMM_LAUNCH(csc_scan_final_kernel, dim3(grid), dim3(CSC_BLOCK), 0, s, cnt, n, ntiles, bt, cp_out);
    return hipGetLastError();
}

}  // namespace dpmm
