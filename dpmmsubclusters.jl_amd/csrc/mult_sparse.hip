// mult_sparse.hip -- the Multinomial prior on points stored as compressed sparse columns (one column = one point) on gfx950.
//
// Same functions of the reference as mult_sweep.hip and the Multinomial half of suffstats.hip stand in for, for data the
// reference cannot hold: r_i = alpha' x_i (src/distributions/multinomial_dist.jl:13-15) over the STORED entries of x_i only, and
// (N, sum x) per (cluster, sub-cluster) bin (src/priors/multinomial_prior.jl:27-32).
//
// Storage: cp [n + 1] Int64 offsets, ri [nnz] UInt16 feature indices (D <= 65536), val [nnz] Float32 values; the rows of a column are
// strictly increasing and no stored value is zero (checked / dropped at upload).  Work and HBM bytes are proportional to nnz.
//
// Sweep.  The parameter image is transposed, T [d][3K]: columns [0, K) are the cluster rows 3k, column K + 2k + s is row 3k + 1 + s, so
// what one entry needs of the K cluster rows is ONE contiguous piece.  A wave owns 64 consecutive points:
//   1. point by point, lane l accumulates column l (and l + 64) over the point's entries IN INDEX ORDER -- one multiply and one add per
//      entry, the oracle's own association (oracle/dpmm_oracle.c:149-156; a zero term adds nothing) -- entries are read once, 64 at a
//      time, and handed round with v_readlane; the K values (+ cst) go to the wave's 64 columns of the global scratch (L2);
//   2. lane l draws the label of point l from that column with the draw every Multinomial kernel makes (mult_draw_label);
//   3. lane l walks the entries of its own point once more for the two sub-cluster rows of the cluster it drew, then draw2.
// O(nnz_i (K + 2)) multiply-adds per point.  Waves take their 64-point tiles from a ticket, so a tile of long columns does not hold
// up the rest of its workgroup: there is no LDS and no barrier in the kernel.  Table mode (debug tables, predict) evaluates all 3K columns.
//
// Convention: a feature a point does not store contributes nothing, so log p = -Inf there leaves the value finite
// (0 * log 0 = 0); the dense kernels follow IEEE (0 * -Inf = NaN -> -Inf).
#include <algorithm>
#include "dpmm_device.h"
#include "dpmm_kernels.h"

namespace dpmm {

constexpr int SP_WTILE = 64;     // points per wave tile
constexpr int SP_NACC = 2;       // columns per lane and pass over a point's entries

__device__ __forceinline__ int sp_row_of_col(int col, int K) { return col < K ? 3 * col : 3 * ((col - K) >> 1) + 1 + ((col - K) & 1); }

__device__ __forceinline__ float sp_readlane_f(float v, int j) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), j)); }

__global__ __launch_bounds__(256) void mult_sparse_sweep_kernel(MultSweepArgs A, MultSparse S, int64_t nwt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = A.K, RS = 3 * K;
    const int ncols = A.labels_only ? RS : K;
    const int64_t sstride = A.scratch_stride;
    for (;;) {
        int64_t wt = 0;
        if (lane == 0) wt = (int64_t)atomicAdd(S.ticket, 1u);
        wt = ((int64_t)__builtin_amdgcn_readfirstlane((int)(wt >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)wt);
        if (wt >= nwt) break;
        const int64_t base = wt * SP_WTILE;
        const int npt = (int)min((int64_t)SP_WTILE, A.n - base);
        float *scr = A.scratch + (A.scratch_by_tile ? base : ((int64_t)blockIdx.x * 4 + wave) * SP_WTILE);
        // my own point (phases 2 and 3) and its entries
        const bool valid = lane < npt;
        const int64_t myp = base + (valid ? lane : 0);
        const int64_t mylo = S.cp[myp], myhi = valid ? S.cp[myp + 1] : mylo;
        // ---- 1. values of the columns, one point at a time
        for (int pt = 0; pt < npt; ++pt) {
            const int64_t lo = ((int64_t)__builtin_amdgcn_readlane((int)(mylo >> 32), pt) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)mylo, pt);
            const int64_t hi = ((int64_t)__builtin_amdgcn_readlane((int)(myhi >> 32), pt) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)myhi, pt);
            for (int c0 = 0; c0 < ncols; c0 += 64 * SP_NACC) {
                int col[SP_NACC];
                float acc[SP_NACC];
#pragma unroll
                for (int q = 0; q < SP_NACC; ++q) { col[q] = min(c0 + 64 * q + lane, ncols - 1); acc[q] = 0.f; }
                for (int64_t b = lo; b < hi; b += 64) {
                    const int cnt = (int)min((int64_t)64, hi - b);
                    const int64_t e = b + min(lane, cnt - 1);
                    const int dl = (int)S.ri[e];
                    const float vl = S.val[e];
#pragma unroll 4
                    for (int j = 0; j < cnt; ++j) {
                        const int d = __builtin_amdgcn_readlane(dl, j);
                        const float v = sp_readlane_f(vl, j);
                        const float *t = S.T + (size_t)d * RS;
#pragma unroll
                        for (int q = 0; q < SP_NACC; ++q) acc[q] = acc[q] + t[col[q]] * v;
                    }
                }
#pragma unroll
                for (int q = 0; q < SP_NACC; ++q) {
                    const int c = c0 + 64 * q + lane;
                    if (c < ncols) {
                        const int row = sp_row_of_col(c, K);
                        scr[(int64_t)row * sstride + pt] = acc[q] + A.cst[row];
                    }
                }
            }
        }
        if (!A.labels_only) {
            __threadfence_block();      // the column of point `lane` was written by the other lanes of this wave
            // ---- 2. label of my point
            int z = 0;
            const Philox4 rr = philox4x32_10(A.seed, (uint64_t)(A.first_index + myp), A.epoch, STREAM_SWEEP);
            if (valid) z = mult_draw_label(scr + lane, 3 * sstride, K, A.final_argmax, u01(rr.v[0]));
            // ---- 3. the two sub-cluster rows of that cluster over my own entries, in index order
            float b0 = 0.f, b1 = 0.f;
            const float *tz = S.T + K + 2 * z;
            for (int64_t e = mylo; e < myhi; ++e) {
                const float *t = tz + (size_t)S.ri[e] * RS;
                const float v = S.val[e];
                b0 = b0 + t[0] * v;
                b1 = b1 + t[1] * v;
            }
            if (valid) A.bins[myp] = 2 * z + draw2(b0 + A.cst[3 * z + 1], b1 + A.cst[3 * z + 2], u01(rr.v[1]));
            __threadfence_block();      // the scratch columns are reused by this wave's next tile
        }
    }
}

// T [d][3K] from the raw rows logp [3K][ldx]: a 32 x 32 transpose through LDS (both sides coalesced)
__global__ __launch_bounds__(256) void mult_sparse_pack_kernel(const float *__restrict__ logp, float *__restrict__ T, int K, int D, int64_t ldx) {
    __shared__ float tile[32][33];
    const int RS = 3 * K;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int ctiles = (RS + 31) / 32;
    const int64_t ntiles = (int64_t)((D + 31) / 32) * ctiles;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int c0 = (int)(tl % ctiles) * 32, d0 = (int)(tl / ctiles) * 32;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = c0 + ty + 8 * r, d = d0 + tx;
            tile[ty + 8 * r][tx] = (c < RS && d < D) ? logp[(size_t)sp_row_of_col(c, K) * ldx + d] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = d0 + ty + 8 * r, c = c0 + tx;
            if (c < RS && d < D) T[(size_t)d * RS + c] = tile[tx][ty + 8 * r];
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------ statistics
// item = (bin, <= chunk points of the sorted order), as in mult_stats_kernel; one WAVE per item owns the item's slab of D doubles in
// global memory (512 KB at D = 65536: L2, not LDS): cleared, then the item's points are added ONE AFTER THE OTHER in the order of the
// sort, the lanes spread over the entries of a point (a column holds an index once, so no two lanes meet).  Every slab element is
// therefore summed in one fixed order -- deterministic for any values, exact for counts -- and mult_reduce_kernel adds the slabs of a
// bin in item order as it does for the dense kernels.
__global__ __launch_bounds__(64) void mult_sparse_stats_kernel(StatsArgs A, MultSparse S) {
    const int total_items = A.sb.item_start[A.nbins];
    const int lane = threadIdx.x;
    for (int item = blockIdx.x; item < total_items; item += gridDim.x) {
        const int b = find_bin(A.sb.item_start, A.nbins, item);
        const int j = item - A.sb.item_start[b];
        const int bcnt = A.sb.bin_total[b];
        const int seg = A.sb.bin_start[b] + j * A.chunk;
        const int cnt = min(A.chunk, bcnt - j * A.chunk);
        double *slab = A.slabs + (int64_t)item * A.slab_stride;
        for (int d = lane; d < A.D; d += 64) slab[d] = 0.;
        __threadfence_block();
        for (int p = 0; p < cnt; ++p) {
            const int64_t i = A.sb.perm[seg + p];
            const int64_t lo = S.cp[i], hi = S.cp[i + 1];
            for (int64_t e = lo + lane; e < hi; e += 64) {
                const int d = (int)S.ri[e];
                slab[d] = slab[d] + (double)S.val[e];
            }
            __threadfence_block();      // the next point of the item may hold the same features on other lanes
        }
    }
}

// ------------------------------------------------------------------------------------ upload
// One thread per point: offsets inside [0, total], rows in [0, D) and strictly increasing; cnt[i] = stored values that are not zero.
// bad[0] = min over the offending points of (point << 2 | reason); reason 1: index out of range, 2: not strictly increasing
__global__ void csc_check_kernel(const int64_t *__restrict__ cp, const int64_t *__restrict__ rv, const float *__restrict__ nz, int64_t n, int64_t total,
                                 int D, int base, int32_t *__restrict__ cnt, unsigned long long *__restrict__ bad) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = cp[i] - cp[0], hi = cp[i + 1] - cp[0];
        int c = 0, reason = 0;
        if (lo < 0 || hi > total || lo > hi || hi - lo > D) reason = 2;       // (more entries than features: some index repeats)
        else {
            int64_t prev = -1;
            for (int64_t e = lo; e < hi; ++e) {
                const int64_t d = rv[e] - base;
                if (d < 0 || d >= D) { reason = 1; break; }
                if (d <= prev) { reason = 2; break; }
                prev = d;
                c += nz[e] != 0.f ? 1 : 0;
            }
        }
        cnt[i] = c;
        if (reason) atomicMin(bad, ((unsigned long long)i << 2) | (unsigned)reason);
    }
}

__global__ void csc_compact_kernel(const int64_t *__restrict__ cp, const int64_t *__restrict__ rv, const float *__restrict__ nz, int64_t n, int base,
                                   const int64_t *__restrict__ cp_out, uint16_t *__restrict__ ri, float *__restrict__ val) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = cp[i] - cp[0], hi = cp[i + 1] - cp[0];
        int64_t o = cp_out[i];
        for (int64_t e = lo; e < hi; ++e) {
            const float v = nz[e];
            if (v != 0.f) { ri[o] = (uint16_t)(rv[e] - base); val[o] = v; ++o; }
        }
    }
}

hipError_t launch_csc_check(const int64_t *cp, const int64_t *rv, const float *nz, int64_t n, int64_t total, int D, int base, int32_t *cnt,
                            unsigned long long *bad, hipStream_t s) {
    const int grid = (int)std::min<int64_t>(4096, (n + 255) / 256);
    DPMM_LAUNCH(csc_check_kernel, dim3(grid), dim3(256), 0, s, cp, rv, nz, n, total, D, base, cnt, bad);
    return hipGetLastError();
}

hipError_t launch_csc_compact(const int64_t *cp, const int64_t *rv, const float *nz, int64_t n, int base, const int64_t *cp_out, uint16_t *ri, float *val,
                              hipStream_t s) {
    const int grid = (int)std::min<int64_t>(4096, (n + 255) / 256);
    DPMM_LAUNCH(csc_compact_kernel, dim3(grid), dim3(256), 0, s, cp, rv, nz, n, base, cp_out, ri, val);
    return hipGetLastError();
}

hipError_t launch_mult_pack_sparse(const float *logp, float *T, int K, int D, int64_t ldx, hipStream_t s) {
    const int64_t ntiles = (int64_t)((D + 31) / 32) * ((3 * K + 31) / 32);
    DPMM_LAUNCH(mult_sparse_pack_kernel, dim3((unsigned)std::min<int64_t>(ntiles, 8192)), dim3(256), 0, s, logp, T, K, D, ldx);
    return hipGetLastError();
}

// grid: workgroups of four waves; the scratch (sweep mode) holds 256 columns per workgroup, as for the dense kernels
hipError_t launch_mult_sweep_sparse(const MultSweepArgs &a, const MultSparse &sp, int grid, hipStream_t s) {
    const int64_t nwt = (a.n + SP_WTILE - 1) / SP_WTILE;
    hipError_t e = hipMemsetAsync(sp.ticket, 0, sizeof(unsigned), s);
    if (e != hipSuccess) return e;
    const int g = (int)std::max<int64_t>(1, std::min<int64_t>(grid, (nwt + 3) / 4));
    DPMM_LAUNCH(mult_sparse_sweep_kernel, dim3(g), dim3(256), 0, s, a, sp, nwt);
    return hipGetLastError();
}

hipError_t launch_mult_stats_sparse(const StatsArgs &a, const MultSparse &sp, hipStream_t s) {
    const int grid = a.max_items < 1 ? 1 : a.max_items;
    DPMM_LAUNCH(mult_sparse_stats_kernel, dim3(grid), dim3(64), 0, s, a, sp);
    return launch_mult_reduce(a, s);
}

}  // namespace dpmm
