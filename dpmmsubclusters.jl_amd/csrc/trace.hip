// trace.hip -- label samples kept on the device (include/dpmm_hip_trace.h): recording a labelling as 16-bit cluster ids, contingency
// tables between pairs of recorded labellings, the per-point mean of table entries, and reading a labelling back.
//
// A row of the trace holds n ids and is padded to a multiple of 8 ids (16 bytes) with 0xFFFF, which is above every K
// (DPMM_MAX_CLUSTERS = 1024): the kernels below walk whole 16-byte vectors, 8 points per lane and load, and the padding counts nowhere
// without a bounds test of its own.  nvec = vectors of a row.
//
// Tables.  The host packs consecutive pairs (s, t) of one row slot s into a GROUP while their cells fit TRACE_LDS_CELLS 32-bit counters
// (64 KiB of LDS: two workgroups on a CU at the full budget, more when a launch's groups are smaller -- the LDS of a launch is that of
// its largest group).  A workgroup owns one group (blockIdx.y) and one contiguous chunk of points (blockIdx.x): per vector it loads z_s
// once and every z_t of the group once, and does one non-returning LDS add per (point, pair).  Afterwards the non-zero cells go to the
// Int64 device image of the result with 64-bit global adds.  Sums of integers: the result does not depend on the grouping, on the grid
// or on the order of the adds.  A 32-bit counter counts the points of one workgroup's chunk, below 2^32.  A single pair with more
// cells than the budget (300 x 300) adds straight into the global table, as contingency_kernel (labels.hip) does above 8192 cells.
#include "dpmm_device.h"
#include "dpmm_kernels.h"

namespace dpmm {

constexpr int TRACE_THREADS = 512;

static inline int trace_grid(int64_t items, int threads) {
    int64_t g = (items + threads - 1) / threads;
    if (g > 256 * 8) g = 256 * 8;
    if (g < 1) g = 1;
    return (int)g;
}

__device__ __forceinline__ void trace_unpack(const uint4 v, unsigned (&z)[8]) {
    z[0] = v.x & 0xFFFFu; z[1] = v.x >> 16; z[2] = v.y & 0xFFFFu; z[3] = v.y >> 16;
    z[4] = v.z & 0xFFFFu; z[5] = v.z >> 16; z[6] = v.w & 0xFFFFu; z[7] = v.w >> 16;
}

__device__ __forceinline__ unsigned trace_id(int bin) {      // bins = 2 * (label - 1) + (sub - 1); ids above 65534 (never a cluster) saturate
    const unsigned z = (unsigned)(bin >> 1);
    return z < 0xFFFFu ? z : 0xFFFFu;
}

// row[0 .. 8 * nvec) = ids of bins[0 .. n), then 0xFFFF
__global__ __launch_bounds__(256) void trace_record_kernel(const int32_t *__restrict__ bins, int64_t n, uint4 *__restrict__ row, int64_t nvec) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x) {
        unsigned z[8];
        if (8 * v + 8 <= n) {
            const int4 lo = reinterpret_cast<const int4 *>(bins)[2 * v], hi = reinterpret_cast<const int4 *>(bins)[2 * v + 1];
            z[0] = trace_id(lo.x); z[1] = trace_id(lo.y); z[2] = trace_id(lo.z); z[3] = trace_id(lo.w);
            z[4] = trace_id(hi.x); z[5] = trace_id(hi.y); z[6] = trace_id(hi.z); z[7] = trace_id(hi.w);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) z[e] = (8 * v + e < n) ? trace_id(bins[8 * v + e]) : 0xFFFFu;
        }
        row[v] = make_uint4(z[0] | (z[1] << 16), z[2] | (z[3] << 16), z[4] | (z[5] << 16), z[6] | (z[7] << 16));
    }
}
hipError_t launch_trace_record(const int32_t *bins, int64_t n, uint16_t *row, int64_t nvec, hipStream_t s) {
    if (nvec <= 0) return hipSuccess;
    DPMM_LAUNCH(trace_record_kernel, dim3(trace_grid(nvec, 256)), dim3(256), 0, s, bins, n, reinterpret_cast<uint4 *>(row), nvec);
    return hipGetLastError();
}

__global__ __launch_bounds__(TRACE_THREADS) void trace_tables_kernel(const TraceGroup *__restrict__ groups, const TracePair *__restrict__ pairs,
                                                                     int64_t nvec) {
    extern __shared__ unsigned int tab[];
    const TraceGroup g = groups[blockIdx.y];
    const TracePair *__restrict__ P = pairs + g.pair0;
    const int tid = threadIdx.x;
    for (int c = tid; c < g.cells; c += TRACE_THREADS) tab[c] = 0u;
    __syncthreads();
    const int64_t per = (nvec + gridDim.x - 1) / gridDim.x;
    const int64_t v0 = (int64_t)blockIdx.x * per, v1 = min(nvec, v0 + per);
    const uint4 *__restrict__ zs = reinterpret_cast<const uint4 *>(g.zs);
    const unsigned Ks = (unsigned)g.Ks;
    for (int64_t v = v0 + tid; v < v1; v += TRACE_THREADS) {
        unsigned a[8];
        trace_unpack(zs[v], a);
        for (int p = 0; p < g.npairs; ++p) {
            const unsigned Kt = (unsigned)P[p].Kt, cell0 = P[p].cell0;
            unsigned b[8];
            trace_unpack(reinterpret_cast<const uint4 *>(P[p].zt)[v], b);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (a[e] < Ks && b[e] < Kt) atomicAdd(&tab[cell0 + a[e] * Kt + b[e]], 1u);      // (result unused: a non-returning ds_add)
        }
    }
    __syncthreads();
    for (int p = 0; p < g.npairs; ++p) {
        const int cells = g.Ks * P[p].Kt;
        const unsigned *__restrict__ t = tab + P[p].cell0;
        unsigned long long *__restrict__ out = P[p].out;
        for (int c = tid; c < cells; c += TRACE_THREADS)
            if (t[c]) atomicAdd(&out[c], (unsigned long long)t[c]);
    }
}
// groups [ngroups], every group within TRACE_LDS_CELLS; max_cells the largest of them.  gridDim.y is limited to 65535: longer lists go in pieces.
hipError_t launch_trace_tables(const TraceGroup *groups, int ngroups, const TracePair *pairs, int max_cells, int64_t nvec, hipStream_t s) {
    if (ngroups <= 0 || nvec <= 0) return hipSuccess;
    // a handful of workgroups per CU (256 CUs) over all groups, each with a chunk of at least 4 trips of the block
    int64_t chunks = (256 * 8 + ngroups - 1) / ngroups;
    const int64_t longest = (nvec + 4 * TRACE_THREADS - 1) / (4 * TRACE_THREADS);
    if (chunks > longest) chunks = longest;
    if (chunks < 1) chunks = 1;
    for (int g0 = 0; g0 < ngroups; g0 += 65535) {
        const int ng = ngroups - g0 < 65535 ? ngroups - g0 : 65535;
        DPMM_LAUNCH(trace_tables_kernel, dim3((unsigned)chunks, (unsigned)ng), dim3(TRACE_THREADS), sizeof(unsigned) * (size_t)max_cells, s, groups + g0, pairs, nvec);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// one pair whose table does not fit the LDS budget: 64-bit adds straight into the global table
__global__ __launch_bounds__(256) void trace_pair_global_kernel(const uint4 *__restrict__ zs, const uint4 *__restrict__ zt, unsigned Ks, unsigned Kt,
                                                                int64_t nvec, unsigned long long *__restrict__ out) {
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x) {
        unsigned a[8], b[8];
        trace_unpack(zs[v], a);
        trace_unpack(zt[v], b);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (a[e] < Ks && b[e] < Kt) atomicAdd(&out[(size_t)a[e] * Kt + b[e]], 1ull);
    }
}
hipError_t launch_trace_pair_global(const uint16_t *zs, const uint16_t *zt, int Ks, int Kt, int64_t nvec, unsigned long long *out, hipStream_t s) {
    if (nvec <= 0) return hipSuccess;
    DPMM_LAUNCH(trace_pair_global_kernel, dim3(trace_grid(nvec, 256)), dim3(256), 0, s, reinterpret_cast<const uint4 *>(zs),
                reinterpret_cast<const uint4 *>(zt), (unsigned)Ks, (unsigned)Kt, nvec, out);
    return hipGetLastError();
}

// out[i] = (sum over the listed slots, in order, of ratio_j[za_i][z_j,i]) / ns: one lane owns 8 points and adds their terms in the listed order
__global__ __launch_bounds__(256) void trace_confidence_kernel(const uint4 *__restrict__ za, unsigned Ka, const TraceConfSlot *__restrict__ S, int ns,
                                                               const float *__restrict__ ratio, int64_t n, int64_t nvec, float *__restrict__ out,
                                                               int out_vec) {
    const float den = (float)ns;
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * blockDim.x) {
        unsigned a[8];
        trace_unpack(za[v], a);
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
        for (int j = 0; j < ns; ++j) {
            const unsigned K = (unsigned)S[j].K;
            const float *__restrict__ r = ratio + S[j].off;
            unsigned b[8];
            trace_unpack(reinterpret_cast<const uint4 *>(S[j].z)[v], b);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (a[e] < Ka && b[e] < K) ? r[a[e] * K + b[e]] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = acc[e] / den;
        if (out_vec && 8 * v + 8 <= n) {
            reinterpret_cast<float4 *>(out)[2 * v] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            reinterpret_cast<float4 *>(out)[2 * v + 1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (8 * v + e < n) out[8 * v + e] = acc[e];
        }
    }
}
hipError_t launch_trace_confidence(const uint16_t *za, int Ka, const TraceConfSlot *slots, int ns, const float *ratio, int64_t n, int64_t nvec,
                                   float *out, hipStream_t s) {
    if (nvec <= 0 || n <= 0) return hipSuccess;
    const int out_vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0 ? 1 : 0;
    DPMM_LAUNCH(trace_confidence_kernel, dim3(trace_grid(nvec, 256)), dim3(256), 0, s, reinterpret_cast<const uint4 *>(za), (unsigned)Ka, slots, ns, ratio,
                n, nvec, out, out_vec);
    return hipGetLastError();
}

__global__ void trace_read_kernel(const uint16_t *__restrict__ row, int64_t n, int64_t *__restrict__ labels) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) labels[i] = (int64_t)row[i] + 1;
}
hipError_t launch_trace_read(const uint16_t *row, int64_t n, int64_t *labels, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    DPMM_LAUNCH(trace_read_kernel, dim3(trace_grid(n, 256)), dim3(256), 0, s, row, n, labels);
    return hipGetLastError();
}

}  // namespace dpmm
