// holdout.hip -- the held-out points of a range of the score table, compacted in increasing index into the caller's buffers
// (include/dpmm_hip_holdout.h).  The class of a point is the one batchstats_prep_kernel gives it, formed by the same device code
// (batchstats_device.h: bs_mark_gaps, bs_table_passes, bs_class); with use_tail the range's tails were written by typicality.hip in front.
//
// Three launches per range, no atomics, nothing in them waits for another workgroup:
//   class     a workgroup per 256 points, as batchstats_prep_kernel: the workgroup's rows of X read flat for the features that are not
//             finite, lanes along i over the table, the class.  Every wave leaves its ballot of held-out points -- one 64-bit word -- and
//             the workgroup the counts of its four classes: one writer per word.
//   scan      ONE workgroup.  Thread t owns a contiguous piece of the workgroups' counts: it adds them up, the 256 sums are scanned (prefix
//             inside the wave by shuffles, the four waves' totals through LDS), and the thread walks its piece again writing to every
//             workgroup the slot of its first held-out point: the running total in device memory + the counts in front of it.  Thread 0
//             then advances the running totals.  The next range's scan -- of this call or of a later upload -- runs behind this one on the
//             stream and starts from them: ranges and uploads chain with no host synchronisation.
//   gather    a workgroup per 256 points; one with no held-out point, or whose first slot lies at or beyond cap, leaves at once.  A thread
//             ranks its point from the four ballot words (popcounts of the words in front, of the bits below its own) and puts its local
//             id into LDS at that rank; then wave w copies the rows of ranks w, w + 4, ..: lanes along the features, coalesced reads and
//             writes, the row id clamped to the range; lane 0 writes the global index.  Slots at or beyond cap are not written.
// The slot of a held-out point is (held-out points in front of it in the call sequence), a function of the points, the model and the floors
// alone: the class of a point does not depend on its neighbours, and integer sums have no order.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"
#include "batchstats_device.h"

namespace dpmm {

constexpr int HO_WAVES = HOLDOUT_THREADS / 64;

__global__ __launch_bounds__(HOLDOUT_THREADS) void holdout_class_kernel(HoldoutArgs A) {
    __shared__ unsigned gap[HOLDOUT_THREADS];
    __shared__ unsigned wc[HO_WAVES][HOLDOUT_STATE];
    const int K = A.K, D = A.D, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ldx = (int)A.ldx;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    const int64_t base = (int64_t)blockIdx.x * HOLDOUT_THREADS;      // (< A.n: the grid is holdout_groups(A.n))
    gap[tid] = 0;
    __syncthreads();
    const int rows = (int)(A.n - base < HOLDOUT_THREADS ? A.n - base : HOLDOUT_THREADS);
    bs_mark_gaps(gap, A.X + base * A.ldx, rows, ldx, D, tid, HOLDOUT_THREADS);
    const int64_t i = base + tid;
    const bool valid = i < A.n;
    const float *col = A.table + (valid ? i : 0);      // (lanes past the end read point 0 and contribute nothing)
    float m, s;
    int best;
    bool nan_seen;
    bs_table_passes(col, rs, K, m, best, nan_seen, s);
    __syncthreads();
    bool scored, held, incomplete, part;
    bs_class(valid, nan_seen, m, s, gap[tid], A.use_floor, A.min_logdens, A.use_tail, A.min_tail, A.tail, i, scored, held, incomplete, part);
    const unsigned long long hm = __ballot(held), sm = __ballot(valid && !scored), im = __ballot(incomplete), pm = __ballot(part);
    if (lane == 0) {
        A.ballot[(int64_t)blockIdx.x * HO_WAVES + w] = hm;
        wc[w][0] = (unsigned)__popcll(hm);
        wc[w][1] = (unsigned)__popcll(sm);
        wc[w][2] = (unsigned)__popcll(im);
        wc[w][3] = (unsigned)__popcll(pm);
    }
    __syncthreads();
    if (tid < HOLDOUT_STATE) {
        unsigned v = 0;
#pragma unroll
        for (int u = 0; u < HO_WAVES; ++u) v += wc[u][tid];
        A.wgcount[(int64_t)blockIdx.x * HOLDOUT_STATE + tid] = v;
    }
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ unsigned ho_wave_scan(unsigned v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

__global__ __launch_bounds__(HOLDOUT_THREADS) void holdout_scan_kernel(HoldoutArgs A) {
    __shared__ unsigned wtot[HO_WAVES][HOLDOUT_STATE];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t ng = (A.n + HOLDOUT_THREADS - 1) / HOLDOUT_THREADS;      // holdout_groups(A.n)
    const int64_t per = (ng + HOLDOUT_THREADS - 1) / HOLDOUT_THREADS;
    const int64_t g0 = (int64_t)tid * per < ng ? (int64_t)tid * per : ng, g1 = g0 + per < ng ? g0 + per : ng;
    const unsigned long long before = A.state[0];      // (thread 0 rewrites it behind the barrier)
    unsigned sum[HOLDOUT_STATE] = {0, 0, 0, 0};        // (a range holds fewer than 2^31 points)
    for (int64_t g = g0; g < g1; ++g) {
#pragma unroll
        for (int c = 0; c < HOLDOUT_STATE; ++c) sum[c] += A.wgcount[g * HOLDOUT_STATE + c];
    }
    unsigned incl[HOLDOUT_STATE];
#pragma unroll
    for (int c = 0; c < HOLDOUT_STATE; ++c) incl[c] = ho_wave_scan(sum[c], lane);
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c < HOLDOUT_STATE; ++c) wtot[w][c] = incl[c];
    }
    __syncthreads();
    unsigned front = incl[0] - sum[0];                 // held-out points in front of this thread's piece
#pragma unroll
    for (int u = 0; u < HO_WAVES; ++u) front += u < w ? wtot[u][0] : 0u;
    int64_t slot = (int64_t)before + (int64_t)front;
    for (int64_t g = g0; g < g1; ++g) {
        A.wgoff[g] = slot;
        slot += A.wgcount[g * HOLDOUT_STATE];
    }
    if (tid < HOLDOUT_STATE) {
        unsigned long long v = 0;
#pragma unroll
        for (int u = 0; u < HO_WAVES; ++u) v += wtot[u][tid];
        A.state[tid] += v;                             // (state[0] was read by every thread in front of the barrier)
    }
}

__global__ __launch_bounds__(HOLDOUT_THREADS) void holdout_gather_kernel(HoldoutArgs A) {
    __shared__ int ids[HOLDOUT_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int count = (int)A.wgcount[(int64_t)blockIdx.x * HOLDOUT_STATE];
    const int64_t off = A.wgoff[blockIdx.x];
    if (count == 0 || off >= A.cap) return;            // (uniform over the workgroup)
    const int64_t base = (int64_t)blockIdx.x * HOLDOUT_THREADS;
    const int rows = (int)(A.n - base < HOLDOUT_THREADS ? A.n - base : HOLDOUT_THREADS);
    const unsigned long long *bw = A.ballot + (int64_t)blockIdx.x * HO_WAVES;
    int rank = 0;
    unsigned long long own = 0;
#pragma unroll
    for (int u = 0; u < HO_WAVES; ++u) {
        const unsigned long long word = bw[u];
        rank += u < w ? __popcll(word) : 0;
        own = u == w ? word : own;
    }
    if ((own >> lane) & 1ull) ids[rank + __popcll(own & ((1ull << lane) - 1ull))] = tid;      // (ranks 0 .. count - 1, each once)
    __syncthreads();
    const int D = A.D;
    for (int r = w; r < count; r += HO_WAVES) {
        const int64_t slot = off + r;
        if (slot >= A.cap) break;                      // (the slots grow with r)
        const int id = ids[r] < rows ? ids[r] : rows - 1;
        const float *src = A.X + (base + id) * A.ldx;
        float *dst = A.dst_points + slot * D;
        for (int d = lane; d < D; d += 64) dst[d] = src[d];
        if (lane == 0) A.dst_index[slot] = A.index0 + base + id;
    }
}

hipError_t launch_holdout_range(const HoldoutArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.D < 1 || a.D > 256 || a.ldx < a.D || a.ldx > 1024 || a.n >> 31 || a.n > a.stride || a.rstep < 1 || a.cap < 0 ||
        a.index0 < 0 || !a.table || !a.X || !a.ballot || !a.wgcount || !a.wgoff || !a.state || (a.use_tail && !a.tail) ||
        (a.cap > 0 && (!a.dst_points || !a.dst_index)))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)holdout_groups(a.n)), block(HOLDOUT_THREADS);
    DPMM_LAUNCH(holdout_class_kernel, grid, block, 0, s, a);
    DPMM_LAUNCH(holdout_scan_kernel, dim3(1), block, 0, s, a);
    if (a.cap > 0) DPMM_LAUNCH(holdout_gather_kernel, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace dpmm
