// holdout.hip -- the held-out points of a range of the score table, compacted in increasing index into the caller's buffers, for both priors
// (include/dpmm_hip_holdout.h, include/dpmm_hip_countholdout.h).  The class of a point is the one the prior's statistics give it, formed by
// the same device code: NIW batchstats_device.h (bs_mark_gaps, bs_table_passes, bs_class; with use_tail the range's tails were written by
// typicality.hip in front), Multinomial countstats_device.h (cs_mark_gaps, cs_class; with the floor per count the range's totals were written
// by launch_countstats_totals in front).  The Multinomial points come from whichever store is live: rows of Float32 for the Float32 matrix
// and its byte copy, compressed sparse columns for the sparse store.
//
// Three launches per range, no atomics, nothing in them waits for another workgroup:
//   class     (one kernel per prior) a workgroup per 256 points: the workgroup's points scanned for values that are not finite, lanes along
//             i over the table, the class.  Every wave leaves its ballot of held-out points -- one 64-bit word -- and the workgroup the
//             counts of its four classes (ho_publish_class) and -- sparse store -- the stored entries of its held-out points, sum of
//             cp[i + 1] - cp[i], a 64-bit word: one writer per word.
//   scan      ONE workgroup, one kernel; ENTRIES: the entry words are scanned alongside.  Thread t owns a contiguous piece of the
//             workgroups' counts: it adds them up, the 256 sums are scanned (prefix inside the wave by shuffles, the four waves' totals
//             through LDS), and the thread walks its piece again writing to every workgroup the slot (and the entry offset) of its first
//             held-out point: the running totals in device memory + what lies in front.  Then the running totals are advanced.  The next
//             range's scan -- of this call or of a later upload -- runs behind this one on the stream and starts from them: ranges and
//             uploads chain with no host synchronisation.
//   gather, rows (NIW, the Float32 and byte stores): a workgroup per 256 points; one with no held-out point, or whose first slot lies at or
//             beyond cap, leaves at once.  A thread ranks its point from the four ballot words (ho_rank) and puts its local id into LDS at
//             that rank; then wave w copies the rows of ranks w, w + 4, ..: lanes along the features, coalesced reads and writes, bytes
//             widened on the way, the row id clamped to the range; lane 0 writes the global index.  Slots at or beyond cap are not written.
//   gather, sparse store: a workgroup whose first slot or entry offset lies beyond its cap leaves at once -- a point in front of it did not
//             fit.  Else the held-out points' (id, source offset, length) go to LDS at their rank, the lengths are scanned there (256 values:
//             shuffles inside the wave, the waves' totals through LDS), and the workgroup's points that FIT are counted: rank r fits when
//             slot + r + 1 <= cap and offset + (entries up to and including r) <= entry_cap, a monotone condition.  The one workgroup of
//             the whole call sequence that starts inside both caps and has a point that does not fit writes `stored` and `stored_entries`:
//             every workgroup behind it starts beyond a cap.  The colptr slots and indices of the fitting points are written, and their
//             entries are copied as ONE flat range: output entry e finds its column by bisection in the LDS prefix, so writes are
//             coalesced and the work is balanced whatever the column lengths.  uint16 rows widen to int32; offsets are 64-bit.
// The slot of a held-out point is (held-out points in front of it in the call sequence), its entry offset (their entries): functions of the
// points, the model and the floors alone: the class of a point does not depend on its neighbours, and integer sums have no order.
#include <algorithm>
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"
#include "batchstats_device.h"
#include "countstats_device.h"

namespace dpmm {

constexpr int HO_WAVES = HOLDOUT_THREADS / 64;

// inclusive prefix sum over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T ho_wave_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// the rank of this thread's point among the workgroup's held-out ones, or -1: popcounts of the ballot words in front, of the bits below its own
__device__ __forceinline__ int ho_rank(const unsigned long long *bw, int w, int lane) {
    int rank = 0;
    unsigned long long own = 0;
#pragma unroll
    for (int u = 0; u < HO_WAVES; ++u) {
        const unsigned long long word = bw[u];
        rank += u < w ? __popcll(word) : 0;
        own = u == w ? word : own;
    }
    return ((own >> lane) & 1ull) ? rank + __popcll(own & ((1ull << lane) - 1ull)) : -1;
}

// the end of a class kernel: the wave's ballot of held-out points and the workgroup's counts of the four classes.  Holds a barrier: what a
// kernel put into LDS in front of the call (the count kernel's entry words) is visible behind it.
__device__ __forceinline__ void ho_publish_class(const HoldoutCompact &C, unsigned (*wc)[HOLDOUT_STATE], bool held, bool skipped, bool incomplete, bool part, int tid) {
    const int lane = tid & 63, w = tid >> 6;
    const unsigned long long hm = __ballot(held), sm = __ballot(skipped), im = __ballot(incomplete), pm = __ballot(part);
    if (lane == 0) {
        C.ballot[(int64_t)blockIdx.x * HO_WAVES + w] = hm;
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
        C.wgcount[(int64_t)blockIdx.x * HOLDOUT_STATE + tid] = v;
    }
}

__global__ __launch_bounds__(HOLDOUT_THREADS) void holdout_class_kernel(HoldoutArgs A) {
    __shared__ unsigned gap[HOLDOUT_THREADS];
    __shared__ unsigned wc[HO_WAVES][HOLDOUT_STATE];
    const int K = A.K, D = A.D, tid = threadIdx.x;
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
    ho_publish_class(A, wc, held, valid && !scored, incomplete, part, tid);
}

__global__ __launch_bounds__(HOLDOUT_THREADS) void countholdout_class_kernel(CountHoldoutArgs A) {
    __shared__ unsigned gap[HOLDOUT_THREADS];
    __shared__ unsigned wc[HO_WAVES][HOLDOUT_STATE];
    __shared__ unsigned long long we[HO_WAVES];
    const int K = A.K, D = A.D, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t rs = (int64_t)A.rstep * A.stride;
    const int64_t base = (int64_t)blockIdx.x * HOLDOUT_THREADS;      // (< A.n: the grid is holdout_groups(A.n))
    gap[tid] = 0;
    __syncthreads();
    const int rows = (int)(A.n - base < HOLDOUT_THREADS ? A.n - base : HOLDOUT_THREADS);
    const bool sparse = A.store == COUNTSTATS_SPARSE;
    cs_mark_gaps(gap, A.store, A.store == COUNTSTATS_F32 ? A.X + base * A.ldx : nullptr, (int)A.ldx, sparse ? A.cp + base : nullptr, A.val, rows, D, tid,
                 HOLDOUT_THREADS);
    const int64_t i = base + tid;
    const bool valid = i < A.n;
    const float *col = A.table + (valid ? i : 0);      // (lanes past the end read point 0 and contribute nothing)
    float m, s;
    int best;
    bool nan_seen;
    bs_table_passes(col, rs, K, m, best, nan_seen, s);
    __syncthreads();
    bool scored, held, incomplete, part;
    cs_class(valid, nan_seen, m, s, gap[tid], A.use_floor, A.min_logdens, A.use_pc, A.min_pc, A.tot, i, scored, held, incomplete, part);
    unsigned long long ent = (sparse && held) ? (unsigned long long)(A.cp[i + 1] - A.cp[i]) : 0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ent += __shfl_xor(ent, o);      // (integers: the order does not matter)
    if (lane == 0) we[w] = ent;
    ho_publish_class(A, wc, held, valid && !scored, incomplete, part, tid);
    if (tid == HOLDOUT_STATE) {
        unsigned long long v = 0;
#pragma unroll
        for (int u = 0; u < HO_WAVES; ++u) v += we[u];
        A.wgent[blockIdx.x] = v;
    }
}

template <bool ENTRIES>
__global__ __launch_bounds__(HOLDOUT_THREADS) void holdout_scan_kernel(HoldoutCompact C, const unsigned long long *__restrict__ wgent, int64_t *__restrict__ wgeoff) {
    __shared__ unsigned wtot[HO_WAVES][HOLDOUT_STATE];
    __shared__ unsigned long long wetot[HO_WAVES];     // (ENTRIES only)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t ng = (C.n + HOLDOUT_THREADS - 1) / HOLDOUT_THREADS;      // holdout_groups(C.n)
    const int64_t per = (ng + HOLDOUT_THREADS - 1) / HOLDOUT_THREADS;
    const int64_t g0 = (int64_t)tid * per < ng ? (int64_t)tid * per : ng, g1 = g0 + per < ng ? g0 + per : ng;
    const unsigned long long before = C.state[0];      // (rewritten behind the barrier)
    unsigned long long ebefore = 0, esum = 0, eincl = 0;
    if constexpr (ENTRIES) ebefore = C.state[4];
    unsigned sum[HOLDOUT_STATE] = {0, 0, 0, 0};        // (a range holds fewer than 2^31 points)
    for (int64_t g = g0; g < g1; ++g) {
#pragma unroll
        for (int c = 0; c < HOLDOUT_STATE; ++c) sum[c] += C.wgcount[g * HOLDOUT_STATE + c];
        if constexpr (ENTRIES) esum += wgent[g];
    }
    unsigned incl[HOLDOUT_STATE];
#pragma unroll
    for (int c = 0; c < HOLDOUT_STATE; ++c) incl[c] = ho_wave_scan(sum[c], lane);
    if constexpr (ENTRIES) eincl = ho_wave_scan(esum, lane);
    if (lane == 63) {
#pragma unroll
        for (int c = 0; c < HOLDOUT_STATE; ++c) wtot[w][c] = incl[c];
        if constexpr (ENTRIES) wetot[w] = eincl;
    }
    __syncthreads();
    unsigned front = incl[0] - sum[0];                 // held-out points in front of this thread's piece
    unsigned long long efront = eincl - esum;          // ... and their entries
#pragma unroll
    for (int u = 0; u < HO_WAVES; ++u) {
        front += u < w ? wtot[u][0] : 0u;
        if constexpr (ENTRIES) efront += u < w ? wetot[u] : 0ull;
    }
    int64_t slot = (int64_t)before + (int64_t)front;
    [[maybe_unused]] int64_t eoff = (int64_t)(ebefore + efront);
    for (int64_t g = g0; g < g1; ++g) {
        C.wgoff[g] = slot;
        slot += C.wgcount[g * HOLDOUT_STATE];
        if constexpr (ENTRIES) {
            wgeoff[g] = eoff;
            eoff += (int64_t)wgent[g];
        }
    }
    if (tid < HOLDOUT_STATE) {
        unsigned long long v = 0;
#pragma unroll
        for (int u = 0; u < HO_WAVES; ++u) v += wtot[u][tid];
        C.state[tid] += v;                             // (state[0] was read by every thread in front of the barrier)
    }
    if constexpr (ENTRIES) {
        if (tid == HOLDOUT_STATE) {
            unsigned long long v = 0;
#pragma unroll
            for (int u = 0; u < HO_WAVES; ++u) v += wetot[u];
            C.state[4] += v;                           // (as state[0])
        }
    }
}

template <typename T>
__global__ __launch_bounds__(HOLDOUT_THREADS) void holdout_gather_rows_kernel(HoldoutCompact C, const T *__restrict__ X, int64_t ld, int D) {
    __shared__ int ids[HOLDOUT_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int count = (int)C.wgcount[(int64_t)blockIdx.x * HOLDOUT_STATE];
    const int64_t off = C.wgoff[blockIdx.x];
    if (count == 0 || off >= C.cap) return;            // (uniform over the workgroup)
    const int64_t base = (int64_t)blockIdx.x * HOLDOUT_THREADS;
    const int rows = (int)(C.n - base < HOLDOUT_THREADS ? C.n - base : HOLDOUT_THREADS);
    const int rank = ho_rank(C.ballot + (int64_t)blockIdx.x * HO_WAVES, w, lane);
    if (rank >= 0) ids[rank] = tid;                    // (ranks 0 .. count - 1, each once)
    __syncthreads();
    for (int r = w; r < count; r += HO_WAVES) {
        const int64_t slot = off + r;
        if (slot >= C.cap) break;                      // (the slots grow with r)
        const int id = ids[r] < rows ? ids[r] : rows - 1;
        const T *src = X + (base + id) * ld;
        float *dst = C.dst_points + slot * D;
        for (int d = lane; d < D; d += 64) dst[d] = (float)src[d];
        if (lane == 0) C.dst_index[slot] = C.index0 + base + id;
    }
}

__global__ __launch_bounds__(HOLDOUT_THREADS) void countholdout_gather_sparse_kernel(CountHoldoutArgs A) {
    __shared__ int ids[HOLDOUT_THREADS];
    __shared__ int64_t src[HOLDOUT_THREADS];           // source offset of the point of rank r
    __shared__ int pre[HOLDOUT_THREADS + 1];           // entries of the ranks in front of r; [count] = all (a column holds at most 65536: below 2^24)
    __shared__ int wsum[HO_WAVES], wfit[HO_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int count = (int)A.wgcount[(int64_t)blockIdx.x * HOLDOUT_STATE];
    const int64_t off = A.wgoff[blockIdx.x], eoff = A.wgeoff[blockIdx.x];
    if (count == 0 || off > A.cap || eoff > A.entry_cap) return;      // (uniform; beyond a cap: a point in front did not fit)
    const int64_t base = (int64_t)blockIdx.x * HOLDOUT_THREADS;
    const int64_t *cpb = A.cp + base;
    const int rank = ho_rank(A.ballot + (int64_t)blockIdx.x * HO_WAVES, w, lane);
    ids[tid] = 0; src[tid] = 0; pre[tid] = 0;
    __syncthreads();
    if (rank >= 0) {                                   // (a held-out point lies inside the range: base + tid < A.n)
        const int64_t lo = cpb[tid];
        ids[rank] = tid;
        src[rank] = lo;
        pre[rank] = (int)(cpb[tid + 1] - lo);          // its length for now
    }
    __syncthreads();
    const int len = pre[tid];                          // thread r: the length of rank r (0 at and beyond count)
    const int incl = ho_wave_scan(len, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int front = 0;
#pragma unroll
    for (int u = 0; u < HO_WAVES; ++u) front += u < w ? wsum[u] : 0;
    const int mine = front + incl;                     // entries up to and including rank tid
    const bool fits = tid < count && off + tid + 1 <= A.cap && eoff + mine <= A.entry_cap;      // (monotone in tid)
    const unsigned long long fm = __ballot(fits);
    if (lane == 0) wfit[w] = __popcll(fm);
    __syncthreads();                                   // every length has been read
    pre[tid + 1] = mine;                               // (pre[0] stays: thread 0 writes it below)
    if (tid == 0) pre[0] = 0;
    int fit = 0;
#pragma unroll
    for (int u = 0; u < HO_WAVES; ++u) fit += wfit[u];
    __syncthreads();
    if (fit < count && tid == 0) {                     // the boundary workgroup: the only one of the call sequence
        A.state[5] = (unsigned long long)(off + fit);
        A.state[6] = (unsigned long long)(eoff + pre[fit]);
    }
    if (tid < fit) {
        A.dst_colptr[off + tid + 1] = eoff + mine;
        A.dst_index[off + tid] = A.index0 + base + ids[tid];
    }
    const int E = pre[fit];                            // the entries of the fitting points: one flat range of the output
    for (int e = tid; e < E; e += HOLDOUT_THREADS) {
        int lo = 0, hi = fit - 1;                      // the last rank whose entries start at or before e (empty columns in front are passed)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const int64_t q = src[lo] + (e - pre[lo]);
        A.dst_rowval[eoff + e] = (int32_t)A.ri[q];
        A.dst_val[eoff + e] = A.val[q];
    }
}

hipError_t launch_holdout_range(const HoldoutArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.D < 1 || a.D > 256 || a.ldx < a.D || a.ldx > 1024 || a.n >> 31 || a.n > a.stride || a.rstep < 1 || a.cap < 0 ||
        a.index0 < 0 || !a.table || !a.X || !a.ballot || !a.wgcount || !a.wgoff || !a.state || (a.use_tail && !a.tail) ||
        (a.cap > 0 && (!a.dst_points || !a.dst_index)))
        return hipErrorInvalidValue;
    const HoldoutCompact &c = a;
    const dim3 grid((unsigned)holdout_groups(a.n)), block(HOLDOUT_THREADS);
    DPMM_LAUNCH(holdout_class_kernel, grid, block, 0, s, a);
    DPMM_LAUNCH(holdout_scan_kernel<false>, dim3(1), block, 0, s, c, nullptr, nullptr);
    if (a.cap > 0) DPMM_LAUNCH(holdout_gather_rows_kernel<float>, grid, block, 0, s, c, a.X, a.ldx, a.D);
    return hipGetLastError();
}

hipError_t launch_countholdout_range(const CountHoldoutArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    const bool sparse = a.store == COUNTSTATS_SPARSE;
    if (a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.D < 1 || a.D > (1 << 20) || a.n >> 31 || a.n > a.stride || a.rstep < 1 || a.cap < 0 || a.entry_cap < 0 ||
        a.index0 < 0 || !a.table || !a.ballot || !a.wgcount || !a.wgent || !a.wgoff || !a.wgeoff || !a.state || (a.use_pc && !a.tot))
        return hipErrorInvalidValue;
    if (a.store == COUNTSTATS_F32) { if (!a.X || a.ldx < a.D || a.ldx > (1 << 22)) return hipErrorInvalidValue; }
    else if (a.store == COUNTSTATS_U8) { if (!a.X8 || a.ld8 < a.D) return hipErrorInvalidValue; }
    else if (sparse) { if (!a.cp || a.D > 65536) return hipErrorInvalidValue; }
    else return hipErrorInvalidValue;
    if (a.cap > 0 && !a.dst_index) return hipErrorInvalidValue;
    if (a.cap > 0 && !sparse && !a.dst_points) return hipErrorInvalidValue;
    if (a.cap > 0 && sparse && (!a.dst_colptr || (a.entry_cap > 0 && (!a.dst_rowval || !a.dst_val || !a.ri || !a.val)))) return hipErrorInvalidValue;
    const HoldoutCompact &c = a;
    const dim3 grid((unsigned)holdout_groups(a.n)), block(HOLDOUT_THREADS);
    DPMM_LAUNCH(countholdout_class_kernel, grid, block, 0, s, a);
    DPMM_LAUNCH(holdout_scan_kernel<true>, dim3(1), block, 0, s, c, a.wgent, a.wgeoff);
    if (a.cap > 0) {
        if (sparse) DPMM_LAUNCH(countholdout_gather_sparse_kernel, grid, block, 0, s, a);
        else if (a.store == COUNTSTATS_U8) DPMM_LAUNCH(holdout_gather_rows_kernel<uint8_t>, grid, block, 0, s, c, a.X8, a.ld8, a.D);
        else DPMM_LAUNCH(holdout_gather_rows_kernel<float>, grid, block, 0, s, c, a.X, a.ldx, a.D);
    }
    return hipGetLastError();
}

}  // namespace dpmm
