// rank.hip -- exemplars (include/dpmm_hip_rank.h): per cluster the m best and the m worst points by the score s_i = max_k a_k(i), selected
// from the slab of the table a_k(i) that the sweep kernels' table mode wrote (table[k * rstep * stride + i], as score.hip reads it).
//
// A key is one 64-bit word, ord(s) << 32 | ~index (typical list) or ~ord(s) << 32 | ~index (fringe list), ord the usual monotone map of
// a finite Float32 to an unsigned integer: as unsigned integers the keys order like (s descending, index ascending) and (s ascending,
// index ascending), BOTH lists are "the m largest keys, largest first", and 0 -- below every real key, whose upper word is at least
// 0x00800000 -- is the empty slot.  The running list of a (list, cluster) is 64 sorted keys in global memory, one per lane of a wave.
//
// Two launches per chunk of at most RANK_CHUNK points, nothing in them waits for another workgroup:
//   filter   one thread per point, lanes along i (every read of table[k][i .. i + 63] is one coalesced 256-byte line): pass 1 of
//            score_finish_kernel -- maximum, label, NaN seen -- then the point's two keys against the m-th key of its cluster's lists
//            (the thresholds of all K clusters sit in LDS, read once per workgroup; a lane reads word 2 (w K + label), two lanes of a
//            half-wave meet in a bank only with different labels).  A survivor goes to the candidate buffer of its list: one atomic
//            add per wave and list reserves the wave's range, the lanes write behind it in lane order.  WHERE a candidate lands depends
//            on the order of those adds, WHAT the buffer holds does not, and the merge below is a selection by a total order: the
//            result depends on neither.  The per-cluster counts are integer adds in LDS (one per wave where the wave's points share a
//            label), flushed to one of RANK_REPL replicas of the global counters: sums of integers, order-free.
//   merge    one wave per (cluster, list): it walks the candidate buffer 64 entries at a time, keeps those of its cluster that still
//            beat its m-th key, compacts them through 128 words of LDS and, 64 at a time, sorts them (bitonic, in registers: 21
//            compare-exchange steps of __shfl_xor on the 64-bit key) and merges them with its list: max(list[j], batch[63 - j]) holds
//            the 64 largest of the 128 as a bitonic sequence, six more steps sort it.
// The thresholds only move up, and a key at or below a threshold can never enter the first m: dropping it early changes nothing.
// A chunk has at most RANK_CHUNK candidates per list (a point is one at most), so the buffer cannot overflow; writes are bounded anyway.
#include "dpmm_device.h"
#include "dpmm_kernels.h"

namespace dpmm {

constexpr int RF_THREADS = 256;

__device__ __forceinline__ unsigned rank_ord(float s) {      // finite s: a < b  <=>  ord(a) < ord(b)  (-0.0 below +0.0)
    const unsigned u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(RF_THREADS) void rank_filter_kernel(RankArgs A) {
    __shared__ unsigned long long thr[2 * DPMM_MAX_CLUSTERS_K];
    __shared__ unsigned cnt[DPMM_MAX_CLUSTERS_K];
    __shared__ unsigned skipped;
    const int K = A.K, tid = threadIdx.x, lane = tid & 63;
    for (int k = tid; k < K; k += RF_THREADS) {
        thr[k] = A.keys[(int64_t)k * RANK_SLOTS + A.m - 1];
        thr[K + k] = A.keys[(int64_t)(K + k) * RANK_SLOTS + A.m - 1];
        cnt[k] = 0;
    }
    if (tid == 0) skipped = 0;
    if (blockIdx.x == 0 && tid < 2) A.cand_n[(A.parity ^ 1) * 2 + tid] = 0;      // the next chunk's counters: nobody reads them before the next launch
    __syncthreads();
    const int64_t rs = (int64_t)A.rstep * A.stride;
    const unsigned long long below = (1ull << lane) - 1ull;
    // (the trip count is the same for every thread of the workgroup: the ballots below see whole waves)
    for (int64_t base = (int64_t)blockIdx.x * RF_THREADS; base < A.n; base += (int64_t)gridDim.x * RF_THREADS) {
        const int64_t i = base + tid;
        const bool valid = i < A.n;
        const float *col = A.table + (valid ? i : 0);      // (lanes past the end read point 0 and contribute nothing)
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
        const bool part = valid && !nan_seen && m > -INFINITY && m < INFINITY;
        // ---- count and skipped
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
        // ---- candidates
        const unsigned o = rank_ord(m);
        const unsigned long long low = (unsigned long long)(~(unsigned)(A.index0 + i));
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            if (!(A.which & (1 << w))) continue;
            const unsigned long long key = ((unsigned long long)(w ? ~o : o) << 32) | low;
            const bool pass = part && key > thr[w * K + best];
            const unsigned long long mask = __ballot(pass);
            if (!mask) continue;
            const int leader = __ffsll((long long)mask) - 1;
            unsigned at = 0;
            if (lane == leader) at = atomicAdd(&A.cand_n[A.parity * 2 + w], (unsigned)__popcll(mask));
            at = __shfl(at, leader);
            const int64_t pos = (int64_t)at + __popcll(mask & below);
            if (pass && pos < A.cap) {
                A.cand_key[w * A.cap + pos] = key;
                A.cand_k[w * A.cap + pos] = (uint16_t)best;
            }
        }
    }
    __syncthreads();
    unsigned long long *count = A.count + (int64_t)(blockIdx.x % RANK_REPL) * (K + 1);
    for (int k = tid; k < K; k += RF_THREADS)
        if (cnt[k]) atomicAdd(&count[k], (unsigned long long)cnt[k]);
    if (tid == 0 && skipped) atomicAdd(&count[K], (unsigned long long)skipped);
}

__device__ __forceinline__ unsigned long long rank_cx(unsigned long long v, int j, bool keep_max) {
    const unsigned long long p = __shfl_xor(v, j);
    const unsigned long long hi = v > p ? v : p, lo = v > p ? p : v;
    return keep_max ? hi : lo;
}

// 64 keys, one per lane, sorted so that lane 0 holds the largest
__device__ __forceinline__ unsigned long long rank_sort64(unsigned long long v, int lane) {
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) v = rank_cx(v, j, ((lane & j) == 0) == ((lane & k) == 0));
    return v;
}

// list and batch sorted (largest in lane 0): the 64 largest of both, sorted
__device__ __forceinline__ unsigned long long rank_merge64(unsigned long long list, unsigned long long batch, int lane) {
    const unsigned long long r = __shfl(batch, 63 - lane);
    unsigned long long v = list > r ? list : r;
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) v = rank_cx(v, j, (lane & j) == 0);
    return v;
}

__global__ __launch_bounds__(64) void rank_merge_kernel(RankArgs A) {
    __shared__ unsigned long long buf[128];
    const int k = blockIdx.x, w = blockIdx.y, lane = threadIdx.x;
    if (!(A.which & (1 << w))) return;
    int64_t cn = A.cand_n[A.parity * 2 + w];
    if (cn > A.cap) cn = A.cap;
    if (cn == 0) return;
    unsigned long long *list = A.keys + (int64_t)(w * A.K + k) * RANK_SLOTS;
    const unsigned long long *ckey = A.cand_key + w * A.cap;
    const uint16_t *ck = A.cand_k + w * A.cap;
    unsigned long long L = list[lane];
    const unsigned long long below = (1ull << lane) - 1ull;
    int pend = 0;      // keys waiting in buf; every value below is the same in all lanes (one wave, whole-wave ballots)
    bool changed = false;
    for (int64_t base = 0; base < cn; base += 64) {
        const unsigned long long t = __shfl(L, A.m - 1);
        const int64_t j = base + lane;
        unsigned long long key = 0;
        if (j < cn && ck[j] == (uint16_t)k) key = ckey[j];
        const bool mine = key > t;      // (t >= 0: a lane without a candidate holds key 0 and never passes)
        const unsigned long long mask = __ballot(mine);
        if (!mask) continue;
        if (mine) buf[pend + __popcll(mask & below)] = key;
        pend += __popcll(mask);
        __syncthreads();
        if (pend >= 64) {
            const unsigned long long B = buf[lane];
            const unsigned long long rest = buf[64 + lane];
            __syncthreads();
            pend -= 64;
            if (lane < pend) buf[lane] = rest;
            __syncthreads();
            L = rank_merge64(L, rank_sort64(B, lane), lane);
            changed = true;
        }
    }
    if (pend) {
        const unsigned long long B = lane < pend ? buf[lane] : 0ull;
        L = rank_merge64(L, rank_sort64(B, lane), lane);
        changed = true;
    }
    if (changed) list[lane] = L;
}

hipError_t launch_rank_chunk(const RankArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.n > a.cap || a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.m < 1 || a.m > RANK_SLOTS || !(a.which & 3)) return hipErrorInvalidValue;
    int64_t g = (a.n + RF_THREADS - 1) / RF_THREADS;
    if (g > 1024) g = 1024;
    DPMM_LAUNCH(rank_filter_kernel, dim3((int)g), dim3(RF_THREADS), 0, s, a);
    DPMM_LAUNCH(rank_merge_kernel, dim3(a.K, 2), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ---- the lists as the caller reads them
__global__ __launch_bounds__(256) void rank_read_kernel(const unsigned long long *keys, const unsigned long long *count, int K, int m, int which,
                                                        RankOut o) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < K * m) {
        const int k = t / m, j = t - k * m;
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            int64_t *idx = w ? o.fringe_idx : o.typ_idx;
            float *sc = w ? o.fringe_score : o.typ_score;
            const unsigned long long key = (which & (1 << w)) ? keys[(int64_t)(w * K + k) * RANK_SLOTS + j] : 0ull;
            const unsigned h = w ? ~(unsigned)(key >> 32) : (unsigned)(key >> 32);
            const unsigned u = (h & 0x80000000u) ? (h & 0x7fffffffu) : ~h;      // ord's inverse
            if (idx) idx[t] = key ? (int64_t)(~(unsigned)key) : -1;
            if (sc) sc[t] = key ? __uint_as_float(u) : __uint_as_float(0x7fc00000u);
        }
    }
    if (t <= K) {
        unsigned long long v = 0;
        for (int r = 0; r < RANK_REPL; ++r) v += count[(int64_t)r * (K + 1) + t];
        if (t < K) { if (o.count) o.count[t] = (int64_t)v; }
        else if (o.skipped) o.skipped[0] = (int64_t)v;
    }
}

hipError_t launch_rank_read(const unsigned long long *keys, const unsigned long long *count, int K, int m, int which, const RankOut &o, hipStream_t s) {
    const int work = K * m > K + 1 ? K * m : K + 1;
    DPMM_LAUNCH(rank_read_kernel, dim3((work + 255) / 256), dim3(256), 0, s, keys, count, K, m, which, o);
    return hipGetLastError();
}

}  // namespace dpmm
