// recommend.hip -- top-m next-count probabilities of the Multinomial prior (include/dpmm_hip_recommend.h): from a range of the table a_k(i)
// that the sweep kernels' table mode wrote (table[k * rstep * stride + i]), the range's points in whichever of the three count stores is
// live, and the Float32 image theta[k][d] of dpmm_set_recommend to the m unseen features of largest r_id = sum_k p_ik theta_kd per point.
//
// A workgroup of four waves owns RC_PTS = 32 points of the range:
//   row      lane l walks the table row of point p = l & 31 (all eight lanes of a point: the same statements on the same words) with the
//            functions of score_device.h: M, the label, S;
//   probs    p_ik = e_k / S -- the bits `probs` holds -- into LDS, ps[k * 32 + p], K padded to even with a row of zeros; a point that takes
//            no part has zeros throughout.  The (n, K) matrix exists nowhere else;
//   pairs    the cluster pairs (2q, 2q + 1) with a p that is not 0 for some point of the tile, in increasing q: the others are left out, their
//            terms are exact zeros (a Float32 expf underflows to exactly 0 for far clusters);
//   blocks   wave w takes the 32-feature blocks w, w + 4, ...  A block is one chain of v_mfma_f32_32x32x2_f32 from 0 over the pairs that
//            stay: A operand theta (lane l: theta[2q + (l >> 5)][f0 + (l & 31)], 128-byte lines of the padded image), B operand the
//            probabilities (ps[(2q + (l >> 5)) * 32 + (l & 31)]: 64 consecutive words).  Lane l then holds the scores of point l & 31 for the
//            16 features f0 + 8 (r >> 2) + 4 (l >> 5) + (r & 3);
//   seen     a 32-bit mask of the block per point: dense stores from the words of X the lane's 16 features occupy (each word of X is read
//            once), sparse store from a cursor into the point's entries -- rows are strictly increasing inside a column (both upload paths
//            refuse anything else, csc_io.hip and mult_sparse.hip) -- that every wave advances over the blocks it does not own;
//   select   a lane keeps the m best keys it has met in MT registers (score.hip's unrolled chain of selects; MT = 4 or 16 >= m) and a
//            threshold: the larger of its own m-th key and that of the other lane of its point in the wave.  A key at or below the m-th
//            key of ANY list of the point can never enter the point's first m, so dropping it changes nothing.  The wave leaves the fast
//            path only when a score of some lane beats that lane's threshold;
//   merge    the eight lists of a point meet in LDS (over the probabilities, which are dead by then); lane p of wave 0 selects the m
//            largest keys of point p -- a selection by a total order: the result does not depend on the order the keys arrive in.
// A key is one 64-bit word, (bits(r) + 1) << 32 | ~feature, r >= 0: as unsigned integers the keys order like (r descending, feature
// ascending); 0 is the empty slot.  One writer per output word, no atomics; the points that take no part are counted per tile in a word only
// this workgroup writes (the host adds the words up).
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"

namespace dpmm {

typedef float rc_f32x16 __attribute__((ext_vector_type(16)));

constexpr int RC_PTS = 32;               // points per workgroup
constexpr int RC_WAVES = 4;              // waves per workgroup: every fourth block of 32 features each
constexpr int RC_LISTS = 2 * RC_WAVES;   // lists per point: one per lane that holds scores of the point
constexpr unsigned long long RC_FULL = ~0ull;      // a slot that takes no key (a real key's upper word is at most 0x7f800001)

// the carried key moves in where it ranks higher; the displaced one is carried on
template <int MT>
__device__ __forceinline__ void rc_insert(unsigned long long (&tk)[MT], unsigned long long key) {
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const unsigned long long t = tk[j];
        tk[j] = key > t ? key : t;
        key = key > t ? t : key;
    }
}

template <int MT, int STORE>
__global__ __launch_bounds__(64 * RC_WAVES) void recommend_kernel(RecommendArgs A) {
    extern __shared__ unsigned long long rc_smem[];                 // the probabilities, then the lists
    __shared__ uint16_t act[DPMM_MAX_CLUSTERS_K / 2];
    __shared__ int nact;
    float *const ps = reinterpret_cast<float *>(rc_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pt = lane & 31, half = lane >> 5;
    const int K = A.K, Kp = A.Kp, D = A.D, mm = A.m;
    const int64_t i0 = (int64_t)blockIdx.x * RC_PTS;
    const int npt = A.n - i0 < RC_PTS ? (int)(A.n - i0) : RC_PTS;
    const int64_t i = i0 + pt;
    const bool valid = pt < npt;
    // ---- the point's row of the table: M, label, S (score_device.h)
    const float *col = A.table + (valid ? i : 0);                   // (lanes past the end read point 0 and write nothing)
    const int64_t rs = (int64_t)A.rstep * A.stride;
    float m = -INFINITY;
    int best = 0;
    bool nan_seen = false;
    for (int k = 0; k < K; ++k) score_max_step(col[(int64_t)k * rs], k, m, best, nan_seen);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += score_e(col[(int64_t)k * rs], m);
    const bool part = valid && !nan_seen && m > -INFINITY && m < INFINITY;
    if (wave == 0) {
        if (valid && half == 0 && A.labels) A.labels[i] = best + 1;
        const unsigned long long sm = __ballot(valid && half == 0 && !part);
        if (lane == 0) A.skip[blockIdx.x] += (unsigned)__popcll(sm);      // (this word has no other writer; launches of a stream are ordered)
    }
    // ---- the probabilities: row k by the lanes of half k & 1 of wave (k >> 1) & 3
    for (int k = 2 * wave + half; k < Kp; k += 2 * RC_WAVES)
        ps[k * RC_PTS + pt] = (part && k < K) ? score_p(score_e(col[(int64_t)k * rs], m), s) : 0.f;
    __syncthreads();
    // ---- the pairs that stay, in increasing order (lane l looks at pair base + l: 64 words, walked from word l on so that the lanes meet in no bank)
    if (wave == 0) {
        const unsigned long long below = (1ull << lane) - 1ull;
        int cnt = 0;
        for (int base = 0; base < Kp / 2; base += 64) {
            const int q = base + lane;
            bool any = false;
            if (q < Kp / 2)
                for (int w = 0; w < 64; ++w) any = any || ps[q * 64 + ((w + lane) & 63)] != 0.f;
            const unsigned long long mask = __ballot(any);
            if (any) act[cnt + __popcll(mask & below)] = (uint16_t)q;
            cnt += __popcll(mask);
        }
        if (lane == 0) nact = cnt;
    }
    __syncthreads();
    const int na = nact;
    // ---- the blocks of this wave
    // (the first MT - m slots hold a key above every real one for good: slot MT - 1 is the lane's m-th key, at an index the compiler knows --
    // tk[m - 1] would put the list into scratch memory)
    unsigned long long tk[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) tk[j] = j < MT - mm ? RC_FULL : 0ull;
    unsigned long long thr = 0ull;
    int64_t cur = 0, cend = 0;                                      // sparse store: the entries of the point that are still ahead
    if (STORE == COUNTSTATS_SPARSE && valid) { cur = A.cp[i]; cend = A.cp[i + 1]; }
    const int nblk = (D + 31) / 32;
    const float *const pp = ps + half * RC_PTS + pt;
#pragma unroll 1
    for (int fb = wave; fb < nblk; fb += RC_WAVES) {
        const int f0 = fb * 32;
        rc_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float *const th = A.theta + (int64_t)half * A.Dp + f0 + pt;
        int j = 0;
        for (; j + 4 <= na; j += 4) {                               // four steps at a time: the loads of all four in front of the first product
            const int q0 = act[j], q1 = act[j + 1], q2 = act[j + 2], q3 = act[j + 3];
            const float a0 = th[(int64_t)(2 * q0) * A.Dp], a1 = th[(int64_t)(2 * q1) * A.Dp], a2 = th[(int64_t)(2 * q2) * A.Dp], a3 = th[(int64_t)(2 * q3) * A.Dp];
            const float b0 = pp[q0 * 64], b1 = pp[q1 * 64], b2 = pp[q2 * 64], b3 = pp[q3 * 64];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b3, acc, 0, 0, 0);
        }
        for (; j < na; ++j) {
            const int q = act[j];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(th[(int64_t)(2 * q) * A.Dp], pp[q * 64], acc, 0, 0, 0);
        }
        // ---- the features of the block the point has seen: bit 8 g + j of `seen` is feature f0 + 8 g + 4 half + j (j < 4)
        unsigned seen = 0u;
        if (STORE == COUNTSTATS_F32) {
            if (valid) {
                const float *row = A.X + i * A.ldx + f0 + 4 * half;  // (ldx is a multiple of 4 and the rows are 16-byte aligned: a group of four lies inside the row or behind it)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if (f0 + 4 * half + 8 * g < A.ldx) {
                        const float4 x = *reinterpret_cast<const float4 *>(row + 8 * g);
                        seen |= (unsigned)(x.x != 0.f) << (8 * g) | (unsigned)(x.y != 0.f) << (8 * g + 1) | (unsigned)(x.z != 0.f) << (8 * g + 2) |
                                (unsigned)(x.w != 0.f) << (8 * g + 3);
                    }
                }
            }
        } else if (STORE == COUNTSTATS_U8) {
            if (valid) {
                const uint8_t *row = A.X8 + i * A.ld8 + f0 + 4 * half;   // (ld8 is a multiple of 128: the block lies inside the row)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const uint32_t x = *reinterpret_cast<const uint32_t *>(row + 8 * g);
                    seen |= (unsigned)((x & 0xffu) != 0u) << (8 * g) | (unsigned)((x & 0xff00u) != 0u) << (8 * g + 1) |
                            (unsigned)((x & 0xff0000u) != 0u) << (8 * g + 2) | (unsigned)((x & 0xff000000u) != 0u) << (8 * g + 3);
                }
            }
        } else {
            while (cur < cend && (int)A.ri[cur] < f0) ++cur;
            unsigned bm = 0u;
            while (cur < cend) {
                const int r = (int)A.ri[cur] - f0;
                if (r >= 32) break;
                if (A.val[cur] != 0.f) bm |= 1u << r;
                ++cur;
            }
            seen = bm >> (4 * half);
        }
        if (!A.exclude) seen = 0u;
        // ---- the keys of the lane's 16 scores; the slow path only if one of them, in some lane, beats its lane's threshold
        unsigned long long key[16];
        unsigned long long kmax = 0ull;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int f = f0 + 8 * (r >> 2) + 4 * half + (r & 3);
            const float v = acc[r];
            const bool ok = part && f < D && !((seen >> (8 * (r >> 2) + (r & 3))) & 1u) && v == v;
            key[r] = ok ? (((unsigned long long)(__float_as_uint(v) + 1u) << 32) | (unsigned long long)(~(unsigned)f)) : 0ull;
            kmax = key[r] > kmax ? key[r] : kmax;
        }
        if (__ballot(kmax > thr) == 0) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (__ballot(key[r] > thr) == 0) continue;
            rc_insert<MT>(tk, key[r]);                              // (a key at or below the lane's last one falls through the chain)
            const unsigned long long own = tk[MT - 1];
            const unsigned long long other = __shfl_xor(own, 32);
            thr = own > other ? own : other;
        }
    }
    // ---- the eight lists of a point side by side, over the probabilities
    __syncthreads();
    unsigned long long *const lists = rc_smem;
#pragma unroll
    for (int j = 0; j < MT; ++j) lists[(pt * RC_LISTS + 2 * wave + half) * MT + j] = tk[j];
    __syncthreads();
    if (wave != 0 || half != 0 || !valid) return;
    unsigned long long fk[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) fk[j] = 0ull;
    constexpr int PER = RC_LISTS * MT;                              // keys of a point; lane p starts at key p, so that the lanes meet in no bank
    const unsigned long long *const mine = lists + pt * PER;
#pragma unroll 1
    for (int q = 0; q < PER; ++q) {
        const unsigned long long k2 = mine[(q + pt) & (PER - 1)];
        if (k2 != RC_FULL && k2 > fk[MT - 1]) rc_insert<MT>(fk, k2);
    }
    int32_t *const fo = A.features + i * A.ld;
    float *const po = A.prob + i * A.ld;
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        if (j < mm) {
            const unsigned long long k2 = fk[j];
            fo[j] = k2 ? (int32_t)(~(unsigned)k2) : -1;
            po[j] = k2 ? __uint_as_float((unsigned)(k2 >> 32) - 1u) : __uint_as_float(0x7fc00000u);
        }
    }
    for (int64_t j = mm; j < A.ld; ++j) { fo[j] = 0; po[j] = 0.f; }  // the padding columns [m, ld)
}

template <int MT, int STORE>
static hipError_t launch_rc(const RecommendArgs &a, unsigned tiles, hipStream_t s) {
    const size_t probs = sizeof(float) * (size_t)a.Kp * RC_PTS, lists = sizeof(unsigned long long) * RC_PTS * RC_LISTS * MT;
    const size_t lds = probs > lists ? probs : lists;
    static bool attr = false;
    if (!attr) {
        hipError_t e = hipFuncSetAttribute((const void *)recommend_kernel<MT, STORE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(sizeof(float) * DPMM_MAX_CLUSTERS_K * RC_PTS));
        if (e != hipSuccess) return e;
        attr = true;
    }
    DPMM_LAUNCH((recommend_kernel<MT, STORE>), dim3(tiles), dim3(64 * RC_WAVES), lds, s, a);
    return hipGetLastError();
}

template <int STORE>
static hipError_t launch_rc_store(const RecommendArgs &a, unsigned tiles, hipStream_t s) {
    return a.m <= 4 ? launch_rc<4, STORE>(a, tiles, s) : launch_rc<16, STORE>(a, tiles, s);
}

hipError_t launch_recommend_range(const RecommendArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.Kp != a.K + (a.K & 1) || a.D < 1 || a.Dp % 32 || a.Dp < a.D || a.m < 1 || a.m > RECOMMEND_MAX_TOP || a.m > a.D ||
        a.ld < a.m)
        return hipErrorInvalidValue;
    if (a.store == COUNTSTATS_SPARSE ? (!a.cp || a.D > 65536) : a.store == COUNTSTATS_U8 ? (!a.X8 || a.ld8 % 4 || a.ld8 < 32 * (int64_t)((a.D + 31) / 32)) : (!a.X || a.ldx % 4))
        return hipErrorInvalidValue;
    const int64_t tiles = (a.n + RC_PTS - 1) / RC_PTS;
    if (tiles >> 31) return hipErrorInvalidValue;
    if (a.store == COUNTSTATS_SPARSE) return launch_rc_store<COUNTSTATS_SPARSE>(a, (unsigned)tiles, s);
    if (a.store == COUNTSTATS_U8) return launch_rc_store<COUNTSTATS_U8>(a, (unsigned)tiles, s);
    return launch_rc_store<COUNTSTATS_F32>(a, (unsigned)tiles, s);
}

}  // namespace dpmm
