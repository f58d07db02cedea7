// count_explain.hip -- the top-m surprising features of a count point (include/dpmm_hip_count_explain.h): from a range of the table a_k(i)
// that the sweep kernels' table mode wrote (table[k * rstep * stride + i]), the range's points in whichever of the three count stores is
// live, and the Float64 tables log theta, log1p(-theta) and `order` of dpmm_set_count_explain to, per point, the `top` features of largest
// |residual| under Binomial(t, theta_kd), k the point's label, with their counts, expectations, residuals and exact binomial tails.
//
// A wave owns COUNT_EXPLAIN_TILE = 32 consecutive points and shares nothing with the other waves of its workgroup (no LDS, no barrier):
//   rows     lane l walks the table row of point l & 31 over the clusters of parity l >> 5: one 64-bit key per entry, ordered like Julia's
//            argmax (the first NaN wins, else the first maximum; -0 counts as +0), the two halves meet by one exchange.  The key holds the
//            label and the class of the row (a NaN or no finite entry: skipped -- the rule of dpmm_hip_rank.h);
//   then point by point, the 64 lanes on one point:
//   total    t, cs_wave_total of countstats_device.h over the store's values, and with it the scan for a value that is not finite or
//            negative.  Such a point, or one with t = 0, is incomplete;
//   scores   dense stores: lanes along the features; sparse store: lanes along the point's entries, then the features it does NOT hold from
//            the head of order[k] (their |residual| cannot increase along it, l1m being non-decreasing), 64 positions at a time, each lane
//            bisecting the point's sorted entries, until `top` kept candidates rank strictly above the next position's |residual| as Float32:
//            two features whose theta differ by an ulp round to one residual and the lower index, later in the list, must still come
//            first.  A candidate is one 64-bit key, (bits(|residual|) + 1) << 32 | ~feature: as unsigned integers the keys order like
//            (|residual| descending, feature ascending); 0 is the empty slot.  A lane keeps the MT >= top best keys it has met in
//            registers, sorted, behind its last one as a threshold (the chain of selects of recommend.hip);
//   merge    `top` rounds of a 64-bit wave maximum over the lanes' heads; the lane that held the winner drops it.  A selection by a total
//            order: the result is unique;
//   winners  lane j < top writes winner j: the feature and |residual|, the bits that ranked it;
//   finish   a second kernel, one lane per slot, reads the winner's count from the store and writes it, t theta, the signed residual and
//            the binomial tail (count_explain_math.h), the padding columns, the labels and the totals: the exponentials and the incomplete
//            beta function stay out of the selection, which works on logarithms alone (explain.hip splits its kernels the same way).
// One writer per output word, no atomics; skipped and incomplete points are counted per wave in words only this wave writes.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "countstats_device.h"
#include "count_explain_math.h"

namespace dpmm {

constexpr int CE_WAVES = 4;              // waves per workgroup (independent of each other)
constexpr int CE_PTS = COUNT_EXPLAIN_TILE;

__device__ __forceinline__ unsigned long long ce_wave_max(unsigned long long v) {      // (exp_wave_max of explain.hip)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}

// entry k of a table row as a key: NaN above everything, else the value's bits in an order-preserving form; ties to the lower k
__device__ __forceinline__ unsigned long long ce_row_key(float a, int k) {
    unsigned hi = 0xffffffffu;
    if (a == a) {
        const unsigned b = __float_as_uint(a + 0.f);      // (-0 + 0 = +0)
        hi = b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
    }
    return ((unsigned long long)hi << 32) | (unsigned long long)(~(unsigned)k);
}
constexpr unsigned CE_ROW_NAN = 0xffffffffu, CE_ROW_PINF = 0xff800000u, CE_ROW_NINF = 0x007fffffu;

// the carried key moves in where it ranks higher; the displaced one is carried on (rc_insert of recommend.hip)
template <int MT>
__device__ __forceinline__ void ce_insert(unsigned long long (&tk)[MT], unsigned long long key) {
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const unsigned long long t = tk[j];
        tk[j] = key > t ? key : t;
        key = key > t ? t : key;
    }
}

// the key of feature d with value x (0: no candidate on this side)
__device__ __forceinline__ unsigned long long ce_key(double x, double t, double lt, double lth, double l1m, int d, int want) {
    int side;
    const float r = ce_score(x, t, lt, lth, l1m, &side);
    const bool cand = want == COUNT_EXPLAIN_BOTH || (want == COUNT_EXPLAIN_OVER ? side > 0 : side < 0);
    return cand ? (((unsigned long long)(__float_as_uint(r) + 1u) << 32) | (unsigned long long)(~(unsigned)d)) : 0ull;
}

// the first entry of [lo, hi) whose row is not below d (rows are strictly increasing inside a column)
__device__ __forceinline__ int64_t ce_find(const uint16_t *ri, int64_t lo, int64_t hi, int d) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int)ri[mid] < d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <int MT, int STORE>
__global__ __launch_bounds__(64 * CE_WAVES) void count_explain_kernel(CountExplainArgs A) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * CE_WAVES + (threadIdx.x >> 6);
    const int64_t i0 = tile * CE_PTS;
    if (i0 >= A.n) return;                                          // (a whole wave)
    const int npt = A.n - i0 < CE_PTS ? (int)(A.n - i0) : CE_PTS;
    const int K = A.K, D = A.D, top = A.top;
    // ---- the rows of the tile's points
    const int pt = lane & 31, half = lane >> 5;
    const float *col = A.table + i0 + (pt < npt ? pt : 0);          // (lanes past the end read point 0 of the tile and write nothing)
    const int64_t rs = (int64_t)A.rstep * A.stride;
    unsigned long long row = 0ull;
    for (int k = half; k < K; k += 2) {
        const unsigned long long key = ce_row_key(col[(int64_t)k * rs], k);
        row = key > row ? key : row;
    }
    {
        const unsigned long long other = __shfl_xor(row, 32);
        row = other > row ? other : row;
    }
    const unsigned row_hi = (unsigned)(row >> 32);
    const int my_label = (int)(~(unsigned)row);
    const bool my_part = row_hi != CE_ROW_NAN && row_hi != CE_ROW_PINF && row_hi != CE_ROW_NINF;
    if (lane < npt) A.lab[i0 + lane] = my_label;
    unsigned n_inc = 0;
#pragma unroll 1
    for (int p = 0; p < npt; ++p) {
        const int64_t i = i0 + p;
        const int k = __builtin_amdgcn_readfirstlane(__shfl(my_label, p));
        const bool part = __builtin_amdgcn_readfirstlane((int)__shfl((int)my_part, p)) != 0;
        // ---- the total, and the scan for a value the binomial law has no place for
        double t;
        bool bad = false;
        int64_t e0 = 0, e1 = 0;
        if (STORE == COUNTSTATS_F32) {
            const float *x = A.X + i * A.ldx;
            t = cs_wave_total(x, D, lane);
            for (int d = lane; d < D; d += 64) { const float v = x[d]; bad = bad || !(v >= 0.f && v < INFINITY); }
        } else if (STORE == COUNTSTATS_U8) {
            t = cs_wave_total(A.X8 + i * A.ld8, D, lane);
        } else {
            e0 = A.cp[i]; e1 = A.cp[i + 1];
            t = cs_wave_total(A.val + e0, e1 - e0, lane);
            for (int64_t e = e0 + lane; e < e1; e += 64) { const float v = A.val[e]; bad = bad || !(v >= 0.f && v < INFINITY); }
        }
        const bool incomplete = part && (__ballot(bad) != 0ull || !(t > 0.));
        if (incomplete) ++n_inc;
        if (lane == 0) A.tot[i] = part ? t : (double)NAN;
        if (!part || incomplete) {
            if (lane < top) A.features[i * A.ld + lane] = -1;
            continue;
        }
        const double lt = log(t);
        const double *const lth = A.lth + (int64_t)k * D, *const l1m = A.l1m + (int64_t)k * D;
        unsigned long long tk[MT];
#pragma unroll
        for (int j = 0; j < MT; ++j) tk[j] = 0ull;
        // ---- the scores
        if (STORE != COUNTSTATS_SPARSE) {
            for (int d = lane; d < D; d += 64) {
                const double x = STORE == COUNTSTATS_F32 ? (double)A.X[i * A.ldx + d] : (double)A.X8[i * A.ld8 + d];
                const unsigned long long key = ce_key(x, t, lt, lth[d], l1m[d], d, A.side);
                if (key > tk[MT - 1]) ce_insert<MT>(tk, key);
            }
        } else {
            for (int64_t e = e0 + lane; e < e1; e += 64) {
                const int d = (int)A.ri[e];
                if (d >= D) continue;
                const unsigned long long key = ce_key((double)A.val[e], t, lt, lth[d], l1m[d], d, A.side);
                if (key > tk[MT - 1]) ce_insert<MT>(tk, key);
            }
            if (A.side != COUNT_EXPLAIN_OVER) {                    // a feature the point does not hold lies under its expectation
                const int32_t *const ord = A.order + (int64_t)k * D;
#pragma unroll 1
                for (int pos0 = 0; pos0 < D; pos0 += 64) {
                    const int pos = pos0 + lane;
                    if (pos < D) {
                        const int d = ord[pos];
                        const int64_t e = ce_find(A.ri, e0, e1, d);
                        if (!(e < e1 && (int)A.ri[e] == d)) {
                            const unsigned long long key = ce_key(0., t, lt, lth[d], l1m[d], d, A.side);
                            if (key > tk[MT - 1]) ce_insert<MT>(tk, key);
                        }
                    }
                    if (pos0 + 64 >= D) break;
                    // what the rest of the list can reach at most, as a key above every feature index
                    int side;
                    const float rn = ce_score(0., t, lt, 0., l1m[ord[pos0 + 64]], &side);
                    const unsigned long long lim = ((unsigned long long)(__float_as_uint(rn) + 1u) << 32) | 0xffffffffull;
                    int above = 0;
#pragma unroll
                    for (int j = 0; j < MT; ++j) above += tk[j] > lim ? 1 : 0;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) above += __shfl_xor(above, o);
                    if (above >= top) break;
                }
            }
        }
        // ---- the merge: `top` rounds; lane j keeps winner j
        unsigned long long mine = 0ull;
#pragma unroll 1
        for (int r = 0; r < top; ++r) {
            const unsigned long long best = ce_wave_max(tk[0]);
            if (lane == r) mine = best;
            if (best != 0ull && tk[0] == best) {
#pragma unroll
                for (int j = 0; j + 1 < MT; ++j) tk[j] = tk[j + 1];
                tk[MT - 1] = 0ull;
            }
        }
        // ---- the winners: the feature and |residual|, the bits that ranked it; count_explain_finish_kernel does the rest
        if (lane < top) {
            A.features[i * A.ld + lane] = mine ? (int)(~(unsigned)mine) : -1;
            if (mine) A.residual[i * A.ld + lane] = __uint_as_float((unsigned)(mine >> 32) - 1u);
        }
    }
    const unsigned long long skipped = __ballot(lane < npt && !my_part);
    if (lane == 0) {                                                // (these words have no other writer; launches of a stream are ordered)
        A.skip[tile] += (unsigned)__popcll(skipped);
        A.incomplete[tile] += n_inc;
    }
}

// Slot j of point i, one lane each, behind count_explain_kernel: the winner's count from the store, t theta, the sign of the residual -- the
// side by the statements that ranked it -- and the exact binomial tail; NaN throughout for a slot without a candidate; zeros in the padding
// columns j + top, j + 2 top, .. < ld of the five arrays; the lane of slot 0 also writes the point's label and total where asked for.
__global__ __launch_bounds__(256) void count_explain_finish_kernel(CountExplainArgs A) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= A.n * A.top) return;
    const int64_t i = e / A.top, j = e - i * A.top, at = i * A.ld + j;
    const int d = A.features[at];
    const double t = A.tot[i];
    float cnt = NAN, expect = NAN, res = NAN, tail = NAN;
    if (d >= 0) {
        double x;
        if (A.store == COUNTSTATS_F32) x = (double)A.X[i * A.ldx + d];
        else if (A.store == COUNTSTATS_U8) x = (double)A.X8[i * A.ld8 + d];
        else {
            const int64_t e1 = A.cp[i + 1], f = ce_find(A.ri, A.cp[i], e1, d);
            x = (f < e1 && (int)A.ri[f] == d) ? (double)A.val[f] : 0.;
        }
        const int64_t q = (int64_t)A.lab[i] * A.D + d;
        const double lth = A.lth[q], l1m = A.l1m[q];
        const int side = ce_side_of(x, log(t), lth, l1m);
        double th, thc;
        ce_theta(lth, l1m, th, thc);
        const float r = A.residual[at];
        cnt = (float)x;
        expect = (float)(t * th);
        res = side < 0 ? -r : r;
        tail = (float)ce_tail(x, t, side, lth, l1m, nullptr);
    }
    A.count[at] = cnt; A.expected[at] = expect; A.residual[at] = res; A.feature_tail[at] = tail;
    for (int64_t c = j + A.top; c < A.ld; c += A.top) {
        const int64_t z = i * A.ld + c;
        A.features[z] = 0; A.count[z] = 0.f; A.expected[z] = 0.f; A.residual[z] = 0.f; A.feature_tail[z] = 0.f;
    }
    if (j == 0) {
        if (A.labels) A.labels[i] = (int64_t)A.lab[i] + 1;
        if (A.total) A.total[i] = t;
    }
}

template <int MT, int STORE>
static hipError_t launch_ce(const CountExplainArgs &a, unsigned blocks, hipStream_t s) {
    DPMM_LAUNCH((count_explain_kernel<MT, STORE>), dim3(blocks), dim3(64 * CE_WAVES), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    DPMM_LAUNCH(count_explain_finish_kernel, dim3((unsigned)((a.n * a.top + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int STORE>
static hipError_t launch_ce_store(const CountExplainArgs &a, unsigned blocks, hipStream_t s) {
    return a.top <= 4 ? launch_ce<4, STORE>(a, blocks, s) : launch_ce<16, STORE>(a, blocks, s);
}

hipError_t launch_count_explain_range(const CountExplainArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (a.K < 1 || a.K > DPMM_MAX_CLUSTERS_K || a.D < 1 || a.top < 1 || a.top > COUNT_EXPLAIN_MAX_TOP || a.top > a.D || a.ld < a.top || a.side < COUNT_EXPLAIN_BOTH ||
        a.side > COUNT_EXPLAIN_UNDER || a.stride < a.n || !a.table || !a.lth || !a.l1m || !a.order || !a.features || !a.count || !a.expected || !a.residual ||
        !a.feature_tail || !a.skip || !a.incomplete || !a.tot || !a.lab)
        return hipErrorInvalidValue;
    if (a.store == COUNTSTATS_SPARSE ? (!a.cp || a.D > 65536) : a.store == COUNTSTATS_U8 ? (!a.X8 || a.ld8 < a.D) : (a.store != COUNTSTATS_F32 || !a.X || a.ldx < a.D))
        return hipErrorInvalidValue;
    const int64_t blocks = (a.n + CE_PTS * CE_WAVES - 1) / (CE_PTS * CE_WAVES);
    if (blocks >> 31 || (a.n * a.top + 255) / 256 >> 31) return hipErrorInvalidValue;
    if (a.store == COUNTSTATS_SPARSE) return launch_ce_store<COUNTSTATS_SPARSE>(a, (unsigned)blocks, s);
    if (a.store == COUNTSTATS_U8) return launch_ce_store<COUNTSTATS_U8>(a, (unsigned)blocks, s);
    return launch_ce_store<COUNTSTATS_F32>(a, (unsigned)blocks, s);
}

}  // namespace dpmm
