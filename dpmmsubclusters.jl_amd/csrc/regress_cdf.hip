// regress_cdf.hip -- conditional CDF and quantiles of every target (include/dpmm_hip_regress_cdf.h): from a range of the score table and the
// range's points to F_id(y) = sum_k p_ik T_nu_k((y - mu_ikd) / sigma_ikd) at given y, and to the y at which F_id reaches given levels.
//
// Both kernels keep the tile of regress_kernel (regress.hip, regress_device.h), in statements of their own (see regress_device.h): 32 points per workgroup, one wave per 32 targets, the points staged transposed
// in LDS, the row of the table walked with score_device.h (p_ik has the bits `probs` holds), clusters whose p is 0 for the whole tile left
// out, mu_ikd the SAME Float32 chain (accumulator started from c, v_mfma_f32_32x32x2_f32 in increasing e), q_ik recovered from the table
// entry as regress_kernel's STD branch does, and the results leave through the wave-private LDS tile as 128-byte segments.
//
// A lane holds 16 targets of one point.  The Float64 tail (typicality_math.h, a continued fraction) is not unrolled 16 times: the 16
// arguments of a lane go through 16 words of LDS that only this lane reads and writes (ex[r * 64 + lane]) -- storage a run-time loop can
// index, where registers would need scratch -- and come back as the half tail with the sign of t.  No cross-lane traffic, so no barrier.
//
// The quantile kernel solves level by level, in increasing level.  Per (point, target): the bracket [min_k y_kq, max_k y_kq],
// y_kq = mu_ikd + sigma_ikd z_kq, over the clusters with p_ik != 0, widened to Float32 values; a point with one such cluster gets y_kq
// itself.  Otherwise candidates are Float32 values inside the bracket, ordered as integers: F and the density f at the candidate in
// Float64 (the chains are run again for every candidate: cheap beside the continued fractions), the bracket end on the candidate's side
// replaced, and the next candidate is Newton's y - (F - level) / f -- its Float32 neighbour on the far side if it rounds to y itself --
// when it lies strictly inside the bracket and the step made progress (the bracket or |F - level| at least halved, or Newton moves by one
// Float32 value at most: it has arrived, and the neighbour closes the bracket); else the arithmetic
// midpoint; and the midpoint of the ORDERED INTEGERS once the candidates left (RC_CAP in all) are only just enough for pure bisection
// to bring the ends to adjacent Float32 values.  The loop has that fixed trip count; it is left early only when every lane of the wave is
// done.  The root is the upper end -- the smallest Float32 y of the bracket with F(y) >= level -- so it is non-decreasing in the level up to
// the rounding of F; a running maximum over the increasing levels makes that hold by construction.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "score_device.h"
#include "typicality_math.h"

namespace dpmm {

typedef float rc_f32x16 __attribute__((ext_vector_type(16)));

constexpr int RC_PTS = 32;               // points per workgroup
constexpr int RC_XP = 33;                // words per feature row of the staged points
constexpr int RC_MAXW = 4;               // waves per workgroup at most: 32 targets each
constexpr int RC_CAP = 48;               // candidates per root at most: 32 for pure bisection over the Float32 values, 16 to spare

// the staged points: xs[e * 33 + p], zeros past the end of the range; bad[p]: a feature of point p is not finite.  Ends with a barrier.
__device__ __forceinline__ void rc_stage(const float *X, int64_t ldx, int64_t i0, int npt, int D, float *xs, int *bad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (threadIdx.x < RC_PTS) bad[threadIdx.x] = 0;
    __syncthreads();
    for (int p = wave; p < RC_PTS; p += nw) {
        const float *row = X + (i0 + (p < npt ? p : 0)) * ldx;
        bool nf = false;
        for (int e = lane; e < D; e += 64) {
            const float v = p < npt ? row[e] : 0.f;
            nf = nf || !(fabsf(v) < INFINITY);
            xs[e * RC_XP + p] = v;
        }
        if (__ballot(nf) && lane == 0) bad[p] = 1;
    }
    __syncthreads();
}

// mu of cluster k for point lane & 31 and the targets t0 + 8 (r >> 2) + 4 (lane >> 5) + (r & 3): regress_kernel's chain, statement by statement
__device__ __forceinline__ rc_f32x16 rc_chain(const float *c, const float *Bt, const float *xs, int k, int D, int Tp, int t0, int pt, int half) {
    const float *ck = c + (int64_t)k * Tp + t0 + 4 * half;
    rc_f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 c4 = *reinterpret_cast<const float4 *>(ck + 8 * g);
        acc[4 * g] = c4.x; acc[4 * g + 1] = c4.y; acc[4 * g + 2] = c4.z; acc[4 * g + 3] = c4.w;
    }
    const float *bk = Bt + ((int64_t)k * D + half) * Tp + t0 + pt;
    const float *xk = xs + half * RC_XP + pt;
    int e = 0;
    for (; e + 8 <= D; e += 8) {
        const float b0 = bk[(int64_t)e * Tp], b1 = bk[(int64_t)(e + 2) * Tp], b2 = bk[(int64_t)(e + 4) * Tp], b3 = bk[(int64_t)(e + 6) * Tp];
        const float x0 = xk[e * RC_XP], x1 = xk[(e + 2) * RC_XP], x2 = xk[(e + 4) * RC_XP], x3 = xk[(e + 6) * RC_XP];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b0, x0, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b1, x1, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b2, x2, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b3, x3, acc, 0, 0, 0);
    }
    for (; e < D; e += 2) {
        const bool in = e + half < D;
        const float b = in ? bk[(int64_t)e * Tp] : 0.f;
        const float x = in ? xk[e * RC_XP] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(b, x, acc, 0, 0, 0);
    }
    return acc;
}

// (df_k + q_ik) / (df_k + D_o), q_ik from the table entry a as regress_kernel recovers it
__device__ __forceinline__ double rc_scale(const double *hd, int k, float a, double dDo, double *nu) {
    const double h = hd[2 * k], df = hd[2 * k + 1];
    double q = df * expm1(2.0 * (h - (double)a) / (df + dDo));
    q = q > 0.0 ? q : 0.0;
    *nu = df + dDo;
    return (df + q) / (df + dDo);
}

// the 16 V_kd of a lane times sc, rooted: sigma_ikd
__device__ __forceinline__ void rc_sigma(const float *V, int k, int Tp, int t0, int half, double sc, double *sig) {
    const float *vk = V + (int64_t)k * Tp + t0 + 4 * half;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v4 = *reinterpret_cast<const float4 *>(vk + 8 * g);
        sig[4 * g] = sqrt(sc * (double)v4.x); sig[4 * g + 1] = sqrt(sc * (double)v4.y);
        sig[4 * g + 2] = sqrt(sc * (double)v4.z); sig[4 * g + 3] = sqrt(sc * (double)v4.w);
    }
}

// rows of `out` for the points of the tile from the wave's LDS tile (word pt * 33 + target), two points per trip
__device__ __forceinline__ void rc_flush(float *out, int64_t row0, int64_t ld, const float *os, int npt, int nt, int t0, int pt, int half) {
    __builtin_amdgcn_wave_barrier();
    for (int p = half; p < npt; p += 2)
        if (pt < nt) out[(row0 + p) * ld + t0 + pt] = os[p * RC_XP + pt];
    __builtin_amdgcn_wave_barrier();
}

__global__ __launch_bounds__(64 * RC_MAXW) void regress_cdf_kernel(RegressCdfArgs A) {
    extern __shared__ double rc_smem[];
    __shared__ int bad[RC_PTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int pt = lane & 31, half = lane >> 5;
    const int D = A.D, K = A.K, Tp = A.Tp;
    double *const ex = rc_smem + wave * (16 * 64);
    float *const xs = reinterpret_cast<float *>(rc_smem + nw * (16 * 64));
    float *const os = xs + D * RC_XP + wave * (RC_PTS * RC_XP);
    const int64_t i0 = (int64_t)blockIdx.x * RC_PTS;
    const int npt = A.n - i0 < RC_PTS ? (int)(A.n - i0) : RC_PTS;
    rc_stage(A.X, A.ldx, i0, npt, D, xs, bad);
    // ---- the point's row of the table: M, label, S (score_device.h)
    const int64_t i = i0 + pt;
    const bool valid = pt < npt;
    const float *col = A.table + (valid ? i : 0);
    const int64_t rs = A.stride;
    float m = -INFINITY;
    int best = 0;
    bool nan_seen = false;
    for (int k = 0; k < K; ++k) score_max_step(col[(int64_t)k * rs], k, m, best, nan_seen);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += score_e(col[(int64_t)k * rs], m);
    const bool part = valid && !nan_seen && m > -INFINITY && m < INFINITY && !bad[pt];
    const int tb = blockIdx.y * nw + wave;
    if (blockIdx.y == 0 && wave == 0) {
        if (valid && half == 0 && A.labels) A.labels[i] = best + 1;
        const unsigned long long sm = __ballot(valid && half == 0 && !part);
        if (lane == 0) A.skip[blockIdx.x] += (unsigned)__popcll(sm);
    }
    if (tb * 32 >= Tp) return;                          // (a whole wave; no barrier below)
    const int t0 = tb * 32;
    const int nt = A.Dt - t0 < 32 ? A.Dt - t0 : 32;
    // ---- y of the tile through the wave's LDS tile: coalesced reads, then the lane's 16
    for (int p = half; p < RC_PTS; p += 2) os[p * RC_XP + pt] = (p < npt && pt < nt) ? A.y[(i0 + p) * A.ldy + t0 + pt] : 0.f;
    __builtin_amdgcn_wave_barrier();
    float y[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) y[r] = os[pt * RC_XP + 8 * (r >> 2) + 4 * half + (r & 3)];
    __builtin_amdgcn_wave_barrier();
    double sumc[16], sums[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { sumc[r] = 0.0; sums[r] = 0.0; }
    const double dDo = (double)D;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const float a = col[(int64_t)k * rs];
        const float p = part ? score_p(score_e(a, m), s) : 0.f;
        if (__ballot(p != 0.f) == 0) continue;
        const rc_f32x16 acc = rc_chain(A.c, A.Bt, xs, k, D, Tp, t0, pt, half);
        if (p != 0.f) {
            double nu, sig[16];
            const double sc = rc_scale(A.hd, k, a, dDo, &nu);
            rc_sigma(A.V, k, Tp, t0, half, sc, sig);
#pragma unroll
            for (int r = 0; r < 16; ++r) ex[r * 64 + lane] = ((double)y[r] - (double)acc[r]) / sig[r];
#pragma unroll 1
            for (int r = 0; r < 16; ++r) {
                const double t = ex[r * 64 + lane];
                ex[r * 64 + lane] = copysign(0.5 * typ_tail(t * t, nu, 1, nullptr), t);
            }
            const double pd = (double)p;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const double v = ex[r * 64 + lane], hh = fabs(v);
                const bool neg = signbit(v);
                sumc[r] += pd * (neg ? hh : 1.0 - hh);
                sums[r] += pd * (neg ? 1.0 - hh : hh);
            }
        }
    }
    // ---- out
    const float fnan = __uint_as_float(0x7fc00000u);
    for (int pass = 0; pass < (A.sf ? 2 : 1); ++pass) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = (float)(pass == 0 ? sumc[r] : sums[r]);
            if (y[r] == INFINITY) v = pass == 0 ? 1.f : 0.f;
            if (y[r] == -INFINITY) v = pass == 0 ? 0.f : 1.f;
            if (!part || y[r] != y[r]) v = fnan;
            os[pt * RC_XP + 8 * (r >> 2) + 4 * half + (r & 3)] = v;
        }
        rc_flush(pass == 0 ? A.cdf : A.sf, i0, A.ld, os, npt, nt, t0, pt, half);
    }
    // ---- the padding columns [Dt, ld): zeros, by the wave that owns the last block of targets
    if (t0 + 32 >= Tp && A.ld > A.Dt) {
        const int64_t w = A.ld - A.Dt;
        for (int p = 0; p < npt; ++p)
            for (int64_t j = lane; j < w; j += 64) {
                A.cdf[(i0 + p) * A.ld + A.Dt + j] = 0.f;
                if (A.sf) A.sf[(i0 + p) * A.ld + A.Dt + j] = 0.f;
            }
    }
}

// Float32 values in their order as integers (-0 and +0 both 0), and back
__device__ __forceinline__ int rc_ord(float x) {
    const int b = __float_as_int(x);
    return b >= 0 ? b : (int)(0x80000000u - (unsigned)b);
}
__device__ __forceinline__ float rc_unord(int o) { return __int_as_float(o >= 0 ? o : (int)(0x80000000u - (unsigned)o)); }
// the largest Float32 value <= v / the smallest >= v, as ordered integers (v finite or infinite, not NaN)
__device__ __forceinline__ int rc_ord_down(double v) {
    const float f = (float)v;
    const int o = rc_ord(f);
    return (double)f > v ? o - 1 : o;
}
__device__ __forceinline__ int rc_ord_up(double v) {
    const float f = (float)v;
    const int o = rc_ord(f);
    return (double)f < v ? o + 1 : o;
}

__global__ __launch_bounds__(64 * RC_MAXW) void regress_quantile_kernel(RegressQuantileArgs A) {
    extern __shared__ double rc_smem[];
    __shared__ int bad[RC_PTS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int pt = lane & 31, half = lane >> 5;
    const int D = A.D, K = A.K, Tp = A.Tp, L = A.L;
    double *const ex = rc_smem + wave * (32 * 64);       // [r][lane]: t, then the signed half tail; [16 + r][lane]: sigma, then the density
    float *const xs = reinterpret_cast<float *>(rc_smem + nw * (32 * 64));
    float *const os = xs + D * RC_XP + wave * (RC_PTS * RC_XP);
    const int64_t i0 = (int64_t)blockIdx.x * RC_PTS;
    const int npt = A.n - i0 < RC_PTS ? (int)(A.n - i0) : RC_PTS;
    rc_stage(A.X, A.ldx, i0, npt, D, xs, bad);
    const int64_t i = i0 + pt;
    const bool valid = pt < npt;
    const float *col = A.table + (valid ? i : 0);
    const int64_t rs = A.stride;
    float m = -INFINITY;
    int best = 0;
    bool nan_seen = false;
    for (int k = 0; k < K; ++k) score_max_step(col[(int64_t)k * rs], k, m, best, nan_seen);
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += score_e(col[(int64_t)k * rs], m);
    const bool part = valid && !nan_seen && m > -INFINITY && m < INFINITY && !bad[pt];
    const int tb = blockIdx.y * nw + wave;
    if (blockIdx.y == 0 && wave == 0) {
        if (valid && half == 0 && A.labels) A.labels[i] = best + 1;
        const unsigned long long sm = __ballot(valid && half == 0 && !part);
        if (lane == 0) A.skip[blockIdx.x] += (unsigned)__popcll(sm);
    }
    if (tb * 32 >= Tp) return;                          // (a whole wave; no barrier below)
    const int t0 = tb * 32;
    const int nt = A.Dt - t0 < 32 ? A.Dt - t0 : 32;
    const double dDo = (double)D;
    // ---- the clusters of this lane's point with p != 0: how many; the last one's mu and sigma (all there is to know if it is the only one)
    int nz = 0, k1 = 0;
    float mu1[16];
    double sig1[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { mu1[r] = 0.f; sig1[r] = 0.0; }
    if (part)
        for (int k = 0; k < K; ++k)
            if (score_p(score_e(col[(int64_t)k * rs], m), s) != 0.f) { ++nz; k1 = k; }
    const bool solve = __ballot(nz > 1) != 0;          // a tile of points with one cluster each runs every chain once, and none per level
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const float a = col[(int64_t)k * rs];
        const float p = part ? score_p(score_e(a, m), s) : 0.f;
        if (__ballot(p != 0.f && nz == 1) == 0) continue;
        const rc_f32x16 acc = rc_chain(A.c, A.Bt, xs, k, D, Tp, t0, pt, half);
        if (p != 0.f && nz == 1) {
            double nu;
            const double sc = rc_scale(A.hd, k, a, dDo, &nu);
            rc_sigma(A.V, k, Tp, t0, half, sc, sig1);
#pragma unroll
            for (int r = 0; r < 16; ++r) mu1[r] = acc[r];
        }
    }
    const float fnan = __uint_as_float(0x7fc00000u);
    float prev[16];                                      // the root of the level before: the running maximum
#pragma unroll
    for (int r = 0; r < 16; ++r) prev[r] = -INFINITY;
#pragma unroll 1
    for (int lv = 0; lv < L; ++lv) {
        const double level = A.levels[lv];
        int ilo[16], ihi[16], iy[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) ilo[r] = ihi[r] = iy[r] = 0;
        if (nz == 1) {
            const double z = A.z[(int64_t)k1 * L + lv];
#pragma unroll
            for (int r = 0; r < 16; ++r) ilo[r] = ihi[r] = iy[r] = rc_ord((float)((double)mu1[r] + sig1[r] * z));
        }
        if (solve) {
            // ---- the bracket of the lanes with several clusters
            double ylo[16], yhi[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) { ylo[r] = INFINITY; yhi[r] = -INFINITY; }
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const float a = col[(int64_t)k * rs];
                const float p = part ? score_p(score_e(a, m), s) : 0.f;
                if (__ballot(p != 0.f && nz > 1) == 0) continue;
                const rc_f32x16 acc = rc_chain(A.c, A.Bt, xs, k, D, Tp, t0, pt, half);
                if (p != 0.f && nz > 1) {
                    double nu, sig[16];
                    const double sc = rc_scale(A.hd, k, a, dDo, &nu);
                    rc_sigma(A.V, k, Tp, t0, half, sc, sig);
                    const double z = A.z[(int64_t)k * L + lv];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const double yk = (double)acc[r] + sig[r] * z;
                        ylo[r] = yk < ylo[r] ? yk : ylo[r];
                        yhi[r] = yk > yhi[r] ? yk : yhi[r];
                    }
                }
            }
            float res[16];                               // |F - level| at the candidate before (progress is judged against it)
            if (nz > 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    ilo[r] = rc_ord_down(ylo[r]); ihi[r] = rc_ord_up(yhi[r]);
                    const int mid = rc_ord((float)(0.5 * (ylo[r] + yhi[r])));
                    iy[r] = (mid > ilo[r] && mid < ihi[r]) ? mid : ilo[r] + (int)(((int64_t)ihi[r] - ilo[r]) >> 1);
                    res[r] = INFINITY;
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) res[r] = 0.f;
            }
            // ---- the candidates
#pragma unroll 1
            for (int it = 0; it < RC_CAP; ++it) {
                unsigned act = 0;                        // bit r: the ends of root r are not adjacent yet
                if (nz > 1) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) act |= ((int64_t)ihi[r] - ilo[r] > 1) ? 1u << r : 0u;
                }
                if (__ballot(act != 0) == 0) break;
                double F[16], f[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) { F[r] = 0.0; f[r] = 0.0; }
#pragma unroll 1
                for (int k = 0; k < K; ++k) {
                    const float a = col[(int64_t)k * rs];
                    const float p = part ? score_p(score_e(a, m), s) : 0.f;
                    if (__ballot(p != 0.f && act != 0) == 0) continue;
                    const rc_f32x16 acc = rc_chain(A.c, A.Bt, xs, k, D, Tp, t0, pt, half);
                    if (p != 0.f && act != 0) {
                        double nu, sig[16];
                        const double sc = rc_scale(A.hd, k, a, dDo, &nu);
                        rc_sigma(A.V, k, Tp, t0, half, sc, sig);
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            ex[r * 64 + lane] = ((double)rc_unord(iy[r]) - (double)acc[r]) / sig[r];
                            ex[(16 + r) * 64 + lane] = sig[r];
                        }
                        const double lc = A.lc[k], hn = 0.5 * (nu + 1.0);
#pragma unroll 1
                        for (int r = 0; r < 16; ++r) {
                            if (!(act >> r & 1)) continue;
                            const double t = ex[r * 64 + lane], t2 = t * t;
                            ex[r * 64 + lane] = copysign(0.5 * typ_tail(t2, nu, 1, nullptr), t);
                            ex[(16 + r) * 64 + lane] = exp(lc - hn * log1p(t2 / nu)) / ex[(16 + r) * 64 + lane];
                        }
                        const double pd = (double)p;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const double v = ex[r * 64 + lane], hh = fabs(v);
                            F[r] += pd * (signbit(v) ? hh : 1.0 - hh);
                            f[r] += pd * ex[(16 + r) * 64 + lane];
                        }
                    }
                }
                const int left = RC_CAP - 1 - it;        // candidates after this one
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (!(act >> r & 1)) continue;
                    const int64_t w_old = (int64_t)ihi[r] - ilo[r];
                    const bool below = F[r] < level;
                    if (below) ilo[r] = iy[r]; else ihi[r] = iy[r];
                    const int64_t w = (int64_t)ihi[r] - ilo[r];
                    const double dF = F[r] - level;
                    const float rnow = (float)fabs(dF);
                    const bool progress = 2 * w <= w_old || 2.f * rnow <= res[r];
                    res[r] = rnow;
                    const double yc = (double)rc_unord(iy[r]);
                    int in = rc_ord((float)(yc - dF / f[r]));
                    const bool near = in >= iy[r] - 1 && in <= iy[r] + 1;      // Newton has arrived: the root is next to y
                    if (in == iy[r]) in = below ? iy[r] + 1 : iy[r] - 1;
                    const int imid = ilo[r] + (int)(w >> 1);
                    const int amid = rc_ord((float)(0.5 * ((double)rc_unord(ilo[r]) + (double)rc_unord(ihi[r]))));
                    const bool spare = left >= 34 || w <= ((int64_t)1 << (left > 0 ? left - 1 : 0));
                    int next = imid;
                    if (spare) {
                        if ((progress || near) && in > ilo[r] && in < ihi[r]) next = in;
                        else if (amid > ilo[r] && amid < ihi[r]) next = amid;
                    }
                    iy[r] = next;
                }
            }
            if (nz > 1) {
#pragma unroll
                for (int r = 0; r < 16; ++r)            // the upper end; the midpoint if the candidates ran out first
                    iy[r] = ((int64_t)ihi[r] - ilo[r] > 1) ? ilo[r] + (int)(((int64_t)ihi[r] - ilo[r]) >> 1) : ihi[r];
            }
        }
        // ---- out: level lv of every point of the tile
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = nz >= 1 ? rc_unord(iy[r]) : fnan;
            v = v > prev[r] ? v : prev[r];
            prev[r] = v;
            os[pt * RC_XP + 8 * (r >> 2) + 4 * half + (r & 3)] = (part && nz >= 1) ? v : fnan;
        }
        rc_flush(A.out + lv * A.ld, i0, A.ld * L, os, npt, nt, t0, pt, half);
        if (t0 + 32 >= Tp && A.ld > A.Dt) {
            const int64_t w = A.ld - A.Dt;
            for (int p = 0; p < npt; ++p)
                for (int64_t j = lane; j < w; j += 64) A.out[((i0 + p) * L + lv) * A.ld + A.Dt + j] = 0.f;
        }
    }
}

// the most either kernel asks for: 4 waves, D = 256 (DPMM_MAX_D): 64 KiB of lane words, 33 KiB of points, 16.5 KiB of output tiles
constexpr int RC_LDS_MAX = 8 * RC_MAXW * 32 * 64 + 4 * (256 * RC_XP + RC_MAXW * RC_PTS * RC_XP);

static bool rc_shape_ok(int64_t n, int K, int D, int Dt, int Tp, int64_t ld) {
    return K >= 1 && D >= 1 && D <= 256 && Dt >= 1 && Tp % 32 == 0 && Tp >= Dt && ld >= Dt && !(((n + RC_PTS - 1) / RC_PTS) >> 31);
}

hipError_t launch_regress_cdf_range(const RegressCdfArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (!rc_shape_ok(a.n, a.K, a.D, a.Dt, a.Tp, a.ld) || a.ldy < a.Dt) return hipErrorInvalidValue;
    const int blocks = a.Tp / 32;
    const int nw = blocks < RC_MAXW ? blocks : RC_MAXW;
    const dim3 grid((unsigned)((a.n + RC_PTS - 1) / RC_PTS), (unsigned)((blocks + nw - 1) / nw));
    const size_t lds = sizeof(double) * (size_t)nw * 16 * 64 + sizeof(float) * ((size_t)a.D * RC_XP + (size_t)nw * RC_PTS * RC_XP);
    static bool attr = false;
    if (!attr) { hipFuncSetAttribute((const void *)regress_cdf_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RC_LDS_MAX); attr = true; }
    DPMM_LAUNCH(regress_cdf_kernel, grid, dim3(64 * nw), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_regress_quantile_range(const RegressQuantileArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (!rc_shape_ok(a.n, a.K, a.D, a.Dt, a.Tp, a.ld) || a.L < 1 || a.L > REGRESS_MAX_LEVELS) return hipErrorInvalidValue;
    const int blocks = a.Tp / 32;
    const int nw = blocks < RC_MAXW ? blocks : RC_MAXW;
    const dim3 grid((unsigned)((a.n + RC_PTS - 1) / RC_PTS), (unsigned)((blocks + nw - 1) / nw));
    const size_t lds = sizeof(double) * (size_t)nw * 32 * 64 + sizeof(float) * ((size_t)a.D * RC_XP + (size_t)nw * RC_PTS * RC_XP);
    static bool attr = false;
    if (!attr) { hipFuncSetAttribute((const void *)regress_quantile_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, RC_LDS_MAX); attr = true; }
    DPMM_LAUNCH(regress_quantile_kernel, grid, dim3(64 * nw), lds, s, a);
    return hipGetLastError();
}

}  // namespace dpmm
