// missing.hip -- points with missing (NaN) features under the Student-t predictive (include/dpmm_hip_missing.h, which states the
// mathematics): between the evaluation of a range of the score table and its finish pass,
//   miss_list_kernel    compacts the positions of the range's points that have 1 .. min(16, D - 1) NaN features and counts those with more.
//                       A NaN feature makes the point's entry NaN under every cluster, so row 0 of the table (n floats, just written)
//                       names the candidates and only their x is looked at; an entry that is NaN for another reason (an Inf feature
//                       against a zero of R) has no NaN feature and is left alone.  One atomic per wave and counter.
//   miss_patch_kernel   one wave per listed point, looping over the clusters; no workgroup barrier anywhere (the list's length is read
//                       from device memory, waves leave when they please).  Lane l carries features / rows l, l + 64, .. (NT = ceil(D / 64)
//                       of them).  Per cluster:
//                         (miss_system, missing_device.h) z = x - m on O, 0 on M; y = R z in Float32 by miss_rz<NT>: column j of R is one coalesced row of the transposed copy Rt
//                         (zero below the diagonal and in the pad), z_j goes round with v_readlane;
//                         g = C'y, A = C'C (C = R[:, M]): columns of Rt again, products and wave sums in Float64; A goes to r x r words of
//                         wave-private LDS, where lane a factors row a (Cholesky, column by column) and the two triangular solves leave t_a
//                         in lane a;
//                         q_o = |y - C t|^2 as the squared norm of the residual; the entry in Float64, rounded once.
//                       The IMPUTE instantiation runs behind it on the patched table: M, S and p_k = e_k / S as score_finish_kernel forms
//                       them (same operations, same bits), t_k by the same steps, and lane a < r accumulates sum_k p_k (m[M_a] - t_a) in
//                       Float64 for the one output word it owns.
//   miss_draw_kernel    (include/dpmm_hip_impute.h, which states the law and the keying) one wave per (listed point, draw) on the patched
//                       table: the cumulative p_k in Float64 against one 53-bit uniform pick k; for that cluster alone y, g, A = L L', t and
//                       q_o by the patch kernel's steps, w = L'^-1 n by its back-substitution from r Float32 Box-Muller normals, g ~ chi^2 by
//                       the sampler's Marsaglia-Tsang; lane a < r writes (m[M_a] - t_a) + sqrt((df + q_o) / g) w_a, Float64 rounded once.
//                       miss_draw_copy_kernel writes the rest of every draw's image in front of it.
//   miss_transpose_kernel   Rt[k][j][i] = R_k[i][j] from the packed upper triangles of the parameter staging, once per parameter set.
// The missing set is not stored: the wave that reads x gets it from a ballot per 64 features.
#include "dpmm_device.h"
#include "dpmm_kernels.h"
#include "sample_device.h"
#include "missing_device.h"

namespace dpmm {

constexpr int MISS_WAVES = 4;                  // waves per workgroup of the patch kernel (they share nothing)

__global__ __launch_bounds__(256) void miss_transpose_kernel(const float *__restrict__ Rpk, int64_t step, float *__restrict__ Rt, int K, int D, int Dp) {
    const int64_t total = (int64_t)K * D * Dp;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int i = (int)(e % Dp);
        const int j = (int)((e / Dp) % D);
        const int k = (int)(e / ((int64_t)Dp * D));
        // packed upper triangle: row i holds the columns i .. D - 1 from word i D - i (i - 1) / 2
        Rt[e] = (i <= j) ? Rpk[(int64_t)k * step + (int64_t)i * D - (int64_t)i * (i - 1) / 2 + (j - i)] : 0.f;
    }
}

__global__ __launch_bounds__(256) void miss_list_kernel(MissArgs A) {
    const int lane = threadIdx.x & 63;
    const int cap = A.D - 1 < MISS_MAX ? A.D - 1 : MISS_MAX;
    // (the 64 points of a trip belong to one wave: its trip count is uniform, the ballots see whole waves)
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); base < A.n; base += (int64_t)gridDim.x * 256) {
        const int64_t i = base + lane;
        int r = 0;
        if (i < A.n) {
            const float a = A.table[i];
            if (a != a) {
                const float *x = A.X + i * A.ldx;
                for (int j = 0; j < A.D; ++j) r += (x[j] != x[j]) ? 1 : 0;
            }
        }
        const bool lst = r >= 1 && r <= cap, over = r > cap;
        const unsigned long long ml = __ballot(lst), mo = __ballot(over);
        if (ml) {
            int at = 0;      // (the list holds at most n < 2^32 entries; `ml` is wave-uniform, so lane 0 is active here)
            if (lane == 0) {
                at = (int)(unsigned)atomicAdd(&A.cnt[0], (unsigned long long)__popcll(ml));
                atomicAdd(&A.cnt[1], (unsigned long long)__popcll(ml));
            }
            const unsigned at0 = (unsigned)__builtin_amdgcn_readfirstlane(at);
            if (lst) A.list[(uint64_t)at0 + (uint64_t)__popcll(ml & ((1ull << lane) - 1ull))] = (uint32_t)i;
        }
        if (mo && lane == 0) atomicAdd(&A.cnt[2], (unsigned long long)__popcll(mo));
    }
}

// M and S of score_finish_kernel from a point's (patched) column: p_k = expf(a_k - M) / S, a NaN entry counting as -Inf
__device__ __forceinline__ void miss_column_ms(const float *col_i, int64_t stride, int K, float &mx, float &ssum) {
    mx = -INFINITY; ssum = 0.f;
    for (int k = 0; k < K; ++k) {
        const float a = col_i[(int64_t)k * stride];
        if (a == a && a > mx) mx = a;
    }
    for (int k = 0; k < K; ++k) {
        float a = col_i[(int64_t)k * stride];
        if (a != a) a = -INFINITY;
        ssum += expf(a - mx);
    }
}
__device__ __forceinline__ float miss_column_p(const float *col_i, int64_t stride, int k, float mx, float ssum) {
    float a = col_i[(int64_t)k * stride];
    if (a != a) a = -INFINITY;
    return expf(a - mx) / ssum;
}

template <int NT, bool IMPUTE>
__global__ __launch_bounds__(64 * MISS_WAVES) void miss_patch_kernel(MissArgs A) {
    __shared__ double sA[MISS_WAVES][MISS_MAX * MISS_LDA];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *const Am = sA[wave];
    const int D = A.D, K = A.K;
    constexpr int Dp = 64 * NT;
    const unsigned long long total = A.cnt[0];
    const unsigned long long nw = (unsigned long long)gridDim.x * MISS_WAVES;
    for (unsigned long long e = (unsigned long long)blockIdx.x * MISS_WAVES + wave; e < total; e += nw) {
        const int64_t i = A.list[e];
        float xv[NT];
        unsigned long long nm[NT];
        int myM;
        const int r = miss_read_point<NT>(A.X + i * A.ldx, D, lane, xv, nm, myM);
        float *const col_i = A.table + i;
        float mx = -INFINITY, ssum = 0.f;
        double acc = 0.0;
        if constexpr (IMPUTE) miss_column_ms(col_i, A.stride, K, mx, ssum);
        for (int k = 0; k < K; ++k) {
            const float *const Rk = A.Rt + (int64_t)k * D * Dp;
            const float *const mk = A.mu + (int64_t)k * A.mu_step;
            float y[NT];
            double gl;
            const double half_logdet = miss_system<NT>(Rk, mk, xv, nm, myM, r, D, lane, Am, y, gl);
            miss_lds_fence();      // (the next cluster overwrites A)
            if constexpr (IMPUTE) {
                const float pk = miss_column_p(col_i, A.stride, k, mx, ssum);
                if (lane < r) acc += (double)pk * ((double)mk[myM] - gl);
            } else {
                const double q = miss_residual<NT>(Rk, y, gl, myM, r, lane);
                const double *ck = A.cst + (int64_t)k * MISS_CST;
                const double df = ck[0];
                const double val = ck[r] - half_logdet - 0.5 * (df + (double)(D - r)) * log1p(q / df);
                if (lane == 0) col_i[(int64_t)k * A.stride] = (float)val;
            }
        }
        if constexpr (IMPUTE) {
            if (lane < r) A.out[i * A.ld_out + myM] = (float)acc;
        }
    }
}

// ---- include/dpmm_hip_impute.h: draws of the missing features.  The copy writes every draw's image of the range (the points as they are,
// zeros in the pad, comp = -1); the draw kernel then rewrites the NaN words of the listed points, one wave per (listed point, draw).
__global__ __launch_bounds__(256) void miss_draw_copy_kernel(MissArgs A, MissDraw W, int64_t width) {
    const int64_t step = (int64_t)gridDim.x * 256, q0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t words = (int64_t)W.ndraws * A.n * width;
    for (int64_t e = q0; e < words; e += step) {
        const int64_t d = e % width, i = (e / width) % A.n, jd = e / (width * A.n);
        W.out[jd * W.draw_stride + i * W.ld + d] = d < A.D ? A.X[i * A.ldx + d] : 0.f;
    }
    if (W.comp)
        for (int64_t e = q0; e < (int64_t)W.ndraws * A.n; e += step) W.comp[(e / A.n) * W.comp_stride + e % A.n] = -1;
}

template <int NT>
__global__ __launch_bounds__(64 * MISS_WAVES) void miss_draw_kernel(MissArgs A, MissDraw W) {
    __shared__ double sA[MISS_WAVES][MISS_MAX * MISS_LDA];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *const Am = sA[wave];
    const int D = A.D, K = A.K;
    constexpr int Dp = 64 * NT;
    const unsigned long long nd = (unsigned long long)W.ndraws;
    const unsigned long long total = A.cnt[0] * nd;
    const unsigned long long nw = (unsigned long long)gridDim.x * MISS_WAVES;
    for (unsigned long long item = (unsigned long long)blockIdx.x * MISS_WAVES + wave; item < total; item += nw) {
        const unsigned long long e = item / nd;      // (the draws of a point are neighbours: its row and its column stay in the cache)
        const int64_t jd = (int64_t)(item - e * nd);
        const int64_t i = A.list[e];
        float xv[NT];
        unsigned long long nm[NT];
        int myM;
        const int r = miss_read_point<NT>(A.X + i * A.ldx, D, lane, xv, nm, myM);
        const uint64_t gi = (uint64_t)(W.i0 + i);
        const uint32_t b0 = 64u * (uint32_t)(W.draw0 + jd);
        // ---- the component: the cumulative sums of p_k in cluster order, inverted with one uniform
        const float *const col_i = A.table + i;
        float mx, ssum;
        miss_column_ms(col_i, A.stride, K, mx, ssum);
        const Philox4 rc = philox4x32_10(W.seed, gi, b0, STREAM_IMPUTE_COMP);
        const double u = sample_u53(rc.v[0], rc.v[1]);
        double cum = 0.0;
        int k = -1, klast = 0;      // (no cluster of positive probability -- an infinite observed feature --: cluster 0)
        for (int kk = 0; kk < K && k < 0; ++kk) {
            const float pk = miss_column_p(col_i, A.stride, kk, mx, ssum);
            if (!(pk > 0.f)) continue;
            cum += (double)pk;
            klast = kk;
            if (u < cum) k = kk;
        }
        k = __builtin_amdgcn_readfirstlane(k < 0 ? klast : k);
        // ---- that cluster's system, w = L'^-1 n and q_o
        const float *const Rk = A.Rt + (int64_t)k * D * Dp;
        const float *const mk = A.mu + (int64_t)k * A.mu_step;
        float y[NT];
        double gl;
        miss_system<NT>(Rk, mk, xv, nm, myM, r, D, lane, Am, y, gl);
        float nv = 0.f;
        if (lane < r) {       // coordinate a of n: word a & 3 of block a >> 2, Box-Muller as sample_niw_kernel
            const Philox4 rn = philox4x32_10(W.seed, gi, b0 + (uint32_t)(lane >> 2), STREAM_IMPUTE_NORMAL);
            const bool hi = (lane & 2) != 0;
            const float rad = sqrtf(fmaxf(-2.0f * __logf(sample_u32(hi ? rn.v[2] : rn.v[0])), 0.0f));
            const float th = 6.2831853071795865f * sample_u32(hi ? rn.v[3] : rn.v[1]);
            nv = rad * ((lane & 1) ? __sinf(th) : __cosf(th));
        }
        double wv = (double)nv;
        for (int j = r - 1; j >= 0; --j) {
            if (lane == j) wv = wv / Am[j * MISS_LDA + j];
            const double wj = miss_rl_d(wv, j);
            if (lane < j) wv -= Am[j * MISS_LDA + lane] * wj;
        }
        miss_lds_fence();      // (the next item overwrites A)
        const double q = miss_residual<NT>(Rk, y, gl, myM, r, lane);
        const double dfo = A.cst[(int64_t)k * MISS_CST] + (double)(D - r);
        const double g = sample_chi2(dfo, W.seed, gi, STREAM_IMPUTE_CHI, b0);
        const double sc = sqrt((A.cst[(int64_t)k * MISS_CST] + q) / g);
        if (lane < r) W.out[jd * W.draw_stride + i * W.ld + myM] = (float)(((double)mk[myM] - gl) + sc * wv);
        if (W.comp && lane == 0) W.comp[jd * W.comp_stride + i] = k;
    }
}

template <bool IMPUTE>
static void launch_patch_nt(const MissArgs &a, int grid, hipStream_t s) {
    const int nt = (a.D + 63) / 64;
    if (nt == 1) DPMM_LAUNCH((miss_patch_kernel<1, IMPUTE>), dim3(grid), dim3(64 * MISS_WAVES), 0, s, a);
    else if (nt == 2) DPMM_LAUNCH((miss_patch_kernel<2, IMPUTE>), dim3(grid), dim3(64 * MISS_WAVES), 0, s, a);
    else if (nt == 3) DPMM_LAUNCH((miss_patch_kernel<3, IMPUTE>), dim3(grid), dim3(64 * MISS_WAVES), 0, s, a);
    else DPMM_LAUNCH((miss_patch_kernel<4, IMPUTE>), dim3(grid), dim3(64 * MISS_WAVES), 0, s, a);
}

static bool miss_args_ok(const MissArgs &a) { return a.K >= 1 && a.D >= 1 && a.D <= 256 && a.n <= a.stride && a.n <= (int64_t)0xffffffffll; }

hipError_t launch_miss_transpose(const float *Rpk, int64_t step, float *Rt, int K, int D, hipStream_t s) {
    if (K < 1 || D < 1 || D > 256) return hipErrorInvalidValue;
    const int Dp = miss_pitch(D);
    const int64_t total = (int64_t)K * D * Dp;
    DPMM_LAUNCH(miss_transpose_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 4096)), dim3(256), 0, s, Rpk, step, Rt, K, D, Dp);
    return hipGetLastError();
}

hipError_t launch_miss_list(const MissArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (!miss_args_ok(a)) return hipErrorInvalidValue;
    DPMM_LAUNCH(miss_list_kernel, dim3((unsigned)std::min<int64_t>((a.n + 255) / 256, 2048)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_miss_patch(const MissArgs &a, bool impute, int max_grid, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    if (!miss_args_ok(a) || (impute && (!a.out || a.ld_out < a.D))) return hipErrorInvalidValue;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((a.n + MISS_WAVES - 1) / MISS_WAVES, max_grid));
    if (impute) launch_patch_nt<true>(a, grid, s);
    else launch_patch_nt<false>(a, grid, s);
    return hipGetLastError();
}

hipError_t launch_miss_draw(const MissArgs &a, const MissDraw &w, int max_grid, hipStream_t s) {
    if (a.n <= 0 || w.ndraws <= 0) return hipSuccess;
    const int64_t width = std::min<int64_t>(w.ld, w.draw_stride);
    if (!miss_args_ok(a) || !w.out || width < a.D || w.i0 < 0 || w.draw0 < 0 || w.draw0 + w.ndraws > MISS_DRAW_MAX) return hipErrorInvalidValue;
    const int64_t words = (int64_t)w.ndraws * a.n * width, items = (int64_t)w.ndraws * a.n;
    DPMM_LAUNCH(miss_draw_copy_kernel, dim3((unsigned)std::min<int64_t>((words + 255) / 256, 4096)), dim3(256), 0, s, a, w, width);
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((items + MISS_WAVES - 1) / MISS_WAVES, max_grid));
    const int nt = (a.D + 63) / 64;
    if (nt == 1) DPMM_LAUNCH((miss_draw_kernel<1>), dim3(grid), dim3(64 * MISS_WAVES), 0, s, a, w);
    else if (nt == 2) DPMM_LAUNCH((miss_draw_kernel<2>), dim3(grid), dim3(64 * MISS_WAVES), 0, s, a, w);
    else if (nt == 3) DPMM_LAUNCH((miss_draw_kernel<3>), dim3(grid), dim3(64 * MISS_WAVES), 0, s, a, w);
    else DPMM_LAUNCH((miss_draw_kernel<4>), dim3(grid), dim3(64 * MISS_WAVES), 0, s, a, w);
    return hipGetLastError();
}

}  // namespace dpmm
