/*
 * dpmm_hip_sample.h -- optional companion of dpmm_hip.h: drawing new points from a fitted model into caller-owned device memory.
 * Additive: DPMM_ABI_VERSION is unchanged.
 *
 * The laws are the ones dpmm_set_predictive_* scores with:
 *   NIW           x = m_k + sqrt(df_k / g) A_k z,  z ~ N(0, I_D), g ~ chi^2(df_k) = 2 Gamma(df_k / 2): the multivariate Student-t
 *                 MvT(df_k, m_k, A_k A_k') with A_k = sqrt((kappa + 1) / (kappa df)) U upper triangular, 1 <= D <= DPMM_MAX_DIM_NIW;
 *   Multinomial   x ~ Multinomial(trials, theta_k), every trial one draw from an alias table (Walker / Vose) of D buckets:
 *                 bucket j = (uint64(r0) * D) >> 32; category j if r1 < thr[k][j], else alias[k][j].  Integer arithmetic only.
 * The caller states which points belong to which cluster: sample i (GLOBAL index, counted from 0 over the whole draw) is of cluster k
 * when cluster_start[k] <= i < cluster_start[k + 1]; the points come grouped by cluster.
 *
 * Keying.  Every random word comes from Philox4x32-10 with key `seed` and counter (i low, i high, block, stream): i the GLOBAL sample
 * index, `block` a block number, `stream` one of
 *   40 (normals)       block b -> z[4b .. 4b + 3]: (v0, v1) and (v2, v3) are two Box-Muller pairs in Float32,
 *                      u = (v + 0.5) 2^-32, radius sqrt(-2 log u_a), angle 2 pi u_b; cos -> the even, sin -> the odd coordinate;
 *   41 (chi^2)         Marsaglia-Tsang rounds t = 0 .. 7 in Float64: block 2t the proposal's normal (53-bit Box-Muller, cos), block 2t + 1
 *                      its uniform; block 63 the uniform of the shape < 1 boost.  After 8 rejections the last positive proposal is
 *                      accepted: a round rejects with probability < 0.05, so the law's total variation from Gamma is below 0.05^8 < 4e-11;
 *   42 (multinomial)   block b -> trials 2b (r0 = v0, r1 = v1) and 2b + 1 (r0 = v2, r1 = v3).
 * The value of sample i therefore depends on (seed, i, its cluster, the model) alone: not on n, on the first index of a call, on how a
 * draw is cut into calls, or on the ctx.
 *
 * A call writes at most n_local (the ctx's capacity) samples: n > n_local is DPMM_EINVAL.  The ctx's points are neither read nor changed.
 */
#ifndef DPMM_HIP_SAMPLE_H
#define DPMM_HIP_SAMPLE_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* most trials per point of a sparse draw: one point's draws are sorted in LDS (4096 words) */
#define DPMM_SAMPLE_MAX_TRIALS_SPARSE 4096
/* most trials per point of a dense draw: the counts are exact in Float32 */
#define DPMM_SAMPLE_MAX_TRIALS_DENSE 16777216

/* NIW contexts.  m [K][D], A [K][D][D] row-major (upper triangular; what lies below the diagonal is ignored), df [K] > 0; host memory,
 * copied.  K in 1 .. DPMM_MAX_CLUSTERS. */
int dpmm_set_sampler_niw(dpmm_ctx *ctx, int K, const float *m, const float *A, const float *df);

/* Multinomial contexts.  thr [K][D] acceptance thresholds (accept bucket j when r1 < thr), alias [K][D] in [0, D); host memory, copied. */
int dpmm_set_sampler_mult(dpmm_ctx *ctx, int K, const uint32_t *thr, const int32_t *alias);

typedef struct {
    int64_t        i0;             /* global index of the call's first sample                                              */
    int64_t        n;              /* samples of this call, 0 <= n <= n_local                                              */
    const int64_t *cluster_start;  /* [K + 1] host memory, non-decreasing global indices; [i0, i0 + n) lies inside them    */
    uint64_t       seed;
    int64_t        trials;         /* Multinomial: trials per point (>= 1); NIW: must be 0                                 */
    /* dense output (device memory): sample i0 + j at x + j * ld, ld >= D floats */
    float         *x;
    int64_t        ld;
    int64_t       *labels;         /* [n] 1-based cluster of every sample, device memory; may be NULL                      */
    /* sparse output (Multinomial, D <= DPMM_MAX_DIM_MULT_SPARSE, trials <= DPMM_SAMPLE_MAX_TRIALS_SPARSE; x must be NULL).
     * First call: colptr set, rowval == nzval == NULL: colptr[j] = nnz0 + entries of the samples before j (n + 1 offsets) and
     * *nnz_out = the entries of the call's samples.  Second call, same request with rowval / nzval set (colptr as the first call
     * left it, both arrays addressed by its ABSOLUTE offsets): row indices strictly increasing inside a column, no stored zero. */
    int64_t       *colptr;         /* [n + 1] device memory                                                                */
    int64_t        nnz0;           /* offset of the call's first entry                                                     */
    int64_t       *rowval;         /* device memory, Int64 like the offsets: what dpmm_upload_points_csc_device reads      */
    float         *nzval;
    int64_t        nnz_extent;     /* entries behind rowval / nzval (second call)                                          */
    int64_t       *nnz_out;        /* host memory (first call)                                                             */
} dpmm_sample_request;

/* Every device address is checked as dpmm_hip_tensor.h describes before anything is launched (DPMM_EINVAL, the message names the
 * argument).  Before dpmm_set_sampler_*: DPMM_ESTATE.  n == 0: DPMM_OK.  Returns after the ctx stream has been synchronised. */
int dpmm_sample_points_device(dpmm_ctx *ctx, const dpmm_sample_request *req);

#ifdef __cplusplus
}
#endif
#endif
