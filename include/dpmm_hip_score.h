/*
 * dpmm_hip_score.h -- optional companion of dpmm_hip.h: scoring new points with a fitted model at any n and K.  Mixture log-density,
 * the best m clusters with their probabilities, labels and the full probability matrix from ONE fused finish kernel, into host or
 * caller-owned device memory.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_predict_points needs -- the points (any upload call) and dpmm_set_predictive_niw / _mult.  `parr` below is the
 * table dpmm_predict returns: parr[k][i] = posterior predictive log-density of point i under cluster k + log w_k.
 *
 * Definitions (Float32 throughout, stated to the bit).  For point i let a_k = parr[k][i] with NaN replaced by -Inf, M = max_k a_k,
 * e_k = expf(a_k - M), S = the sum of e_k in increasing k.  Then
 *   labels   1-based argmax of parr[.][i] by Julia's rule (the first NaN wins, else the first maximum) -- what dpmm_predict_points writes;
 *   probs    e_k / S, row-major [n][K] -- bit-identical to dpmm_predict_points, NaN rows (M = +-Inf) included;
 *   logdens  M + logf(S); -Inf when M is -Inf;
 *   top_idx, top_prob   the m largest values of probs[i][.], ranked by the value written, ties to the lower index;
 *            top_prob[i][j] is bit-identical to probs[i][top_idx[i][j] - 1]; a row without a finite entry (all probabilities NaN)
 *            returns the indices 1..m and those NaNs.
 *
 * Bounded memory: the table is evaluated over ranges of whole tiles of the ctx's points, never more than DPMM_OPT_SCORE_TABLE_MB of it
 * at a time; table and staging buffers belong to the ctx (allocated on first use, grown when a call needs more, freed by dpmm_destroy):
 * a second call of the same shape allocates nothing.  No result depends on the budget.
 */
#ifndef DPMM_HIP_SCORE_H
#define DPMM_HIP_SCORE_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dpmm_set_option key: megabytes (2^20 bytes, fractions allowed) of the score table held at a time.  Default 128: a slab the finish
 * kernel's second pass finds in the 256 MiB last-level cache.  Anything below one tile's rows means one tile; a negative value restores
 * the default.  Multinomial contexts evaluate 3 rows per cluster (the sweep's row layout), all of which count. */
#define DPMM_OPT_SCORE_TABLE_MB 32

#define DPMM_SCORE_MAX_TOP 16

typedef struct {
    int64_t *labels;      /* [n]        1-based argmax, Julia rule (first NaN wins)          */
    float   *logdens;     /* [n]        log sum_k exp(parr[k][i])                            */
    int      m;           /* top-m width, 0 = none, 1 <= m <= min(K, 16)                     */
    int64_t *top_idx;     /* [n][m]     1-based cluster indices, best first                  */
    float   *top_prob;    /* [n][m]     their normalised probabilities                       */
    float   *probs;       /* [n][K]     the full matrix, as dpmm_predict_points writes it    */
} dpmm_score_out;         /* every pointer may be NULL; at least one must not be             */

/* n = n_local of the ctx.  m == 0 with top_idx or top_prob set, m > 0 with neither, m > min(K, 16), or every pointer NULL: DPMM_EINVAL.
 * Before dpmm_set_predictive_*: DPMM_ESTATE.  n_local == 0: DPMM_OK.  Both calls return after the ctx stream has been synchronised. */
int dpmm_score_points(dpmm_ctx *ctx, const dpmm_score_out *out);          /* host memory   */

/* Every non-null output is checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned to its element, the whole
 * extent inside its allocation) before anything is launched: DPMM_EINVAL, the message names the argument. */
int dpmm_score_points_device(dpmm_ctx *ctx, const dpmm_score_out *out);   /* device memory */

#ifdef __cplusplus
}
#endif
#endif
