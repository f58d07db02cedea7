/*
 * dpmm_hip_typicality.h -- optional companion of dpmm_hip.h: a calibrated outlier score for every point under the NIW model the ctx
 * serves.  A log-density (dpmm_hip_score.h) changes its scale with D, with a cluster's volume, with the mixture weights and with every
 * update of the model; the tail probability of the point's squared Mahalanobis distance under its own cluster's Student-t predictive
 * does not: it is uniform on (0, 1) for points that belong to the cluster.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: the points (any dense upload call) and dpmm_set_predictive_niw(K, m, R, logdet, df, w).
 *
 * Definitions.  parr[k][i] and labels are exactly those of dpmm_hip_score.h, formed by the same device code; under
 * DPMM_OPT_SCORE_MISSING the marginal entries of dpmm_hip_missing.h are used.  With M = max_k parr[k][i] over the entries that are not
 * NaN, every point is in exactly one class:
 *   skipped      a NaN in its row of parr, or M not finite (the rule of dpmm_hip_overlap.h and dpmm_hip_batchstats.h); else
 *   incomplete   one of its D features is not finite (a point that DPMM_OPT_SCORE_MISSING marginalised: it is labelled, but this call
 *                does not marginalise q); else
 *   scored.
 * For a scored point, with k = labels[i] - 1 and x_i, m_k, R_k as the ctx holds them (Float32; x_i after the projection if the ctx has
 * one; R_k upper triangular, R_k' R_k = Sigma_k^-1 of the predictive t_df(m_k, Sigma_k)):
 *   mahalanobis  q_i = |R_k (x_i - m_k)|^2 in Float32: z = x_i - m_k, then y_r = sum_{c >= r} R_rc z_c as a chain of FMAs in increasing c,
 *                then the sum of the squares (an FMA chain over rows r, r + 64, .., then a butterfly over 64 partial sums);
 *   tail         P(Q >= q_i) for Q / D ~ F(D, df_k), that is I_x(df_k / 2, D / 2) at x = df_k / (df_k + q_i), the regularised incomplete
 *                beta function, evaluated in Float64 from the Float32 values q_i and df_k and rounded once.  q_i == 0 gives exactly 1;
 *                a result below the smallest normal Float32 may come back as 0.
 * Skipped and incomplete points get mahalanobis = tail = NaN; labels is written for every point.
 *
 * Error bounds.  u = 2^-24.  With a_i = sum_r (sum_c |R_rc| |z_c|)^2, z exact: every y_r carries at most gamma(D + 1) sum_c |R_rc| |z_c|
 * (the rounding of z included), the sum of squares adds gamma(D), together |q_i - exact| <= (3 D + 4) u a_i.  The tail: the continued
 * fraction (modified Lentz) is run on the side where it converges, x < (a + 1) / (a + b + 2), else on the complement, until a factor
 * lies within 2.5e-16 of 1; the prefactor exp(a log x + b log(1 - x) - log B(a, b)) takes log x and log(1 - x) from q and df without
 * cancellation and, for a >= 32, log B(a, b) from the Stirling series of lgamma(a + b) - lgamma(a), whose terms are of size b log a, not
 * a log a.  Relative to I_x of the same Float32 (q_i, df_k) the result is within 1e-9 before the one rounding to Float32 (6e-8)
 * wherever the tail is at least 1e-30.
 *
 * Determinism.  q_i and tail_i are functions of the point and its cluster alone: one writer per point, no floating-point atomics, the
 * same bits whatever the cut into uploads or the budget DPMM_OPT_SCORE_TABLE_MB.
 *
 * Limits: the NIW prior, every D it takes.  The Multinomial predictive has no closed-form tail: DPMM_EINVAL.
 *
 * Memory: the score table of dpmm_hip_score.h, the transposed factors of dpmm_hip_missing.h (K * D * 64 ceil(D / 64) floats), 8 bytes per
 * point of one range of the table, and for the host variant the staging of one range's outputs; all belong to the ctx.
 */
#ifndef DPMM_HIP_TYPICALITY_H
#define DPMM_HIP_TYPICALITY_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int64_t *labels;         /* [n]   1-based argmax, Julia rule: what dpmm_score_points writes                       */
    float   *mahalanobis;    /* [n]   q_i; NaN for a skipped or incomplete point                                      */
    float   *tail;           /* [n]   I_{df / (df + q_i)}(df / 2, D / 2); NaN for a skipped or incomplete point       */
    int64_t *skipped;        /* [1]   points with a NaN in their row of parr or M not finite         (host memory)    */
    int64_t *incomplete;     /* [1]   points not skipped with a feature that is not finite           (host memory)    */
} dpmm_typicality_out;       /* every pointer may be NULL; at least one must not be                                   */

/* n = n_local of the ctx.  Multinomial ctx, out == NULL or every pointer NULL: DPMM_EINVAL.  Before dpmm_set_predictive_niw:
 * DPMM_ESTATE.  n_local == 0: DPMM_OK (the counters are 0).  Both calls return after the ctx stream has been synchronised. */
int dpmm_typicality_points(dpmm_ctx *ctx, const dpmm_typicality_out *out);          /* host memory                        */

/* labels, mahalanobis and tail are checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned to its element,
 * the whole extent inside its allocation) before anything is launched: DPMM_EINVAL, the message names the argument. */
int dpmm_typicality_points_device(dpmm_ctx *ctx, const dpmm_typicality_out *out);   /* device memory; counters stay host  */

/* A calibrated floor for the accumulation of dpmm_hip_batchstats.h, set between dpmm_batchstats_begin and the first
 * dpmm_batchstats_accumulate (else DPMM_ESTATE).  use != 0: a point that is not skipped, whose features are all finite and whose tail
 * (the Float32 value above) is below min_tail is counted in held_out and adds nothing else -- beside the floor min_logdens of
 * dpmm_batchstats_begin, if that is in use: either one holds a point out.  min_tail outside (0, 1] or NaN: DPMM_EINVAL.  use == 0:
 * no floor (what dpmm_batchstats_begin leaves); nothing of this header runs then and the sums are what they were without it.  The
 * tails of one range (4 bytes per point) and the scratch above are allocated by the first accumulate that needs them. */
int dpmm_batchstats_set_min_tail(dpmm_ctx *ctx, int use, float min_tail);

#ifdef __cplusplus
}
#endif
#endif
