/*
 * dpmm_hip_missing.h -- optional companion of dpmm_hip_score.h: points with MISSING features (NIW only).  A NaN feature is a missing
 * one: with DPMM_OPT_SCORE_MISSING on, such a point is scored by the marginal of every cluster's Student-t predictive over the features
 * it does have, and dpmm_impute_points fills the gaps with the mixture of the conditional means.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_score_points needs -- the points (any upload call that keeps NaN) and dpmm_set_predictive_niw.
 *
 * Definitions.  Cluster k's predictive is t_df(m, Sigma), Sigma^-1 = R'R, R upper triangular (the arguments of dpmm_set_predictive_niw).
 * A point has the missing set M = its NaN features, r = |M|, the observed set O, D_o = D - r.  +-Inf is a value, not a gap.
 *   MARGINALISED   1 <= r <= min(DPMM_SCORE_MAX_MISSING, D - 1);
 *   OVER THE CAP   r beyond that (r == D included): the point keeps the all-NaN row it has without the option.
 * For a marginalised point, with z = x - m on O and 0 on M (Float32), y = R z (Float32, as the table kernel), and in Float64
 * C = R[:, M], g = C'y, A = C'C (r x r, SPD), t = A^-1 g (by Cholesky), q_o = |y - C t|^2 (the explicit residual):
 *   parr[k][i] = lgamma((df + D_o) / 2) - lgamma(df / 2) - D_o / 2 log(df pi) - (logdet + logdet A) / 2 - (df + D_o) / 2 log1p(q_o / df) + log w_k
 *   E[x_M | x_O, k] = m_M - t
 * the value rounded to Float32 once.  Every consumer of the table sees these entries: labels, probabilities, top-m, log-density
 * (dpmm_hip_score.h) and exemplars (dpmm_hip_rank.h) follow with their own definitions unchanged.
 *
 * Memory: the list of a range's points with gaps, three counters and a transposed copy of the K factors ([K][D][64 ceil(D / 64)] Float32)
 * belong to the ctx; allocated by the first call that marginalises (never while the option is off and dpmm_impute_points is not called),
 * bounded by the range DPMM_OPT_SCORE_TABLE_MB sets, freed by dpmm_destroy.
 */
#ifndef DPMM_HIP_MISSING_H
#define DPMM_HIP_MISSING_H

#include "dpmm_hip_score.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dpmm_set_option key: 0 (default): a NaN feature makes the point's row of the table NaN, as ever.  1: dpmm_score_points[_device] and
 * dpmm_rank_accumulate marginalise, between the evaluation of every range of the table and its finish pass.  On a Multinomial ctx
 * setting it to 1 is DPMM_EINVAL. */
#define DPMM_OPT_SCORE_MISSING 33

#define DPMM_SCORE_MAX_MISSING 16

/* out[0] = marginalised, out[1] = over-the-cap points among the ctx's points that the last dpmm_score_points[_device],
 * dpmm_rank_accumulate or dpmm_impute_points[_device] evaluated; both 0 when that call ran with the option off (dpmm_impute_points
 * always counts) or returned before it evaluated anything (n_local == 0, an error).  Waits for the ctx stream. */
int dpmm_score_missing_counts(dpmm_ctx *ctx, int64_t out[2]);

/* The ctx's points as Float32 rows, out [n_local][ld], ld >= D, columns [D, ld) written as 0 -- the layout of dpmm_get_points_device --
 * with every NaN feature of a marginalised point replaced by sum_k p_k (m_M - t_k), p_k = e_k / S of dpmm_hip_score.h taken from the
 * marginal table (accumulated in Float64, rounded once).  Observed features, complete points and over-the-cap points are copied bit for
 * bit.  Works whether or not DPMM_OPT_SCORE_MISSING is set.  Before dpmm_set_predictive_niw: DPMM_ESTATE; a Multinomial ctx: DPMM_EINVAL.
 * Both calls return after the ctx stream has been synchronised. */
int dpmm_impute_points(dpmm_ctx *ctx, float *out, int64_t ld);                 /* host memory   */

/* d_out is checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned, the whole extent inside its allocation)
 * before anything is launched: DPMM_EINVAL, the message names the argument. */
int dpmm_impute_points_device(dpmm_ctx *ctx, float *d_out, int64_t ld);        /* device memory */

#ifdef __cplusplus
}
#endif
#endif
