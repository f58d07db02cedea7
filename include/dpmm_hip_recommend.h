/*
 * dpmm_hip_recommend.h -- optional companion of dpmm_hip_score.h: TOP-m NEXT-COUNT PROBABILITIES (Multinomial only).  For every point of the
 * ctx: the m features the fitted mixture expects next, and their probabilities, among the features the point does not hold yet.
 * Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_score_points needs -- the points (any upload call, any of the three count stores: the Float32 matrix, the byte
 * copy, sparse columns) and dpmm_set_predictive_mult -- then dpmm_set_recommend.
 *
 * Definitions.  Under cluster k the posterior predictive of one more count is theta_kd = alpha'_kd / sum_d alpha'_kd; the caller forms it
 * in Float64 and hands it over.  With p_ik = e_k / S of dpmm_hip_score.h (Float32, the bits `probs` holds; never written to memory here)
 *     r_id = sum_k p_ik theta_kd.
 * Feature d is SEEN by point i when the store's value for it is not 0: x_id != 0 in the Float32 matrix and the byte copy, an entry kept
 * with a value that is not 0 in the sparse columns.  The CANDIDATES of a point are its unseen features (exclude_seen != 0) or all D
 * features (exclude_seen == 0).  features[i][0 .. m) are the m candidates of largest r_id, largest first, ties to the lower feature index,
 * 0-based; prob[i][j] is r of features[i][j].  Given the computed Float32 values the answer is unique.  A point with fewer than m
 * candidates has -1 / NaN in the remaining slots.  A point whose row of the table has a NaN or no finite entry (the rule of
 * dpmm_hip_rank.h) takes no part: -1 / NaN throughout, counted in `skipped`.
 *
 * What is rounded where.  theta is rounded to Float32 once, by dpmm_set_recommend.  r_id is ONE Float32 chain on the matrix pipe
 * (v_mfma_f32_32x32x2_f32): it starts from 0 and takes the clusters in increasing k, two per instruction, K padded to even with zeros.  A
 * pair of clusters whose p is exactly 0 for every point of a tile of 32 points is left out: its terms are exact zeros, the bits do not
 * change.  No atomics on the outputs, one writer per word: the bits do not depend on the capacity of the ctx, on how the points were cut
 * into uploads or on DPMM_OPT_SCORE_TABLE_MB.
 *
 * The bound (u = 2^-24; "exact" = the Float64 evaluation of r_id from the returned Float32 p_ik and the Float64 theta).  Every term is
 * non-negative, theta is rounded once (one u), the chain has K steps (one u each, one more for the instruction's inner sum):
 *     |prob - exact| <= (K + 2) u exact.
 *
 * Memory: the Float32 image of theta, (K rounded up to even) x (D rounded up to a multiple of 32) floats -- 256 MiB at K = 1024,
 * D = 65536; 2.5 MB at K = 32, D = 20000 -- and one counter word per 32 points of a range belong to the ctx; allocated by
 * dpmm_set_recommend and the first dpmm_recommend_points (never before), freed by dpmm_destroy.  A host call stages its outputs on the
 * device, 8 m + 8 bytes per point of a range.  Nothing grows with n D or n K.  The score table is evaluated range by range inside
 * DPMM_OPT_SCORE_TABLE_MB, as dpmm_score_points does.
 */
#ifndef DPMM_HIP_RECOMMEND_H
#define DPMM_HIP_RECOMMEND_H

#include "dpmm_hip_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_RECOMMEND_MAX_TOP DPMM_SCORE_MAX_TOP

/* theta: host Float64 [K][D] for the K clusters of the predictive set in force, rounded to Float32 and stored as a padded image.  A null
 * table or an NIW ctx: DPMM_EINVAL.  Before dpmm_set_predictive_mult: DPMM_ESTATE.  A table that cannot be allocated: DPMM_EHIP.  A later
 * dpmm_set_predictive_* invalidates the table: the calls below return DPMM_ESTATE until it is set again. */
int dpmm_set_recommend(dpmm_ctx *ctx, const double *theta);

/* features: [n_local][ld] Int32, prob: [n_local][ld] Float32, ld >= m, columns [m, ld) written as 0 -- the layout of dpmm_regress_points;
 * 1 <= m <= min(D, DPMM_RECOMMEND_MAX_TOP).  labels: null, or [n_local] the 1-based labels dpmm_score_points gives (the same pass over the
 * row).  skipped: null, or one word for the number of points that take no part.  Every refusal comes before any launch: an NIW ctx, m out
 * of range, ld < m, a null features or prob: DPMM_EINVAL; without dpmm_set_recommend in force: DPMM_ESTATE.  Both calls return after the
 * ctx stream has been synchronised. */
int dpmm_recommend_points(dpmm_ctx *ctx, int m, int exclude_seen, int32_t *features, float *prob, int64_t ld, int64_t *labels,
                          int64_t *skipped);                                                                                     /* host memory   */

/* d_features, d_prob and d_labels are checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned, the whole extent
 * inside its allocation) before anything is launched: DPMM_EINVAL, the message names the argument.  skipped is host memory. */
int dpmm_recommend_points_device(dpmm_ctx *ctx, int m, int exclude_seen, int32_t *d_features, float *d_prob, int64_t ld, int64_t *d_labels,
                                 int64_t *skipped);                                                                              /* device memory */

#ifdef __cplusplus
}
#endif
#endif
