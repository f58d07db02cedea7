/*
 * dpmm_hip_regress.h -- optional companion of dpmm_hip_score.h: MIXTURE REGRESSION (NIW only).  The ctx serves the model restricted to the
 * GIVEN features (its D is D_o); the caller hands it per-cluster regression tables onto D_t TARGET features, and dpmm_regress_points
 * returns, for every point of the ctx, the mixture of the clusters' conditional means and -- if asked -- the standard deviation of the
 * mixture of their conditional laws.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_score_points needs -- the points (any upload call) and dpmm_set_predictive_niw -- then dpmm_set_regression.
 *
 * Definitions.  Cluster k of the ctx has the predictive t_df(m, Sigma) over the given features and the table entry
 *     parr[k][i] = h_k - (df_k + D_o) / 2 log1p(q_ik / df_k),      q_ik = |R_k (x_i - m_k)|^2,
 * h_k the x-independent constant (log w_k included).  The caller's tables say E[x_M | x_O = x, k] = c_k + B_k x and
 * Var[x_Md | x_O = x, k] = s_ik V_kd with s_ik = (df_k + q_ik) / (df_k + D_o - 2).  With p_ik = e_k / S of dpmm_hip_score.h (Float32, the
 * bits `probs` holds) and mu_ikd = c_kd + sum_e B_kde x_ie:
 *     mean[i][d] = sum_k p_ik mu_ikd
 *     std[i][d]  = sqrt(max(0, sum_k p_ik (s_ik V_kd + mu_ikd^2) - (sum_k p_ik mu_ikd)^2))
 *     s_ik from q_ik = max(0, df_k expm1(2 (h_k - parr[k][i]) / (df_k + D_o))): recovered from the table entry the range holds.
 * A point TAKES PART unless its row of the table has a NaN or no finite entry (the rule of dpmm_hip_rank.h) or one of its features is not
 * finite; the rows of mean and std of every other point are NaN, and `skipped` counts them.
 *
 * What is rounded where.  B, c and V are rounded to Float32 once, by dpmm_set_regression; h and df stay Float64.  mu_ikd is ONE Float32
 * chain on the matrix pipe (v_mfma_f32_32x32x2_f32): it starts from c_kd and adds the products B_kde x_ie in increasing e, each step one
 * fused multiply-add.  s_ik, the products with p_ik and both sums over k (increasing k, clusters with p_ik == 0 left out -- their terms
 * are exact zeros) are Float64; the difference under the root is formed in Float64 from the UNROUNDED sums; mean and std are rounded to
 * Float32 once.  No atomics on the outputs, one writer per word: the bits do not depend on the capacity of the ctx, on how the points
 * were cut into uploads or on DPMM_OPT_SCORE_TABLE_MB.
 *
 * The bound (u = 2^-24; "exact" = the Float64 evaluation of the definitions from the returned Float32 p_ik, the Float64 tables and the
 * Float32 points).  Let a_ikd = |c_kd| + sum_e |B_kde| |x_ie|.  The roundings of c and B (one u), the D_o steps of the chain (one u each),
 * the Float64 sums (below u in all) and the final rounding (one u) give, for a point that takes part,
 *     |mean - exact| <= (D_o + 4) u sum_k p_ik a_ikd.
 * For the variance let d_ik = (D_o + 3) u a_ikd bound the error of mu_ikd, m = sum_k p_ik mu_ikd, and t_ik bound the error of the table
 * entry parr[k][i] (tests/tools/predictive_ref.py derives one); dq / dparr = -2 (df + q) / (df + D_o), so the recovery moves s_ik by at
 * most s_ik expm1(2 t_ik / (df_k + D_o)).  Because sum_k p_ik 2 mu_ik d_ik - 2 m sum_k p_ik d_ik = 2 sum_k p_ik d_ik (mu_ik - m), the large
 * common part of the cluster means cancels in the bound as it does in the Float64 difference:
 *     |var - exact| <= sum_k p_ik [ s_ik V_kd (expm1(2 t_ik / (df_k + D_o)) + 3 u) + 2 d_ik |mu_ikd - m| + d_ik^2 ] + (sum_k p_ik d_ik)^2
 *                      + (K + 4) 2^-52 (sum_k p_ik (s_ik V_kd + mu_ikd^2) + m^2)
 * and |std - exact| <= min(sqrt(dv), dv / exact std) + 2 u exact std for a variance bound dv.
 *
 * Memory: the Float32 tables ([K][D_o][32 ceil(D_t / 32)] + 2 [K][32 ceil(D_t / 32)] floats, 2 K doubles) and one counter word per 32
 * points of a range belong to the ctx; allocated by dpmm_set_regression and the first dpmm_regress_points (never before), freed by
 * dpmm_destroy.  The score table is evaluated range by range inside DPMM_OPT_SCORE_TABLE_MB, as dpmm_score_points does.
 */
#ifndef DPMM_HIP_REGRESS_H
#define DPMM_HIP_REGRESS_H

#include "dpmm_hip_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_REGRESS_MAX_TARGETS 256

/* Host Float64 arrays for the K clusters of the predictive set in force: B [K][D_t][D] (D the ctx's, the given features in the order of
 * the ctx's), c [K][D_t], V [K][D_t], h [K].  D_t outside 1..DPMM_REGRESS_MAX_TARGETS, a null array or a Multinomial ctx: DPMM_EINVAL.
 * Before dpmm_set_predictive_niw: DPMM_ESTATE.  A later dpmm_set_predictive_* invalidates the tables: the calls below return DPMM_ESTATE
 * until they are set again. */
int dpmm_set_regression(dpmm_ctx *ctx, int D_t, const double *B, const double *c, const double *V, const double *h);

/* mean, std: [n_local][ld] Float32, ld >= D_t, columns [D_t, ld) written as 0 -- the layout of dpmm_impute_points; std may be NULL.
 * labels: null, or [n_local] the 1-based labels dpmm_score_points gives (the same pass over the row).  skipped: null, or one word for the
 * number of points that take no part.  Without dpmm_set_regression in force: DPMM_ESTATE; a Multinomial ctx: DPMM_EINVAL; std asked for
 * while a cluster has df + D <= 2 (no variance): DPMM_EINVAL.  Both calls return after the ctx stream has been synchronised. */
int dpmm_regress_points(dpmm_ctx *ctx, float *mean, float *std, int64_t ld, int64_t *labels, int64_t *skipped);                 /* host memory   */

/* d_mean, d_std and d_labels are checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned, the whole extent
 * inside its allocation) before anything is launched: DPMM_EINVAL, the message names the argument.  skipped is host memory. */
int dpmm_regress_points_device(dpmm_ctx *ctx, float *d_mean, float *d_std, int64_t ld, int64_t *d_labels, int64_t *skipped);    /* device memory */

#ifdef __cplusplus
}
#endif
#endif
