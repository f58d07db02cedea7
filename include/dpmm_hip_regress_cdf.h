/*
 * dpmm_hip_regress_cdf.h -- optional companion of dpmm_hip_regress.h: the CONDITIONAL CDF AND QUANTILES of every target given the given
 * features (NIW only).  Where dpmm_regress_points returns a mean and a spread and dpmm_regress_draw_points draws, these calls return
 * calibrated probabilities: F_id(y), the probability under the fitted mixture that target d of point i lies below y, its complement, and
 * the y at which F_id reaches given levels.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_regress_points needs (points, dpmm_set_predictive_niw, dpmm_set_regression); the quantiles also
 * dpmm_set_regression_levels.  df + D <= 2 is no obstacle: a Student-t has a CDF for every df.
 *
 * Definitions (the symbols of dpmm_hip_regress.h: p_ik, mu_ikd = c_kd + sum_e B_kde x_ie, q_ik recovered from the table entry).  Given
 * x_O = x_i and cluster k, target d is Student-t with nu_k = df_k + D_o degrees of freedom, location mu_ikd and scale
 *     sigma_ikd^2 = (df_k + q_ik) / (df_k + D_o) V_kd
 * (the variance dpmm_regress_points uses without the factor nu / (nu - 2)).  With T_nu the CDF of t_nu and t = (y - mu_ikd) / sigma_ikd:
 *     cdf[i][d] = F_id(y_id) = sum_k p_ik T_nu_k(t_ikd)            sf[i][d] = sum_k p_ik (1 - T_nu_k(t_ikd))
 * Every component enters each sum from its side that does not cancel: with tail = I_{nu / (nu + t^2)}(nu / 2, 1 / 2) = P(|t_nu| > |t|), the
 * Float64 tail of dpmm_hip_typicality.h at D = 1, a component gives tail / 2 to the sum whose side t lies on (cdf for t < 0, sf for t > 0)
 * and 1 - tail / 2 to the other.  So sf = 1e-12 is returned as that, not as 0.  A NaN in y gives NaN in that entry alone; y = -Inf gives
 * cdf 0 and sf 1, y = +Inf cdf 1 and sf 0, exactly.  A point that takes no part (the rule of dpmm_hip_regress.h) has NaN rows and is
 * counted in `skipped`.
 *
 * Quantiles.  dpmm_set_regression_levels hands over L increasing levels in (0, 1) and z[k][q] = T_nu_k^-1(level_q) in Float64
 * (host/condition.py: student_t_ppf).  For (point, target, level): over the clusters with p_ik != 0, y_kq = mu_ikd + sigma_ikd z_kq; at
 * min_k y_kq every component CDF is <= level, at max_k y_kq every one is >= level, so the root of F_id = level lies between.  A point with
 * ONE such cluster gets y_kq itself, rounded once (level 1 / 2: z = 0, the bits of mu, those of `mean` -- but a zero is returned as
 * +0 whatever its sign: the values pass through the ordered integers, in which -0 and +0 are one).  Otherwise the bracket is widened
 * to Float32 values and a safeguarded solve runs over Float32 candidates: F (the cdf sum above) and the density
 * f = sum_k p_ik g_nu_k(t) / sigma_ikd, g the density of t_nu, in Float64 at the candidate; the bracket end on the candidate's side is
 * replaced; the next candidate is Newton's y - (F - level) / f (its Float32 neighbour on the far side if it rounds to y) when that lies
 * strictly inside and the step before made progress -- it halved the number of Float32 values in the bracket or |F - level|, or Newton
 * moves by one Float32 value at most (it has arrived; the neighbour closes the bracket) -- and the
 * arithmetic midpoint otherwise.  There are 48 candidates per root at most, a compile-time trip count; as soon as the number of Float32
 * values in the bracket exceeds 2^(candidates left - 1) only midpoints of the ORDERED Float32 values are taken, so the ends are adjacent
 * when the candidates run out (32 halvings suffice for any bracket); were they not, the midpoint would be returned.  The value returned is
 * the UPPER end: the smallest Float32 y of the bracket whose F(y) >= level.  It is a function of (the point, the model, the level) alone --
 * not of the capacity, the uploads, DPMM_OPT_SCORE_TABLE_MB, the order of the points or the other levels.  Monotonicity: F as evaluated is
 * non-decreasing in y up to its Float64 rounding, so the value is non-decreasing in the level; to make this hold BY CONSTRUCTION the
 * levels are solved in increasing order and a value is raised to that of the level before it.  That changes a value only if two levels
 * are closer than the rounding of F (about 2^-48).
 *
 * What is rounded where.  As dpmm_hip_regress.h: B, c, V Float32 once, mu the one Float32 chain of dpmm_regress_points (the same bits), h
 * and df Float64.  q, sigma, t, the tails and densities and both sums over k (increasing k, clusters with p_ik == 0 left out) are Float64;
 * cdf, sf and the quantiles are rounded to Float32 once.  y is Float32.  No atomics, one writer per word.
 *
 * The bounds (u = 2^-24; "exact" = the Float64 evaluation of the definitions from the returned Float32 p_ik, the Float64 tables, the
 * Float32 points and the Float32 y).  With a_ikd, d_ik = (D_o + 3) u a_ikd (the error of mu) and t_ik (the error of the table entry) of
 * dpmm_hip_regress.h: the recovery moves (df + q) by the factor 1 + r_ik, |r_ik| <= expm1(2 t_ik / (df_k + D_o)), the rounding of V and the
 * Float64 steps add 3 u, so sigma is off by the factor (1 + e)^(1/2), e_ik = r_ik + 3 u, and t by at most
 *     dt_ikd = d_ik / sigma_ikd + |t_ikd| (e_ik / 2) / (1 - e_ik).
 * A component's CDF moves by at most its density, at the point of [|t| - dt, |t|] nearest 0 (t_nu is unimodal), times dt.  The tail is
 * accurate to 2^-20 relative (dpmm_hip_typicality.h), and tail / 2 = h_ikd is the part of a component that was computed (1 - h is exact
 * to 2^-53).  The sums are of non-negative terms: (K + 4) 2^-52 relative; the final rounding u relative.  Hence for a point that takes part
 *     |cdf - exact| <= b_F(i, d) = sum_k p_ik [ g_nu_k(max(0, |t_ikd| - dt_ikd)) dt_ikd + 2^-20 h_ikd ] + ((K + 4) 2^-52 + u) exact + 2^-150
 * and the same for sf with its own exact value in the term before the last.  The last term is the final rounding where Float32 is
 * subnormal (below 2^-126; below 2^-150 a value is returned as 0).  Far in a tail every other term is small RELATIVE to the side that
 * does not cancel, so that side keeps its relative accuracy down to the end of the Float32 range.
 * Quantiles: the contract is in probability, where the problem is well conditioned even between two far modes.  For the returned y, with
 * y- its Float32 predecessor: F(y-) < level <= F(y) as evaluated, so
 *     |F_exact(y) - level| <= max(b_F at y, b_F at y-) + max(f_exact(y), f_exact(y-)) (y - y-)
 * the first term the error of the evaluated F, the second the step of F_exact between two neighbouring Float32 values (f_exact has one
 * mode per component; the maximum over the step is at an end unless a mode lies inside, which the first-order statement ignores).
 * A point with one cluster: y = mu + sigma z rounded, within d_ik + sigma |z| (e / 2) / (1 - e) + u |y| of exact, i.e. the same contract.
 *
 * Memory: dpmm_set_regression_levels allocates (K L + L + K) doubles on the device; the calls use the counter words of
 * dpmm_regress_points and, in the host variants, the staging block of dpmm_score_points (inputs and outputs of one range); freed by
 * dpmm_destroy.  The score table is evaluated range by range inside DPMM_OPT_SCORE_TABLE_MB.
 */
#ifndef DPMM_HIP_REGRESS_CDF_H
#define DPMM_HIP_REGRESS_CDF_H

#include "dpmm_hip_regress.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_REGRESS_MAX_LEVELS 16

/* y, cdf, sf: [n_local][ldy] / [n_local][ld] Float32, ldy, ld >= D_t, columns [D_t, ld) of cdf and sf written as 0 -- the layout of `mean`;
 * sf may be NULL.  labels, skipped: as dpmm_regress_points.  Without dpmm_set_regression in force: DPMM_ESTATE; a Multinomial ctx, a null
 * y or cdf, ldy or ld < D_t: DPMM_EINVAL.  Both calls return after the ctx stream has been synchronised. */
int dpmm_regress_cdf_points(dpmm_ctx *ctx, const float *y, int64_t ldy, float *cdf, float *sf, int64_t ld, int64_t *labels, int64_t *skipped);   /* host memory */

/* d_y, d_cdf, d_sf and d_labels are checked as dpmm_hip_tensor.h describes before anything is launched (DPMM_EINVAL, the message names the
 * argument).  skipped is host memory. */
int dpmm_regress_cdf_points_device(dpmm_ctx *ctx, const float *d_y, int64_t ldy, float *d_cdf, float *d_sf, int64_t ld, int64_t *d_labels,
                                   int64_t *skipped);                                                                                            /* device memory */

/* L levels, strictly increasing, inside (0, 1), and z [K][L] (host Float64) for the regression tables in force.  L outside
 * 1..DPMM_REGRESS_MAX_LEVELS, a level outside (0, 1) or not above the one before, a z that is not finite, a null array or a Multinomial
 * ctx: DPMM_EINVAL.  Without dpmm_set_regression in force: DPMM_ESTATE.  A later dpmm_set_predictive_* or dpmm_set_regression
 * invalidates the levels: dpmm_regress_quantile_points returns DPMM_ESTATE until they are set again. */
int dpmm_set_regression_levels(dpmm_ctx *ctx, int L, const double *levels, const double *z);

/* out: [n_local][L][ld] Float32, ld >= D_t, element (i, q, d) at out[(i * L + q) * ld + d], columns [D_t, ld) written as 0.  labels,
 * skipped: as above.  Without levels in force: DPMM_ESTATE. */
int dpmm_regress_quantile_points(dpmm_ctx *ctx, float *out, int64_t ld, int64_t *labels, int64_t *skipped);                  /* host memory   */
int dpmm_regress_quantile_points_device(dpmm_ctx *ctx, float *d_out, int64_t ld, int64_t *d_labels, int64_t *skipped);       /* device memory */

#ifdef __cplusplus
}
#endif
#endif
