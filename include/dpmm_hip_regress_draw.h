/*
 * dpmm_hip_regress_draw.h -- optional companion of dpmm_hip_regress.h: DRAWS OF THE TARGETS (NIW only).  dpmm_regress_points summarises the
 * law of the targets given the given features by a mean and a standard deviation per target; that law is a mixture with one Student-t
 * per cluster the point could belong to, with several modes as soon as two clusters share the given features.  dpmm_regress_draw_points
 * DRAWS from it, as often as asked: joint intervals, quantiles, P(target a > target b), synthetic completions all follow from the draws.
 * Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_regress_points needs -- the points, dpmm_set_predictive_niw, dpmm_set_regression -- then
 * dpmm_set_regression_factor.
 *
 * The law, in the notation of dpmm_hip_regress.h (the ctx serves the marginal model over the D_o given features; cluster k has B_k, c_k,
 * h_k, df_k).  One more table: with A the precision of cluster k's joint predictive and A_MM = L L' its block over the targets,
 * W_k = (L^-1)', D_t x D_t upper triangular, W_k W_k' = (A_MM)^-1.  Draw j of point i, for a point that TAKES PART (the rule of
 * dpmm_regress_points):
 *   1. component   k ~ p_ik, p_ik = e_k / S of dpmm_hip_score.h (Float32): the cumulative sums c_k = p_0 + .. + p_k over the clusters of
 *                  positive probability are formed in Float64 in cluster order, and k is the first such cluster with u < c_k, u one 53-bit
 *                  uniform; if rounding leaves none, the last cluster of positive probability.
 *   2. scale       q = max(0, df_k expm1(2 (h_k - parr[k][i]) / (df_k + D_o))), recovered from the table entry as dpmm_regress_points
 *                  does; g ~ chi^2(df_k + D_o); s = (float) sqrt((df_k + q) / g), Float64 up to that single rounding.
 *   3. values      x_M = c_k + B_k x_i + W_k (s n),  n ~ N(0, I) of D_t Float32 Box-Muller normals, s n one Float32 product per
 *                  coordinate.  The right-hand side is ONE Float32 fused-multiply-add chain per target on the matrix pipe
 *                  (v_mfma_f32_32x32x2_f32): it starts from c_kd, runs over the given features in increasing e, then over the normal
 *                  coordinates in increasing a; products with structural zeros of W_k (a below the first target of the block of 32 targets
 *                  d lies in) are left out.  Cov = s^2 W W' -- the conditional t_{df + D_o}(c_k + B_k x, (df + q) / (df + D_o) (A_MM)^-1).
 *                  No df + D_o > 2 condition: the law exists without a variance.
 * A point that takes no part gets NaN in every draw and component -1; `skipped` counts it once per call, not once per draw.
 *
 * THE KEYING -- this paragraph is the contract.  Every random word is Philox4x32-10 with key = seed and counter = (global point index
 * i0 + i as two 32-bit words, block, stream), the generator of dpmm_hip_sample.h.  Draw j uses the blocks 64 j + b of three streams:
 *   stream 46, component   b = 0: u = (((v0 << 32 | v1) >> 11) + 0.5) 2^-53;
 *   stream 47, normals     b = 0 .. 63: block b gives the coordinates 4b .. 4b + 3 of n -- coordinate a belongs to target a -- as (cos, sin)
 *                          of two Float32 Box-Muller pairs (v0, v1), (v2, v3) with the 32-bit uniforms (v + 0.5) 2^-32, as
 *                          dpmm_hip_impute.h forms them; DPMM_REGRESS_MAX_TARGETS = 256 is exactly 64 blocks;
 *   stream 48, chi^2       the sampler's Marsaglia-Tsang draw with its block pattern from block 64 j on.
 * A value depends on (seed, global index, draw index, the point, the model) ALONE: not on the capacity of the ctx, on
 * DPMM_OPT_SCORE_TABLE_MB, on how the points were cut into uploads, on how a set of draws is cut into calls by draw0 / ndraws, or on the
 * neighbours of a point in its tile.  No atomics on the outputs, one writer per word.
 *
 * Memory: dpmm_set_regression_factor allocates (never before) K (D_o + D_t) 32 ceil(D_t / 32) floats: cluster k's image is B_k' on top
 * of W_k', read in 128-byte lines.  The first dpmm_regress_draw_points allocates the components and scales of a batch of draws of one range
 * (16 MiB at most; one draw at least); the host variant stages at most 64 MiB of draws at a time (one draw at least).  The score table is
 * evaluated ONCE per range of points for all ndraws draws.
 */
#ifndef DPMM_HIP_REGRESS_DRAW_H
#define DPMM_HIP_REGRESS_DRAW_H

#include "dpmm_hip_regress.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Draw indices lie in [0, DPMM_REGRESS_MAX_DRAWS): 64 blocks each in the 32-bit block number. */
#define DPMM_REGRESS_MAX_DRAWS 67108864

/* W: host Float64 [K][D_t][D_t], upper triangular (the entries below the diagonal are not read), for the tables of dpmm_set_regression
 * in force; rounded to Float32 once.  Without dpmm_set_regression in force: DPMM_ESTATE.  A null W, a Multinomial ctx or
 * D_o + D_t > 256 (the widest joint model): DPMM_EINVAL.  Whatever invalidates the regression tables -- a later dpmm_set_predictive_*,
 * a later dpmm_set_regression -- invalidates the factor with them. */
int dpmm_set_regression_factor(dpmm_ctx *ctx, const double *W);

/* The draws draw0 .. draw0 + ndraws - 1 of the ctx's points.  Element (j - draw0, i, d) is written at
 *     out[(j - draw0) * draw_stride + i * ld + d],   0 <= d < w = min(ld, draw_stride),
 * columns [D_t, w) as 0.  The two layouts of dpmm_impute_draw_points are served, everything else is DPMM_EINVAL:
 *     stacked       ld >= D_t and draw_stride >= n_local * ld;
 *     interleaved   draw_stride >= D_t and ndraws * draw_stride <= ld (floats of the row behind ndraws * draw_stride are not touched).
 * comp: null, or Int32 [ndraws][n_local]: the 0-based drawn cluster, -1 for a point that takes no part.
 * seed: the Philox key.  i0 >= 0: the global index of the ctx's first point.  draw0 >= 0, ndraws >= 1, draw0 + ndraws <= DPMM_REGRESS_MAX_DRAWS.
 * skipped: null, or one word for the number of POINTS that take no part.  Errors as dpmm_regress_points; without
 * dpmm_set_regression_factor in force: DPMM_ESTATE.  Both calls return after the ctx stream has been synchronised. */
int dpmm_regress_draw_points(dpmm_ctx *ctx, float *out, int64_t ld, int64_t draw_stride, int32_t *comp, uint64_t seed, int64_t i0,
                             int64_t draw0, int64_t ndraws, int64_t *skipped);                /* host memory   */

/* d_out and d_comp are checked as dpmm_hip_tensor.h describes before anything is launched: DPMM_EINVAL, the message names the argument.
 * skipped is host memory. */
int dpmm_regress_draw_points_device(dpmm_ctx *ctx, float *d_out, int64_t ld, int64_t draw_stride, int32_t *d_comp, uint64_t seed, int64_t i0,
                                    int64_t draw0, int64_t ndraws, int64_t *skipped);         /* device memory */

#ifdef __cplusplus
}
#endif
#endif
