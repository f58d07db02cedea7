/*
 * dpmm_hip_impute.h -- optional companion of dpmm_hip_missing.h: MULTIPLE IMPUTATION (NIW only).  dpmm_impute_points fills every gap with
 * one number, the mixture of the conditional means; dpmm_impute_draw_points DRAWS the missing features of every marginalised point from
 * p(x_M | x_O) under the fitted mixture, as often as asked: m completed copies of the data, to be analysed separately and pooled.
 * Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_impute_points needs -- the points (any upload call that keeps NaN) and dpmm_set_predictive_niw.
 *
 * The law, in the notation of dpmm_hip_missing.h (cluster k's predictive t_df(m, Sigma), Sigma^-1 = R'R; a marginalised point has the
 * missing set M, r = |M|, D_o = D - r, z, y = R z in Float32 and, in Float64, C = R[:, M], A = C'C = L L', t = A^-1 C'y, q_o = |y - C t|^2).
 * Draw j of point i:
 *   1. component   k ~ p_k, p_k = e_k / S of dpmm_hip_score.h taken from the marginal table (Float32, a NaN entry counting as probability
 *                  0): the cumulative sums c_k = p_0 + .. + p_k over the clusters of positive probability are formed in Float64 in cluster
 *                  order, and k is the first such cluster with u < c_k, u one 53-bit uniform; if rounding leaves none, the last cluster of
 *                  positive probability; if no cluster has one (an infinite observed feature makes the whole column NaN or -Inf), cluster 0,
 *                  and the values come out as non-finite as the point is.
 *   2. values      x_M | x_O, k ~ t_{df + D_o}(m_M - t, (df + q_o) / (df + D_o) A^-1), drawn as
 *                      x_M = (m_M - t) + sqrt((df + q_o) / g) w,    L'w = n,  n ~ N(0, I_r),  g ~ chi^2(df + D_o)
 *                  (Cov w = (L L')^-1 = A^-1).  Only the drawn cluster's system is solved.  The solve, the scale and the sum are Float64,
 *                  rounded to Float32 once; the normals are Float32.
 * Observed features, complete points and over-the-cap points (which keep their NaN) are copied bit for bit, as dpmm_impute_points does.
 *
 * THE KEYING -- this paragraph is the contract.  Every random word is Philox4x32-10 with key = seed and counter = (global point index
 * i0 + i as two 32-bit words, block, stream), the generator of dpmm_hip_sample.h.  Draw j uses the blocks 64 j + b of three streams:
 *   stream 43, component   b = 0: u = (((v0 << 32 | v1) >> 11) + 0.5) 2^-53;
 *   stream 44, normals     b = 0 .. 3: block b gives the coordinates 4b .. 4b + 3 of n -- coordinate a belongs to the a-th missing feature
 *                          in increasing feature order -- as (cos, sin) of two Float32 Box-Muller pairs (v0, v1), (v2, v3) with the 32-bit
 *                          uniforms (v + 0.5) 2^-32, as the NIW sampler forms them;
 *   stream 45, chi^2       the sampler's Marsaglia-Tsang draw with its block pattern: b = 2t and 2t + 1 for round t < 8, b = 63 for the
 *                          boost of a shape below 1.
 * A value depends on (seed, global index, draw index, the point, the model) ALONE: not on the capacity of the ctx, on
 * DPMM_OPT_SCORE_TABLE_MB, on how a set of draws is cut into calls by draw0 / ndraws, or on what else the ctx holds.  A later caller that
 * redraws between sweeps passes a fresh draw index, not a fresh seed.
 *
 * Memory: what dpmm_impute_points uses; the host variant stages at most 64 MiB of draws at a time (one draw at least).
 */
#ifndef DPMM_HIP_IMPUTE_H
#define DPMM_HIP_IMPUTE_H

#include "dpmm_hip_missing.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Draw indices lie in [0, DPMM_IMPUTE_MAX_DRAWS): 64 blocks each in the 32-bit block number. */
#define DPMM_IMPUTE_MAX_DRAWS 67108864

/* The draws draw0 .. draw0 + ndraws - 1 of the ctx's points.  Element (j - draw0, i, f) is written at
 *     out[(j - draw0) * draw_stride + i * ld + f],   0 <= f < w = min(ld, draw_stride),
 * columns [D, w) as 0.  Two layouts are served, everything else is DPMM_EINVAL:
 *     stacked       ld >= D and draw_stride >= n_local * ld: ndraws images of dpmm_impute_points' layout, one behind the other;
 *     interleaved   draw_stride >= D and ndraws * draw_stride <= ld: the draws of a point side by side in its row of ld floats (floats of
 *                   the row behind ndraws * draw_stride are not touched: another call's draws may live there).
 * comp: null, or Int32 [ndraws][n_local]: the 0-based drawn cluster of every marginalised point, -1 for every other point.
 * seed: the Philox key.  i0 >= 0: the global index of the ctx's first point.  draw0 >= 0, ndraws >= 1, draw0 + ndraws <= DPMM_IMPUTE_MAX_DRAWS.
 * The table is evaluated ONCE per range of points for all ndraws draws, and marginalised whether or not DPMM_OPT_SCORE_MISSING is set; the
 * call sets the counts of dpmm_score_missing_counts.  Errors as dpmm_impute_points: before dpmm_set_predictive_niw DPMM_ESTATE, a
 * Multinomial ctx DPMM_EINVAL.  Both calls return after the ctx stream has been synchronised. */
int dpmm_impute_draw_points(dpmm_ctx *ctx, float *out, int64_t ld, int64_t draw_stride, int32_t *comp, uint64_t seed, int64_t i0,
                            int64_t draw0, int64_t ndraws);                                   /* host memory   */

/* d_out and d_comp are checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned, the whole extent inside its
 * allocation) before anything is launched: DPMM_EINVAL, the message names the argument. */
int dpmm_impute_draw_points_device(dpmm_ctx *ctx, float *d_out, int64_t ld, int64_t draw_stride, int32_t *d_comp, uint64_t seed, int64_t i0,
                                   int64_t draw0, int64_t ndraws);                            /* device memory */

#ifdef __cplusplus
}
#endif
#endif
