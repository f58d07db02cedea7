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
 *   incomplete   one of its D features is not finite (a point that DPMM_OPT_SCORE_MISSING marginalised: it is labelled, but without
 *                DPMM_OPT_TYPICALITY_GAPS this call does not marginalise q -- see "Points with gaps"); else
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
 * Points with gaps (DPMM_OPT_TYPICALITY_GAPS = 1, in a call that marginalises; the default is 0 and launches nothing new).  A point that
 * dpmm_hip_missing.h MARGINALISED (M its NaN features, r = |M| <= min(16, D - 1), O the others, D_o = D - r), that is not skipped and whose
 * features on O are all finite is scored under the marginal t_df(m_O, Sigma_OO) of its own cluster.  With z = x - m on O and 0 on M (Float32),
 * y = R z (Float32, the chain above), and in Float64 C = R[:, M], t = (C'C)^-1 C'y by Cholesky, res = y - C t:
 *   mahalanobis  q_o = z_O' P z_O = |res|^2, P = (Sigma_OO)^-1 = A_OO - A_OM A_MM^-1 A_MO, A = R'R: the Float64 residual norm, rounded once to
 *                Float32 -- the steps, in the same order, that gave the point its entry of the table for that cluster;
 *   tail         I_x(df / 2, D_o / 2) at x = df / (df + q_o): the routine above with D_o in the place of D, from the Float32 q_o, rounded once.
 * `incomplete` then counts only the points still not scored (an observed feature that is not finite); points over the cap stay skipped;
 * complete points keep their bits (the passes above run unchanged; a list-driven pass behind them overwrites the words of the listed points).
 * Error bound.  Pi = I - C (C'C)^-1 C' is an orthogonal projector: the Float32 error dy of y reaches res with norm at most |dy|, and
 * |res| <= |y|, so the Float32 part is that of a complete point with a_i taken over O: (3 D + 4) u a_i.  The Float64 part: A_MM = C'C is
 * formed, factored and solved in Float64 (u64 = 2^-53, kappa = cond(A_MM) >= 1, lambda its extreme eigenvalues).  To first order, in norms:
 *   forming    every entry of g = C'y and of A_MM is a Float64 inner product of length D, a chain of NT <= 4 terms and a butterfly of 6:
 *              |dg_a| <= (D + 6) u64 |c_a| |y| and |dA_ab| <= (D + 6) u64 |c_a| |c_b|, so |dg| <= (D + 6) u64 sqrt(r lambda_max) |y| and
 *              |dA| <= (D + 6) u64 tr A_MM <= r (D + 6) u64 |A_MM|;
 *   solving    the Cholesky solve is backward stable, (A_MM + E) t^ = g with |E| <= 4 r (3 r + 1) u64 |A_MM| (Higham, Accuracy and Stability
 *              of Numerical Algorithms, 10.4);
 *   into C t   |C A_MM^-1| = lambda_min^-1/2 and |t| <= lambda_min^-1/2 |C t| <= lambda_min^-1/2 |y|, so the two perturbations of A_MM move
 *              C t by at most kappa r (D + 12 r + 10) u64 |y| and dg by (D + 6) u64 sqrt(r kappa) |y|;
 *   res        r products and subtractions per element: (r + 1) u64 (|y| + sum_a |c_a| |t_a|) <= (r + 1) (1 + sqrt(r kappa)) u64 |y|;
 * with sqrt(r kappa) <= r kappa together |dres| <= r kappa (2 D + 14 r + 18) u64 |y|.  q_o = |res|^2 doubles that (|res| <= |y|), and its own
 * chain and butterfly add 11 u64 |y|^2 <= 12 r kappa u64 |y|^2: |dq_o| <= r kappa (2 D + 14 r + 24) 2^-52 |y|^2, and |y|^2 <= a_i.  Rounded up,
 *   F = 2 r (D + 8 r + 16) 2^-52 cond(A_MM),      |q_o - exact| <= (3 D + 4) u a_i + F a_i.
 * Out of scope: dpmm_batchstats_set_min_tail and the accumulators (a point with gaps stays incomplete there), more than 16 gaps, several
 * ranks, the Multinomial prior.
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
    int64_t *incomplete;     /* [1]   points not skipped with a feature that is not finite (with DPMM_OPT_TYPICALITY_GAPS:     */
                             /*       and not scored with gaps)                                       (host memory)    */
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

/* dpmm_set_option key: 0 (default): a point with gaps is incomplete, as described above.  1: in a call of dpmm_typicality_points[_device]
 * or dpmm_explain_points[_device] that marginalises (DPMM_OPT_SCORE_MISSING on), a marginalised point whose observed features are all
 * finite is SCORED by the marginal of its own cluster's predictive over the features it has ("Points with gaps" above); `incomplete`
 * then counts only the points still not scored.  Without DPMM_OPT_SCORE_MISSING the key changes nothing and launches nothing.  On a
 * Multinomial ctx setting it to 1 is DPMM_EINVAL.  dpmm_batchstats_set_min_tail and the accumulators of dpmm_hip_batchstats.h and
 * dpmm_hip_holdout.h do not look at it: a point with gaps has no x x' to add and stays incomplete there. */
#define DPMM_OPT_TYPICALITY_GAPS 35

#ifdef __cplusplus
}
#endif
#endif
