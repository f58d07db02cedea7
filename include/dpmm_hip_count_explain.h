/*
 * dpmm_hip_count_explain.h -- optional companion of dpmm_hip_score.h: WHICH FEATURES PUT A COUNT POINT OUT (Multinomial only).  For every
 * point of the ctx: the `top` features whose count deviates most from what the point's own cluster expects, with their counts,
 * expectations, signed deviance residuals and exact binomial tails.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_score_points needs -- the points (any upload call, any of the three count stores: the Float32 matrix, the byte
 * copy, sparse columns) and dpmm_set_predictive_mult -- then dpmm_set_count_explain.
 *
 * Definitions.  For point i: k is the label dpmm_score_points gives; t the Float64 total of the store's values of the point (lane l of a
 * wave adds entries l, l + 64, .. in order, a fixed butterfly joins the lanes: a function of the point alone, exact for integer data);
 * theta = theta_kd = alpha'_kd / sum_d alpha'_kd, the plug-in predictive dpmm_score_points scores and dpmm_sample_points draws from, formed
 * in Float64 by the caller; x = x_id the store's value (0 for a feature a sparse column does not hold).  Under that predictive
 * x ~ Binomial(t, theta).  The binomial deviance of feature d is
 *     g_d = 2 [ T1 + T2 ],   T1 = x (log x - log t - log theta),   T2 = (t - x)(log(t - x) - log t - log1p(-theta)),
 * a term whose factor x or t - x is 0 being exactly 0; it is evaluated in Float64 from the caller's Float64 tables of log theta and
 * log1p(-theta).  A feature with x = 0 has g_d = -2 t log1p(-theta): one product, no logarithm -- the same bits as the general formula.
 *     residual     = sign(x - t theta) sqrt(g_d), rounded to Float32 once;
 *     expected     = t theta, Float32;      count = x, Float32;
 *     feature_tail = the exact one-sided binomial tail on the side of the deviation, Float64 rounded to Float32 once:
 *                    over  (x > t theta):  P(X >= x) = I_theta(x, t - x + 1)        (x = t: theta^t),
 *                    under (x < t theta):  P(X <= x) = I_{1-theta}(t - x, x + 1)    (x = 0: exp(t log1p(-theta))),
 *                    x = t theta: 1.
 * I is the regularised incomplete beta function.  The side is read off u = log x - log t - log theta, the factor of T1: over for u > 0,
 * under for u < 0 (x = 0: under), and x and t theta are taken as EQUAL when |u| <= 2^-40: residual 0, tail 1, a candidate of neither
 * one-sided ranking.  This band is an addition to the plain definition "x = t theta": theta reaches the device as a logarithm, u carries
 * a rounding error of a few 2^-53 of the logarithms' size, and an exact comparison would make the class of a point at its expectation an
 * accident of rounding; inside the band the deviance is below 2^-79 x, far below its own rounding error.  For expected and the tail,
 * theta is formed again as exp(log theta) or -expm1(log1p(-theta)), whichever loses nothing.  For values that are no integers the same
 * formulas hold as the continuous extension; they are then no probability statement.
 *
 * Ranking.  The deviance, not a Pearson z-score: for sparse counts a z-score puts every rare feature that occurs once (theta = 1e-6, t = 100,
 * x = 1: z = 100, tail 1e-4) above a common feature at four times its expected count, whose tail can be 1e-14; exp(-g / 2) is the
 * Chernoff bound of the binomial tail, so the deviance follows the tail.  features[i][0 .. top) are the candidates of largest |residual|
 * AS RETURNED IN FLOAT32, largest first, ties to the lower feature index, 0-based; slots behind the candidates hold -1 / NaN.  The
 * candidates are all D features (DPMM_COUNT_EXPLAIN_BOTH), those with x > t theta (_OVER) or those with x < t theta (_UNDER).  Given the
 * computed values the answer is unique.
 *
 * Classes.  A point whose row of the table has a NaN or no finite entry is SKIPPED (the rule of dpmm_hip_rank.h); its total is NaN.  A point
 * that is not skipped but has a value that is not finite or is negative, or t = 0 (an empty point), is INCOMPLETE.  Both have -1 / NaN
 * throughout and are counted.  labels holds the label of every point, as dpmm_score_points writes it.
 *
 * Error bounds (u = 2^-53; g*, r*, tail* the exact values from the same x, t and the Float64 theta; A1 = x (|log x| + |log t| + |log theta|),
 * A2 = (t - x)(|log(t - x)| + |log t| + |log1p(-theta)|), the sizes of what cancels inside T1 and T2 and, next to x = t theta, between them).
 * A bound in |T1| + |T2| alone, the obvious form, does not hold: the three logarithms of a term cancel INSIDE it (T1 is small when x is
 * near t theta although log x, log t and log theta are not), so the sizes of the logarithms, not of the terms, carry the error.
 * Per term: two logarithms of the maths library (2 u of their size each, the library's bound), the table entry (2 u: the caller's logarithm
 * and its rounding), two subtractions and one product (u each); then the sum and the doubling.  Counted generously
 *     |g - g*| <= 16 u (A1 + A2),
 *     |residual - r*| <= 2^-24 |r*| (1 + 2^-20) + 16 u (A1 + A2) / (2 |r*|):
 * the square root halves a relative error, its own rounding is u, and Float32 rounds once.  Where the second term is not small against
 * |r*| -- next to x = t theta -- the statement to test is the one on g.  The tail is held to the contract of dpmm_hip_typicality.h:
 * relatively 2^-20 on tails in [1e-30, 1]; below 1e-30 finite, non-negative and at most 1e-30 (1 + 2^-20).  Totals above 1e7 are outside
 * the contract (the continued fraction needs O(sqrt t) trips and is cut at 20000).
 *
 * No atomics on the outputs, one writer per word and launch (residual holds |residual| between the two kernels of a range): the bits
 * do not depend on the capacity of the ctx, on how the points were cut into uploads or on DPMM_OPT_SCORE_TABLE_MB, and for integer data
 * not on which of the three stores holds it (given equal labels).
 *
 * Memory: the two Float64 tables and the Int32 order, (16 K + 4 K) D bytes -- 20 MiB at K = 32, D = 20000; 1.25 GiB at K = 1024,
 * D = 65536 -- and, per point of a range, the total and the label the second kernel reads (8 + 4 bytes) and two counter words per 32
 * points belong to the ctx; allocated by dpmm_set_count_explain and the first dpmm_count_explain_points (never before), freed by
 * dpmm_destroy.  A host call stages its outputs on the device, 20 top + 16 bytes per point of a range.  Nothing grows with n D or n K.  The score table is evaluated range by range inside DPMM_OPT_SCORE_TABLE_MB, as
 * dpmm_score_points does.
 */
#ifndef DPMM_HIP_COUNT_EXPLAIN_H
#define DPMM_HIP_COUNT_EXPLAIN_H

#include "dpmm_hip_score.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_COUNT_EXPLAIN_MAX_TOP DPMM_SCORE_MAX_TOP
#define DPMM_COUNT_EXPLAIN_BOTH 0
#define DPMM_COUNT_EXPLAIN_OVER 1
#define DPMM_COUNT_EXPLAIN_UNDER 2

/* log_theta, log1m_theta: host Float64 [K][D], log theta_kd and log1p(-theta_kd) for the K clusters of the predictive set in force.  order:
 * host Int32 [K][D], for every cluster a permutation of 0 .. D - 1 along which log1m_theta does not decrease (theta does not increase), equal
 * values in increasing index order; anything else is DPMM_EINVAL.  A null table, a log_theta above 0, a log1m_theta above 0 or a NaN in
 * either, or an NIW ctx: DPMM_EINVAL.  Before dpmm_set_predictive_mult: DPMM_ESTATE.  Tables that cannot be allocated: DPMM_EHIP.  A later
 * dpmm_set_predictive_* invalidates the tables: the calls below return DPMM_ESTATE until they are set again. */
int dpmm_set_count_explain(dpmm_ctx *ctx, const double *log_theta, const double *log1m_theta, const int32_t *order);

typedef struct {
    int top;              /* 1 <= top <= min(D, DPMM_COUNT_EXPLAIN_MAX_TOP) */
    int side;             /* DPMM_COUNT_EXPLAIN_BOTH | _OVER | _UNDER */
    int64_t ld;           /* words between two rows of the five arrays below, ld >= top; columns [top, ld) are written as 0 */
    int32_t *features;    /* [n_local][ld] */
    float *count;         /* [n_local][ld] */
    float *expected;      /* [n_local][ld] */
    float *residual;      /* [n_local][ld] */
    float *feature_tail;  /* [n_local][ld] */
    int64_t *labels;      /* null, or [n_local] the 1-based labels dpmm_score_points gives (the same rule on the same row) */
    double *total;        /* null, or [n_local] t_i; NaN for a skipped point */
    int64_t *skipped;     /* null, or one word of HOST memory: the skipped points */
    int64_t *incomplete;  /* null, or one word of HOST memory: the incomplete points */
} dpmm_count_explain_out;

/* The layout of dpmm_recommend_points, pitched by ld.  Every refusal comes before any launch: an NIW ctx, top or side out of range,
 * ld < top, a null among the five arrays: DPMM_EINVAL; without dpmm_set_count_explain in force: DPMM_ESTATE.  Both calls return after the
 * ctx stream has been synchronised. */
int dpmm_count_explain_points(dpmm_ctx *ctx, const dpmm_count_explain_out *out);             /* the arrays are host memory   */

/* The arrays are checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned, the whole extent inside its
 * allocation) before anything is launched: DPMM_EINVAL, the message names the argument. */
int dpmm_count_explain_points_device(dpmm_ctx *ctx, const dpmm_count_explain_out *out);      /* the arrays are device memory */

#ifdef __cplusplus
}
#endif
#endif
