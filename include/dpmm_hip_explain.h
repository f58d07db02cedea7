/*
 * dpmm_hip_explain.h -- optional companion of dpmm_hip.h and dpmm_hip_typicality.h: WHY a point is atypical of its cluster.  The tail of
 * dpmm_hip_typicality.h says that a point is far out; this header says which features put it there.  A per-feature marginal z-score
 * answers that badly -- in a correlated cluster a point can sit twelve conditional standard deviations out while every marginal looks
 * ordinary -- but under the point's own Student-t predictive the law of one feature given all the others is again a Student-t in closed
 * form, and everything it needs is what the typicality pass already forms.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: the points (any dense upload call) and dpmm_set_predictive_niw(K, m, R, logdet, df, w).
 *
 * Definitions.  labels, mahalanobis, tail, skipped, incomplete and the three classes of a point (skipped, incomplete, scored) are exactly
 * those of dpmm_hip_typicality.h, formed by the same device code: the same bits.  For a scored point, with k = labels[i] - 1, z = x_i - m_k,
 * A = R_k' R_k = Sigma_k^-1, df = df_k, y = R_k z and q = |y|^2 (mahalanobis):
 *   g            = A z = R_k' y, that is g_d = sum_{r <= d} R_rd y_r;
 *   a_d          = A_dd = sum_{r <= d} R_rd^2;
 *   residual     e_d = x_d - E[x_d | x_-d, k] = g_d / a_d, in the units of the data;
 *   q_-d         = q - g_d^2 / a_d, the squared distance of the point without feature d (>= 0 in exact arithmetic);
 *   zscore       t_d = g_d sqrt((df + D - 1) / (a_d (df + max(q_-d, 0)))): for a point of the cluster a Student-t variable with
 *                df + D - 1 degrees of freedom, whatever the other features are;
 *   feature_tail P(|T| >= |t_d|) for that Student-t: I_x(nu / 2, 1 / 2) at nu = df + D - 1, x = nu / (nu + t_d^2) -- the tail of
 *                dpmm_hip_typicality.h at D = 1.
 * At D = 1: t^2 = q and feature_tail = tail.  Skipped and incomplete points get NaN in residual, zscore and feature_tail and -1 in
 * features: without DPMM_OPT_TYPICALITY_GAPS an incomplete point's gaps are not marginalised ("Points with gaps" below).
 *
 * Points with gaps (DPMM_OPT_TYPICALITY_GAPS of dpmm_hip_typicality.h, whose "Points with gaps" defines M, O, D_o, C, t, res, P, q_o and says
 * which points are scored).  For such a point the law of one observed feature d given the OTHER OBSERVED features is again a Student-t:
 *   g'_d         = (P z_O)_d = (R' res)_d for d in O (on M, R' res = C' res = 0 by construction);
 *   a'_d         = P_dd = A_dd - w_d' A_MM^-1 w_d, w_d[a] = (R' c_a)_d = A_{d, M_a}, c_a column M_a of R: A_dd - |L^-1 w_d|^2 with C'C = L L';
 *   residual     g'_d / a'_d;   zscore  g'_d sqrt((df + D_o - 1) / (a'_d (df + max(q_o - g'_d^2 / a'_d, 0))));
 *   feature_tail the two-sided tail of the z-score at df + D_o - 1 degrees of freedom, by the routine above.
 * A feature of M has NaN in the three arrays; in top mode it ranks last (a NaN z-score) and its entry of `features` is -1.
 * Arithmetic: res in Float64 as for q_o, ROUNDED TO FLOAT32, then g' as a chain of Float32 FMAs in increasing r; w_a likewise (Float32
 * chains over the Float32 column); the forward substitution L v = w_d, |v|^2 and the subtraction from A_dd (the Float32 a_d above, widened)
 * in Float64; the three formulas in Float64 from the Float32 g', q_o, df, each result rounded once to Float32.
 * Error bounds (u = 2^-24, kappa = cond(A_MM), a_i over O, F = 2 r (D + 8 r + 16) 2^-52 kappa the Float64 term of dpmm_hip_typicality.h):
 *   g'         |dres| <= |dy| <= (D + 2) u sqrt(a_i), the rounding of res adds u |res|, the chain gamma(D) sum_r |R_rd| |res_r|, and
 *              sum_r |R_rd| |res_r| <= sqrt(A_dd) |res| <= sqrt(A_dd a_i):  |g'_d - exact| <= ((2 D + 3) u + F) sqrt(A_dd a_i) =: dg.
 *   a'         every w_d[a] carries at most D u sqrt(A_dd A_{M_a M_a}), so |dw_d| <= D u sqrt(A_dd tr A_MM); |L^-1| = lambda_min(A_MM)^-1/2
 *              and |v| <= sqrt(A_dd) give |d |v|^2| <= 2 D u A_dd sqrt(r kappa); the Float64 L is the factor of A_MM perturbed by at most
 *              r (D + 12 r + 10) u64 |A_MM| (dpmm_hip_typicality.h), which moves |v|^2 = w' A_MM^-1 w by at most F A_dd, the substitution's
 *              own Float64 roundings included; with the rounding of a_d:
 *              |a'_d - exact| / a'_d <= (A_dd / a'_d) (u (1 + 2 D sqrt(r kappa)) + F) =: ra -- the cancellation in A_dd - |v|^2 is the factor
 *              A_dd / a'_d.
 *   residual   |e_d - exact| <= dg / a'_d + |e_d| (ra + u).
 *   zscore     with dq the bound on q_o and h = df + q_o - g'_d^2 / a'_d, to first order
 *              |t_d - exact| <= sqrt((df + D_o - 1) / (a'_d h)) dg + |t_d| ra / 2 + |t_d| / (2 h) (dq + 2 |g'_d| dg / a'_d + g'_d^2 / a'_d ra) + 2 u |t_d|;
 *              twice that covers the second-order terms.
 *   tail       as above, at df + D_o - 1.
 * Out of scope: what dpmm_hip_typicality.h lists.
 *
 * Arithmetic.  z, y and q by the statements of dpmm_hip_typicality.h.  g_d as a chain of Float32 FMAs in increasing r.  a_d: the Float64 sum
 * of the squares of the Float32 R_rd, rounded once to Float32.  Then in Float32, every operation rounded once, divisions and square roots
 * correctly rounded, nothing contracted:
 *   e_d = g_d / a_d,   s = (g_d g_d) / a_d,   h = df + max(q - s, 0),   t_d = g_d sqrt((df + (D - 1)) / (a_d h)).
 * feature_tail: in Float64 from the Float32 t_d (its square is exact there) and df_k + D - 1 by the routine of dpmm_hip_typicality.h,
 * rounded once; t_d == 0 gives exactly 1, a t_d that is NaN gives NaN.
 *
 * Selection (top = m > 0): the m features of largest |t_d|, largest first, ties to the lower feature index, a t_d that is NaN last;
 * entry j of a row speaks of feature features[j] (0-based).  m rounds of a maximum over the 64 lanes of the point's wave, deterministic.
 * Nothing of size D * n is formed in this mode.
 *
 * Error bounds.  u = 2^-24; every sum below is evaluated in exact arithmetic from the Float32 x, m, R, df.  With
 *   b_d = sum_{r <= d} |R_rd| sum_{c >= r} |R_rc| |z_c|:
 *   g          every y_r carries at most gamma(D + 1) sum_c |R_rc| |z_c| (dpmm_hip_typicality.h); the second chain has at most D terms and
 *              adds gamma(D) sum_r |R_rd| |y_r|: together |g_d - exact| <= (2 D + 3) u b_d =: dg.
 *   residual   |e_d - exact| <= (2 D + 6) u b_d / A_dd: the rounding of a_d (u), the division (u) and |g_d| <= b_d.
 *   zscore     with dq = (3 D + 4) u a_i the bound of dpmm_hip_typicality.h on q and h = df + q_-d in exact arithmetic,
 *              |t_d - exact| <= sqrt((df + D - 1) / (A_dd h)) dg + |t_d| / (2 h) (dq + 2 |g_d| dg / A_dd) + 16 u |t_d|
 *              to first order (the propagation through g / sqrt(h); h >= df damps the cancellation in q - s; the eight roundings of
 *              the Float32 formulas enter with weights of at most 1 each, under the 16 u); twice that covers the second-order terms.
 *   tail       relative to 2 P(T >= |t_d|) of the returned Float32 t_d the result is within 1e-9 before the one rounding to Float32
 *              (6e-8) wherever the tail is at least 1e-30; a result below the smallest normal Float32 may come back as 0.
 *
 * One feature.  At D = 1 exact arithmetic gives q_-d = 0, t^2 = q and feature_tail = tail; Float32 gives this much of it.  y = R z is one
 * product, q = y^2 (1 + d5), and with every d_i one rounding, |d_i| <= u:
 *   g = R y (1 + d1),  a = R^2 (1 + d2),  s = y^2 (1 + 2 d1 + d3 - d2 + d4)   (the product g g and the division),
 *   q - s = y^2 eps exactly (the operands lie within a factor of 2),  |eps| <= 6 u,  where exact arithmetic has 0,
 *   h = df (1 + x)(1 + d10),  0 <= x <= 6 u q / df,   c = df + 0 exactly,
 *   t^2 / q - 1 = 2 d1 - d2 - d10 - x - d6 + d7 + 2 d8 + 2 d9 - d5   (a h: d6; c / (a h): d7; the square root: d8; g sqrt(..): d9)
 * to first order: eleven roundings and the cancellation of q - s, which h damps by df only.  With E = (11 + 6 q / df) u,
 *   |t^2 / q - 1| <= E (1 + E)        for every scored point at D = 1;
 * where q <= df / 8 the cancellation is below one u, the root mean square of the sum is 2.4 u, and the tests hold t^2 to 8 ulp of q
 * there.  No Float32 evaluation of q - s avoids the term: for q >> df it is what dq / (2 h) admits in the bound of the z-score above.
 * The two tails are then the same Float64 routine at the same df, at two arguments that far apart, each rounded once (u) from a value
 * within 1e-9: with S(q) = |d log tail / d log q| = sqrt(q) f(sqrt(q)) / tail(q), f the density of Student-t(df) -- it grows with q, towards
 * q / 2 for large df and df / 2 for large q -- taken at the far end q (1 + E (1 + E)) of the interval,
 *   |feature_tail - tail| / tail <= exp(S E (1 + E)) - 1 + 2 u + 2e-9   wherever the tail is at least 1e-30 (the mean value theorem in log q);
 * for q <= 1 and |t^2 / q - 1| <= 16 u (8 ulp at most) that is below (0.76 * 16 + 2.1) u < 2^-20, the allowance of the tail itself
 * (S <= 0.76: the normal law at q = 1, smaller for every Student-t).
 *
 * Determinism.  Every output word has one writer and is a function of the point and its cluster alone: the same bits whatever the cut
 * into uploads or the budget DPMM_OPT_SCORE_TABLE_MB.
 *
 * Limits: the NIW prior, every D it takes.  A Multinomial ctx: DPMM_EINVAL.
 *
 * Memory: what dpmm_typicality_points needs, and -- allocated by the first call of this header, rebuilt when dpmm_set_predictive_niw
 * has changed the parameters -- a row-major copy of the factors (K * D * 64 ceil(D / 64) floats) and the diagonals a (K * 64 ceil(D / 64)
 * floats); for the host variant the staging of one range's outputs.  A ctx that never calls this header allocates none of it.
 */
#ifndef DPMM_HIP_EXPLAIN_H
#define DPMM_HIP_EXPLAIN_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_EXPLAIN_MAX_TOP 16

typedef struct {
    int64_t *labels;         /* [n]      as dpmm_typicality_out                                                           */
    float   *mahalanobis;    /* [n]      as dpmm_typicality_out                                                           */
    float   *tail;           /* [n]      as dpmm_typicality_out                                                           */
    int64_t *skipped;        /* [1]      as dpmm_typicality_out                                          (host memory)    */
    int64_t *incomplete;     /* [1]      as dpmm_typicality_out                                          (host memory)    */
    float   *residual;       /* [n][ld]  e_d; NaN for a skipped or incomplete point                                       */
    float   *zscore;         /* [n][ld]  t_d; NaN for a skipped or incomplete point                                       */
    float   *feature_tail;   /* [n][ld]  P(|T| >= |t_d|); NaN for a skipped or incomplete point                           */
    int32_t *features;       /* [n][ld]  top > 0 only: the 0-based features the entries speak of; -1 likewise             */
    int32_t  top;            /* 0: all D features in order (entry d is feature d); m: the m of largest |t_d|, best first  */
    int64_t  ld;             /* floats (features: words) between the rows of two points, >= (top ? top : D)               */
} dpmm_explain_out;          /* every pointer may be NULL; at least one must not be                                       */

/* n = n_local of the ctx.  The outputs are point-major; of a row the first (top ? top : D) entries are written, the rest is not
 * touched.  Multinomial ctx, out == NULL, every pointer NULL, top outside 0 .. min(D, DPMM_EXPLAIN_MAX_TOP), features given with
 * top == 0, ld too small or not below 2^31, n_local * ld * 8 not representable in 64 bits: DPMM_EINVAL.  Before dpmm_set_predictive_niw: DPMM_ESTATE.  n_local == 0: DPMM_OK (the counters are 0).
 * Both calls return after the ctx stream has been synchronised. */
int dpmm_explain_points(dpmm_ctx *ctx, const dpmm_explain_out *out);          /* host memory                              */

/* Every array is checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned to its element, the whole extent of
 * n_local * ld entries inside its allocation) before anything is launched: DPMM_EINVAL, the message names the argument. */
int dpmm_explain_points_device(dpmm_ctx *ctx, const dpmm_explain_out *out);   /* device memory; counters stay host        */

#ifdef __cplusplus
}
#endif
#endif
