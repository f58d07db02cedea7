/*
 * dpmm_hip_explain_groups.h -- optional companion of dpmm_hip.h, dpmm_hip_typicality.h and dpmm_hip_explain.h: WHICH GROUP of features makes
 * a point atypical of its cluster.  dpmm_hip_explain.h conditions one feature on all the others; features often come in blocks (the parts
 * of a concatenated embedding, the channels of a sensor, the one-hot columns of a variable, the lags of a series), and inside a correlated
 * block every feature is explained away by its block-mates while the block as a whole can be impossible.  Under the point's own Student-t
 * predictive the law of a block given the rest is again a multivariate Student-t in closed form, and its squared distance has an F law:
 * one calibrated tail per group.  Additive: DPMM_ABI_VERSION is unchanged, no option key is added.
 *
 * State needed: the points (any dense upload call), dpmm_set_predictive_niw(K, m, R, logdet, df, w) and dpmm_set_explain_groups for it.
 *
 * Definitions.  labels, mahalanobis, tail, skipped, incomplete and the three classes of a point are exactly those of
 * dpmm_hip_typicality.h, formed by the same device code: the same bits.  For a scored point, in the notation of dpmm_hip_explain.h
 * (k = labels[i] - 1, z = x_i - m_k, A = R_k' R_k, df = df_k, y = R_k z, q = |y|^2, g = A z = R_k' y), and a group G of s features, -G the
 * other D - s:
 *   conditional residual   x_G - E[x_G | x_-G, k] = A_GG^-1 g_G               (not returned);
 *   group_mahalanobis      q_G = g_G' A_GG^-1 g_G >= 0, its squared length in the conditional metric;
 *   q - q_G                = q_-G, the squared distance of x_-G under its marginal (>= 0 in exact arithmetic);
 *   conditional law        x_G | x_-G ~ t_{df + D - s}(., (df + q_-G) / (df + D - s) A_GG^-1);
 *   statistic              f_G = q_G (df + D - s) / (df + max(q - q_G, 0)): for a point of the cluster f_G / s ~ F(s, df + D - s), whatever
 *                          the other features are;
 *   group_tail             P(F >= f_G / s) = I_x(nu / 2, s / 2) at nu = df + D - s, x = nu / (nu + f_G): the tail of dpmm_hip_typicality.h
 *                          with (q, df, D) = (f_G, df + D - s, s).  Uniform on (0, 1) for points of the cluster; comparable across groups
 *                          of different sizes, across clusters and across D.
 * One feature, G = {d}: q_G = g_d^2 / a_d, f_G = zscore^2 and group_tail = feature_tail of dpmm_hip_explain.h, in exact arithmetic.
 * All features, G = 0 .. D - 1: q_G = q and group_tail = tail.  Skipped and incomplete points get NaN in both arrays (gaps are not
 * marginalised here, whatever DPMM_OPT_TYPICALITY_GAPS says for the first three arrays).
 *
 * Tables.  With A_GG = L L' (Cholesky, L lower triangular) and W = L^-1 (lower triangular): q_G = |W g_G|^2.  The caller forms W in
 * Float64 from the Float32 R it gave dpmm_set_predictive_niw, widened -- the exact A is defined from these values -- and hands it over
 * PACKED: cluster k = 0 .. K - 1, inside it group j = 0 .. G - 1, inside it the rows r = 0 .. s_j - 1 of the lower triangle, row r holding
 * the columns c = 0 .. r:
 *   W_k,j[r][c] = W[k T + base_j + r (r + 1) / 2 + c],   base_j = sum_{i < j} s_i (s_i + 1) / 2,   T = base_G.
 * Row r, column c speak of the features features[offsets[j] + r] and features[offsets[j] + c].  The worker rounds every value to Float32
 * once and keeps, per cluster and group, the columns of W one after the other, each padded with zeros to 64 ceil(s / 64) rows.
 *
 * Arithmetic.  z, y, q and g by the statements of dpmm_hip_explain.h.  Per group, with g_c = g[features[offsets[j] + c]]:
 *   v_r = sum_{c <= r} W_rc g_c as a chain of Float32 FMAs in increasing c from 0 (v = fma(W_rc, g_c, v); the steps c > r of a tile multiply
 *         a stored zero and leave v as it is);
 *   q_G = sum_r v_r^2 in this order: lane l of the point's wave forms p = fma(v_r, v_r, p) from p = 0 over its rows r = l, l + 64, .. in
 *         increasing r; then six exchanges p += p of lane (l xor o), o = 32, 16, 8, 4, 2, 1 -- every lane ends with the same bits;
 *   then in Float32, every operation rounded once, the division correctly rounded, nothing contracted:
 *         h = df + max(q - q_G, 0),   f = (q_G (df + (D - s))) / h           (D - s converted exactly);
 *   group_tail in Float64 from the Float32 f and df_k + (D - s) by the routine of dpmm_hip_typicality.h, rounded once; f == 0 gives
 *         exactly 1, an f that is NaN gives NaN.
 *
 * Error bounds.  u = 2^-24; every sum is evaluated in exact arithmetic from the Float32 x, m, R, df and the Float64 W.
 *   g          |g_c - exact| <= (2 D + 3) u b_c =: dg_c, b_c of dpmm_hip_explain.h.
 *   v          the chain has at most s terms, each W_rc carries one rounding (u), each product and sum one:
 *              |v_r - exact| <= sum_c |W_rc| dg_c + (s + 2) u sum_c |W_rc| |g_c| =: dv_r.
 *   q_G        the squares and their sum (ceil(s / 64) + 6 roundings on a lane's path, of which only ceil(log2 s) + 1 act on non-zero terms):
 *              |q_G - exact| <= 2 sum_r |v_r| dv_r + (s + 2) u q_G to first order; twice that covers the second-order terms.
 *   tail       h and f are correctly rounded functions of the returned Float32 q, q_G, df: a recomputation in Float32 gives the bits of f.
 *              Relative to I_x(nu / 2, s / 2) at that f the result is within 1e-9 before the one rounding to Float32 (6e-8) wherever
 *              the tail is at least 1e-30; a result below the smallest normal Float32 may come back as 0.
 *
 * Determinism.  Every output word has one writer and is a function of the point, its cluster and the groups alone: the same bits
 * whatever the cut into uploads or the budget DPMM_OPT_SCORE_TABLE_MB.  No workgroup barrier, no atomics: g goes through a strip of LDS
 * that belongs to the point's wave (at most 1 KB, at D = 256) so that a group's entries can be gathered by index.
 *
 * Work beyond dpmm_explain_points' two passes over R_k: sum_j s_j <= D FMA steps per point (each over ceil(s_j / 64) row tiles).
 *
 * Limits: the NIW prior, every D it takes, 1 <= G <= DPMM_EXPLAIN_MAX_GROUPS.  A Multinomial ctx: DPMM_EINVAL.  Out of scope: the
 * residual vector of a group, a selection of the top groups (G <= 64: the caller ranks), overlapping groups, gaps, several ranks.
 *
 * Memory: what dpmm_explain_points needs (its row-major copy of the factors is shared), and -- allocated by dpmm_set_explain_groups --
 * K sum_j s_j 64 ceil(s_j / 64) floats of tables and G + 1 + sum_j s_j + 2 G words of descriptors; for the host variant the staging
 * of one range's outputs.  A ctx that never calls dpmm_set_explain_groups allocates none of it.
 */
#ifndef DPMM_HIP_EXPLAIN_GROUPS_H
#define DPMM_HIP_EXPLAIN_GROUPS_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_EXPLAIN_MAX_GROUPS 64

/* The groups and their tables for the predictive parameters in force: G groups, group j the features
 * features[offsets[j]] .. features[offsets[j + 1] - 1], W packed as "Tables" says (K that of dpmm_set_predictive_niw).  Needed:
 * 1 <= G <= DPMM_EXPLAIN_MAX_GROUPS; offsets[0] == 0 and offsets increasing strictly (no empty group); every index 0-based in 0 .. D - 1,
 * increasing strictly inside a group; the groups pairwise disjoint (they need not cover all features); every W value finite.  A violation,
 * a null argument or a Multinomial ctx: DPMM_EINVAL, the message names the argument.  Before dpmm_set_predictive_niw: DPMM_ESTATE.  The
 * worker records the predictive parameter set the tables were made for.  A call that is refused for its arguments or the state changes
 * nothing: tables in force stay in force. */
int dpmm_set_explain_groups(dpmm_ctx *ctx, int32_t G, const int64_t *offsets, const int32_t *features, const double *W);

typedef struct {
    int64_t *labels;              /* [n]      as dpmm_typicality_out                                                      */
    float   *mahalanobis;         /* [n]      as dpmm_typicality_out                                                      */
    float   *tail;                /* [n]      as dpmm_typicality_out                                                      */
    int64_t *skipped;             /* [1]      as dpmm_typicality_out                                     (host memory)    */
    int64_t *incomplete;          /* [1]      as dpmm_typicality_out                                     (host memory)    */
    float   *group_mahalanobis;   /* [n][ld]  q_G; NaN for a skipped or incomplete point                                  */
    float   *group_tail;          /* [n][ld]  P(F >= f_G / s); NaN for a skipped or incomplete point                      */
    int64_t  ld;                  /* floats between the rows of two points, >= G                                          */
} dpmm_explain_groups_out;        /* every pointer may be NULL; at least one must not be                                  */

/* n = n_local of the ctx.  The outputs are point-major; of a row the first G entries are written, the rest is not touched.  Multinomial
 * ctx, out == NULL, every pointer NULL, ld < G or not below 2^31, n_local * ld * 8 not representable in 64 bits: DPMM_EINVAL.  Before
 * dpmm_set_predictive_niw, without tables, or with tables made for an older predictive parameter set than the one in force: DPMM_ESTATE.
 * n_local == 0: DPMM_OK (the counters are 0).  Both calls return after the ctx stream has been synchronised. */
int dpmm_explain_groups_points(dpmm_ctx *ctx, const dpmm_explain_groups_out *out);          /* host memory                */

/* Every array is checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned to its element, the whole extent of
 * n_local * ld entries inside its allocation) before anything is launched: DPMM_EINVAL, the message names the argument. */
int dpmm_explain_groups_points_device(dpmm_ctx *ctx, const dpmm_explain_groups_out *out);   /* device memory; counters host */

#ifdef __cplusplus
}
#endif
#endif
