/*
 * dpmm_hip_batchstats.h -- optional companion of dpmm_hip.h: the per-cluster sufficient statistics of a batch of points under the
 * model the ctx serves, N[k] = sum_i w_ik, sums[k] = sum_i w_ik x_i, S[k] = sum_i w_ik x_i x_i', accumulated on the GPU in Float64 while
 * the table that the label rule evaluates anyway goes by.  They are what the conjugate NIW update needs to fold the batch into the
 * posterior (host/absorb.py), and the moments a drift monitor or an EM step asks for.  The answer is K * (D * D + D + 1) doubles;
 * temporary memory does not grow with n and nothing of size n reaches the host.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: the points (any dense upload call) and dpmm_set_predictive_niw.
 *
 * Definitions.  parr[k][i], labels, M, S, logdens and probs are exactly those of dpmm_hip_score.h / dpmm_hip_overlap.h, formed by the
 * same device code (score_device.h); under DPMM_OPT_SCORE_MISSING the marginal entries of dpmm_hip_missing.h are used, as
 * dpmm_overlap_accumulate does.  x_i is the point as the ctx holds it: Float32, after the projection if the ctx has one.
 * Every point 0 .. n_valid - 1 is in exactly one class:
 *   skipped      a NaN in its row of parr, or M not finite (the rule of dpmm_hip_overlap.h); else
 *   held out     use_floor != 0 and logdens_i < min_logdens, logdens_i the Float32 value dpmm_score_points writes; else
 *   incomplete   one of its D features is not finite (a marginalised point, or a finite row over a feature that is not); else
 *   takes part   and is counted in count[k], k + 1 its label.
 * Only points that take part add to the sums, with the weights
 *   DPMM_BATCHSTATS_HARD   w_ik = 1 if labels_i == k + 1, else 0
 *   DPMM_BATCHSTATS_SOFT   w_ik = (double)p_ik, p_ik the Float32 value probs[i][k], bit-identical to what dpmm_score_points writes
 *   N[k]          sum_i w_ik
 *   sums[k][d]    sum_i w_ik x_id
 *   S[k][d][e]    sum_i (w_ik x_id) x_ie
 * all in Float64.  w_ik x_id is the product of two Float32 values and exact in Float64 (24 + 24 bits); it is formed there, never in
 * Float32.  S[k] is symmetric bit for bit: one triangle is computed and mirrored.  In HARD mode N[k] == count[k] exactly.
 *
 * Error bound.  With T[k][d][e] = sum_i w_ik |x_id| |x_ie| and T1[k][d] = sum_i w_ik |x_id|, u = 2^-53 and
 * gamma(m) = m u / (1 - m u): a term of S is rounded once as a product and passes through fewer than n additions, whatever their
 * order and whether or not product and addition are fused, so |S - exact| <= gamma(n + 1) T, |sums - exact| <= gamma(n) T1 and
 * |N - exact| <= gamma(n) N.  Two such evaluations -- this one and a caller's -- agree within 2 gamma(n + 2) times T, T1 and N.
 *
 * Determinism.  The same points, the same cuts into uploads and the same DPMM_OPT_SCORE_TABLE_MB give the same bits on every run: no
 * floating-point atomics; a range of the table is cut into chunks whose number depends on the range's length, K and D alone; inside a
 * chunk the points with w_ik != 0 are taken in increasing i; every (chunk, cluster, pair of 64-row blocks) has one writer, and the
 * chunks are added in increasing order.  Across other cuts or budgets the results agree within the bound; the counters are equal.
 *
 * Limits: the NIW prior, every D it takes, K up to DPMM_MAX_CLUSTERS.  A Multinomial ctx is refused (DPMM_EINVAL): its statistics, over
 * the Float32, byte and sparse point stores, are those of dpmm_hip_countstats.h.
 *
 * Memory: the accumulators (K * (D * D + D + 1) doubles, 8 * (K + 3) counters), two floats per point of one range of the score table
 * and the chunk partials -- at most DPMM_BATCHSTATS_PARTIAL_BLOCKS blocks of 64 * 64 doubles, 64 MB, plus at most as many rows of
 * 64 + 1 doubles -- belong to the ctx; dpmm_batchstats_begin allocates them (grown when a call needs more, freed by dpmm_destroy),
 * accumulate and read allocate nothing beyond the score table of dpmm_hip_score.h: a second pass of the same shape allocates nothing.
 */
#ifndef DPMM_HIP_BATCHSTATS_H
#define DPMM_HIP_BATCHSTATS_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_BATCHSTATS_HARD 0
#define DPMM_BATCHSTATS_SOFT 1
#define DPMM_BATCHSTATS_PARTIAL_BLOCKS 2048

typedef struct {
    double  *N;              /* [K]        sum_i w_ik over the points that take part                                 */
    double  *sums;           /* [K][D]     sum_i w_ik x_id                                                           */
    double  *S;              /* [K][D][D]  sum_i w_ik x_id x_ie, symmetric bit for bit                               */
    int64_t *count;          /* [K]        points that take part with labels == k + 1                                */
    int64_t *skipped;        /* [1]        points with a NaN in their row of parr or M not finite                    */
    int64_t *incomplete;     /* [1]        points neither skipped nor held out with a feature that is not finite     */
    int64_t *held_out;       /* [1]        points not skipped with logdens < min_logdens (use_floor != 0)            */
} dpmm_batchstats_out;       /* host memory; every pointer may be NULL */

/* Starts an accumulation: clears the ctx-owned N, sums, S and counters and fixes the weights (mode) and the floor (use_floor != 0:
 * points with logdens < min_logdens are held out; min_logdens NaN holds nobody out) of every dpmm_batchstats_accumulate that follows.
 * Multinomial ctx, another mode than the two above: DPMM_EINVAL.  Before dpmm_set_predictive_niw: DPMM_ESTATE. */
int dpmm_batchstats_begin(dpmm_ctx *ctx, int mode, int use_floor, float min_logdens);

/* Adds the points 0..n_valid-1 of the ctx's current upload; points at or beyond n_valid are ignored (the zero padding of a short
 * slab is a perfectly good point of some cluster).  The table is evaluated range by range inside the budget DPMM_OPT_SCORE_TABLE_MB,
 * as dpmm_score_points does.  n_valid outside 0..n_local: DPMM_EINVAL.  Without dpmm_batchstats_begin, or with another K or other
 * predictive parameters than it saw: DPMM_ESTATE.  Every refusal comes before any launch.  Returns without waiting for the GPU. */
int dpmm_batchstats_accumulate(dpmm_ctx *ctx, int64_t n_valid);

/* The sums as they stand, written to host memory; reading does not end the accumulation.  Returns after the ctx stream has been
 * synchronised.  Without dpmm_batchstats_begin: DPMM_ESTATE.  out == NULL: DPMM_EINVAL. */
int dpmm_batchstats_read(dpmm_ctx *ctx, const dpmm_batchstats_out *out);

#ifdef __cplusplus
}
#endif
#endif
