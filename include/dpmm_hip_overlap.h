/*
 * dpmm_hip_overlap.h -- optional companion of dpmm_hip.h: the posterior overlap of the clusters, O[k][j] = sum_i p_ik p_ij, accumulated
 * on the GPU while the table that the label rule evaluates anyway goes by.  The answer is K * K doubles; temporary memory does not
 * grow with n and nothing of size n reaches the host.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_score_points needs -- the points (any upload call) and dpmm_set_predictive_niw / _mult.
 *
 * Definitions.  parr[k][i], labels, M, S and probs are exactly those of dpmm_hip_score.h: M the maximum over k of parr[k][i] with NaN
 * skipped, S the Float32 sum in increasing k of expf(parr[k][i] - M), probs[i][k] = expf(parr[k][i] - M) / S.
 * A point TAKES PART iff its row of parr holds no NaN and M is finite (the rule of dpmm_hip_rank.h).  Every other point is counted in
 * `skipped` and contributes nothing.  For a point that takes part p_ik is the Float32 value probs[i][k], bit-identical to what
 * dpmm_score_points writes (the same device code forms it), and
 *   overlap[k][j]   sum_i (double)p_ik * (double)p_ij        over the points that take part, in Float64
 *   mass[k]         sum_i (double)p_ik
 *   count[k]        the number of points that take part with labels == k + 1         (exact)
 *   skipped[0]      the number of points that do not take part                       (exact)
 * The product of two Float32 values is exact in Float64, so only the order of the additions separates `overlap` (and `mass`) from
 * any other Float64 evaluation of the same sum.  overlap is symmetric bit for bit: one triangle is computed and mirrored.
 *
 * Error bound.  All terms are non-negative, so a Float64 summation of n of them in ANY order lies within a relative n * 2^-53 of the
 * exact sum (every addition rounds a partial sum of non-negative terms by at most 2^-53 of itself, and a term passes through fewer
 * than n additions).  Two such summations -- this one and a caller's -- therefore agree within a relative n * 2^-52 in every entry
 * of overlap and mass, n the number of points accumulated.
 *
 * Determinism.  The same points, the same cuts into uploads and the same DPMM_OPT_SCORE_TABLE_MB give the same bits on every run: no
 * floating-point atomics; a range of the table is cut into chunks whose number depends on the range's length and K alone, every
 * (chunk, block of the matrix) has one writer, and the chunks are added in increasing order.  Across other cuts or budgets the
 * results agree within the bound above; count and skipped are equal.
 *
 * Limits: K up to DPMM_MAX_CLUSTERS, both priors.
 *
 * Memory: the accumulators (K * K + K doubles, 8 * (K + 1) counters), two floats per point of one range of the score table and the
 * chunk partials -- at most DPMM_OVERLAP_PARTIAL_BLOCKS blocks of 64 * 64 doubles plus as many rows of 64 doubles, 17 MB -- belong
 * to the ctx; dpmm_overlap_begin allocates them (grown when a call needs more, freed by dpmm_destroy), accumulate and read allocate
 * nothing beyond the score table of dpmm_hip_score.h: a second pass of the same shape allocates nothing.
 */
#ifndef DPMM_HIP_OVERLAP_H
#define DPMM_HIP_OVERLAP_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_OVERLAP_PARTIAL_BLOCKS 512

typedef struct {
    double  *overlap;        /* [K][K]  sum_i p_ik p_ij over the points that take part, symmetric bit for bit */
    double  *mass;           /* [K]     sum_i p_ik                                                            */
    int64_t *count;          /* [K]     points that take part with labels == k + 1                            */
    int64_t *skipped;        /* [1]     points that do not take part                                          */
} dpmm_overlap_out;          /* host memory; every pointer may be NULL */

/* Starts an accumulation: clears the ctx-owned overlap, mass, count and skipped.  Before dpmm_set_predictive_*: DPMM_ESTATE. */
int dpmm_overlap_begin(dpmm_ctx *ctx);

/* Adds the points 0..n_valid-1 of the ctx's current upload; points at or beyond n_valid are ignored (the zero padding of a short
 * slab is a perfectly good point of some cluster).  The table is evaluated range by range inside the budget DPMM_OPT_SCORE_TABLE_MB,
 * as dpmm_score_points does, under DPMM_OPT_SCORE_MISSING with the marginal entries of dpmm_hip_missing.h.  n_valid outside
 * 0..n_local: DPMM_EINVAL.  Without dpmm_overlap_begin, or with another K or other predictive parameters than it saw: DPMM_ESTATE.
 * Every refusal comes before any launch.  Returns without waiting for the GPU. */
int dpmm_overlap_accumulate(dpmm_ctx *ctx, int64_t n_valid);

/* The sums as they stand, written to host memory; reading does not end the accumulation.  Returns after the ctx stream has been
 * synchronised.  Without dpmm_overlap_begin: DPMM_ESTATE.  out == NULL: DPMM_EINVAL. */
int dpmm_overlap_read(dpmm_ctx *ctx, const dpmm_overlap_out *out);

#ifdef __cplusplus
}
#endif
#endif
