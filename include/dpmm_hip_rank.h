/*
 * dpmm_hip_rank.h -- optional companion of dpmm_hip.h: exemplars, the m most and the m least typical points of every cluster, selected on
 * the GPU while the table that the label rule evaluates anyway goes by.  The answer is K * m indices; temporary memory does not grow
 * with n and nothing of size n reaches the host.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: what dpmm_score_points needs -- the points (any upload call) and dpmm_set_predictive_niw / _mult.
 *
 * Definitions.  Take the table parr[k][i] that dpmm_predict returns, with the label rule of dpmm_hip_score.h.  For point i:
 *   lab_i   the 1-based argmax by Julia's rule (the first NaN wins, else the first maximum);
 *   s_i     the maximum over k of parr[k][i] with NaN skipped, in Float32 -- the M of dpmm_hip_score.h.
 * A point TAKES PART iff its row holds no NaN and s_i is finite.  Otherwise it is counted in `skipped` and appears nowhere else.
 * For a point that takes part, s_i == parr[lab_i - 1][i]: the log predictive density of its own cluster plus log w_k, so inside one
 * cluster it ranks by that cluster's density.
 * The data of a call has points with global 0-based indices 0..n-1, across all slabs (dpmm_rank_accumulate's index_base + i).
 * For every cluster k, the TYPICAL list is the first m points with lab == k that take part, ordered by (s descending, index ascending).
 * The FRINGE list is the first m of those ordered by (s ascending, index ascending).
 *   count[k]   the number of points with lab == k that take part;
 *   unused slots j >= count[k] hold index -1 and score NaN;
 *   scores are returned bit-identical to the table entry.
 * The order is total, so the result is unique.  It does not depend on how the points were cut into uploads, on
 * DPMM_OPT_SCORE_TABLE_MB, on any grid shape or on the order in which candidates were met.
 * (Scores are ordered by their bit patterns, which is the order of the values for every pair of finite numbers but one: -0.0 ranks
 * below +0.0.)
 *
 * Limits: 1 <= m <= DPMM_RANK_MAX_M, K up to DPMM_MAX_CLUSTERS, global indices below 2^32 (a key is one 64-bit word: score | index).
 *
 * Memory: the running lists (2 * K * 64 keys), the counters, a candidate buffer of min(n_local, 262144) points and the staging of
 * dpmm_rank_read belong to the ctx; dpmm_rank_begin allocates them (grown when a call needs more, freed by dpmm_destroy), accumulate
 * and read allocate nothing beyond the score table of dpmm_hip_score.h: a second pass of the same shape allocates nothing.
 */
#ifndef DPMM_HIP_RANK_H
#define DPMM_HIP_RANK_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_RANK_MAX_M 64
#define DPMM_RANK_TYPICAL 1
#define DPMM_RANK_FRINGE 2

typedef struct {
    int64_t *typ_idx;        /* [K][m]  global 0-based indices, most typical first; -1 = unused slot  */
    float   *typ_score;      /* [K][m]  their s, non-increasing; NaN = unused slot                    */
    int64_t *fringe_idx;     /* [K][m]  least typical first                                           */
    float   *fringe_score;   /* [K][m]  non-decreasing                                                */
    int64_t *count;          /* [K]     points of the cluster that take part                          */
    int64_t *skipped;        /* [1]     points that do not take part                                  */
} dpmm_rank_out;             /* every pointer may be NULL; a list that `which` left out is all unused slots */

/* Starts a ranking: clears the ctx-owned running lists, count and skipped.  which: DPMM_RANK_TYPICAL | DPMM_RANK_FRINGE, one at least.
 * m outside 1..DPMM_RANK_MAX_M or which outside 1..3: DPMM_EINVAL.  Before dpmm_set_predictive_*: DPMM_ESTATE. */
int dpmm_rank_begin(dpmm_ctx *ctx, int m, int which);

/* Ranks the points 0..n_valid-1 of the ctx's current upload as global indices index_base + i; points at or beyond n_valid are ignored
 * (the zero padding of a short slab can be the densest point of a cluster).  The table is evaluated range by range inside the budget
 * DPMM_OPT_SCORE_TABLE_MB, as dpmm_score_points does.  n_valid outside 0..n_local, index_base < 0 or index_base + n_valid > 2^32:
 * DPMM_EINVAL.  Without dpmm_rank_begin, or with another K than it saw: DPMM_ESTATE.  Returns without waiting for the GPU. */
int dpmm_rank_accumulate(dpmm_ctx *ctx, int64_t index_base, int64_t n_valid);

/* The lists as they stand; reading does not end the accumulation.  Both calls return after the ctx stream has been synchronised.
 * Without dpmm_rank_begin: DPMM_ESTATE.  out == NULL: DPMM_EINVAL. */
int dpmm_rank_read(dpmm_ctx *ctx, const dpmm_rank_out *out);            /* host memory   */

/* Every non-null output is checked as dpmm_hip_tensor.h describes (device memory of the ctx's device, aligned to its element, the whole
 * extent inside its allocation) before anything is launched: DPMM_EINVAL, the message names the argument. */
int dpmm_rank_read_device(dpmm_ctx *ctx, const dpmm_rank_out *out);     /* device memory */

#ifdef __cplusplus
}
#endif
#endif
