/*
 * dpmm_hip_holdout.h -- optional companion of dpmm_hip.h: the points that the accumulation of dpmm_hip_batchstats.h HOLDS OUT -- those far
 * from every cluster of the served model, by the floor min_logdens or the calibrated floor min_tail of dpmm_hip_typicality.h -- collected
 * on the GPU while the score table goes by: their coordinates and their global indices, compacted in increasing index into device memory
 * of the caller.  They are the points that say the data has changed; host/score.py clusters them and appends what it finds to the served
 * model (Predictor.grow).  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: the points (any dense upload call) and dpmm_set_predictive_niw.
 *
 * Definitions.  Every point 0 .. n_valid - 1 of an upload is in exactly one class -- skipped, else held out, else incomplete, else it takes
 * part -- by the rule of dpmm_hip_batchstats.h with the floors of dpmm_batchstats_begin (use_floor, min_logdens) and of
 * dpmm_batchstats_set_min_tail (use_tail, min_tail), formed by the same device code: the counters of this header equal those of
 * dpmm_batchstats_read over the same calls, and a point is collected here exactly when it is counted in held_out there.
 * With s = 0, 1, .. numbering the held-out points in the order of the calls and, inside a call, of their position i:
 *   dst_index[s]         lo + i, 0-based;
 *   dst_points[s][0..D)  the point as the ctx holds it: Float32, after the projection if the ctx has one, without the padding of its rows.
 * Slots s >= cap are not written; total counts every held-out point, stored = min(total, cap).
 *
 * Determinism.  The result is a function of the points, the model and the floors alone: the same bits whatever the cut into uploads,
 * n_valid inside a range, or the budget DPMM_OPT_SCORE_TABLE_MB.  No atomics: per range of the table, a class pass leaves one ballot word
 * per wave and the counts of every workgroup of 256 points, one workgroup scans the counts from a running total kept in device memory and
 * advances it, and a gather pass ranks the held-out points of a workgroup from the ballots and copies their rows.  Ranges and uploads chain
 * on the ctx stream without a host synchronisation.
 *
 * Limits: the NIW prior and dense points, one ctx (several ranks: each collects its own shard; nothing here merges them).  A Multinomial
 * ctx is refused (DPMM_EINVAL), and so are sparse stores, which only that prior has.  Only held-out points are collected, no other class.
 * Merging a new cluster with an old one is no part of this header or of Predictor.grow.
 *
 * Memory the ctx owns: one 64-bit word per 64 points and four 32-bit words plus one 64-bit word per 256 points of one range of the score
 * table, four counters, and with use_tail the tails and scratch of dpmm_hip_typicality.h; allocated by the first accumulate that needs
 * them, freed by dpmm_destroy.  Nothing else of size n.
 */
#ifndef DPMM_HIP_HOLDOUT_H
#define DPMM_HIP_HOLDOUT_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int64_t *total;          /* [1]   held-out points seen since dpmm_holdout_begin                                    */
    int64_t *stored;         /* [1]   of them written to dst_points / dst_index: min(total, cap)                       */
    int64_t *skipped;        /* [1]   points with a NaN in their row of parr or M not finite                           */
    int64_t *incomplete;     /* [1]   points neither skipped nor held out with a feature that is not finite            */
    int64_t *scored;         /* [1]   points that take part: the rest                                                  */
} dpmm_holdout_out;          /* host memory; every pointer may be NULL */

/* Starts a collection: clears the counters and fixes the floors -- use_floor != 0: points with logdens < min_logdens (min_logdens NaN holds
 * nobody out); use_tail != 0: complete points with tail < min_tail, min_tail in (0, 1]; either one holds a point out -- and the destination
 * of every dpmm_holdout_accumulate that follows: dst_points [cap][D] Float32, point-major and contiguous, dst_index [cap], device memory of
 * the ctx's device, checked as dpmm_hip_tensor.h describes.  cap == 0: the points are only counted, the pointers may be NULL.
 * Multinomial ctx, use_floor == 0 && use_tail == 0, min_tail outside (0, 1] or NaN, cap < 0, a bad pointer: DPMM_EINVAL.  Before
 * dpmm_set_predictive_niw: DPMM_ESTATE. */
int dpmm_holdout_begin(dpmm_ctx *ctx, int use_floor, float min_logdens, int use_tail, float min_tail, float *dst_points, int64_t *dst_index, int64_t cap);

/* Classifies the points 0..n_valid-1 of the ctx's current upload and appends the held-out ones; lo: the global index of point 0 of the
 * upload, as dpmm_rank_accumulate takes it.  The table is evaluated range by range inside the budget DPMM_OPT_SCORE_TABLE_MB.  n_valid
 * outside 0..n_local, lo < 0 or lo + n_valid beyond 2^62: DPMM_EINVAL.  Without dpmm_holdout_begin, or with another K or other predictive
 * parameters than it saw: DPMM_ESTATE.  The destination is checked again.  Every refusal comes before any launch.  Returns without waiting
 * for the GPU: the caller's buffers are complete after dpmm_holdout_read. */
int dpmm_holdout_accumulate(dpmm_ctx *ctx, int64_t lo, int64_t n_valid);

/* The counters as they stand, written to host memory; reading does not end the collection.  Returns after the ctx stream has been
 * synchronised.  Without dpmm_holdout_begin: DPMM_ESTATE.  out == NULL: DPMM_EINVAL. */
int dpmm_holdout_read(dpmm_ctx *ctx, const dpmm_holdout_out *out);

#ifdef __cplusplus
}
#endif
#endif
