/*
 * dpmm_hip_countholdout.h -- optional companion of dpmm_hip.h: the Multinomial counterpart of dpmm_hip_holdout.h and of the calibrated
 * floor of dpmm_hip_typicality.h.  Two things that belong together:
 *
 *   1. a floor that means something for documents.  logdens_i = logsumexp_k(log w_k + x_i . log theta_k) scales with the number of counts
 *      in the point, so the floor min_logdens of dpmm_hip_countstats.h is mostly a length filter: it holds out long ordinary documents and
 *      keeps short novel ones.  The quantity that is comparable across lengths is the log-density PER COUNT, the log of the inverse
 *      perplexity.  No closed-form tail exists for this prior; this floor is what the Multinomial prior has in the place of min_tail.
 *      dpmm_countstats_set_per_count gives it to the accumulation of dpmm_hip_countstats.h (it is declared here as
 *      dpmm_batchstats_set_min_tail is declared in dpmm_hip_typicality.h: dpmm_hip_countstats.h itself is unchanged);
 *   2. the points that accumulation HOLDS OUT, by either floor, collected on the GPU while the score table goes by: compacted in increasing
 *      index into device memory of the caller, from whichever of the three point stores is live.  host/score.py clusters them and appends
 *      what it finds to the served model (Predictor.grow_counts).
 * Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: a Multinomial ctx, the points (any upload call) and dpmm_set_predictive_mult.
 *
 * Definitions.  t_i is the Float64 total of the point's values: of its D features in the dense stores, of its stored entries in the sparse
 * store.  It is formed only when the floor per count is on, by one wave per point: lane l adds entries l, l + 64, .. in order and a fixed
 * butterfly combines the 64 lanes, so t_i is a function of the point alone, whatever the cut into uploads or ranges, and exact for integer
 * data.  Every point 0 .. n_valid - 1 is in exactly one class -- skipped, else held out, else incomplete, else it takes part -- by the rule
 * of dpmm_hip_countstats.h, whose `held out` becomes
 *   held out     use_floor != 0 and logdens_i < min_logdens; or use_per_count != 0, every value of the point is finite, t_i > 0 and
 *                (double)logdens_i < (double)min_logdens_per_count * t_i, logdens_i the Float32 value dpmm_score_points writes.
 * An empty point (t_i == 0) and a point with a value that is not finite are never held out by the floor per count.  The class is formed
 * by one piece of device code (csrc/countstats_device.h) for both headers: the counters of dpmm_countholdout_read equal those of
 * dpmm_countstats_read over the same calls and floors, and a point is collected here exactly when it is counted in held_out there.
 *
 * The destination follows the store that is live at dpmm_countholdout_accumulate.  With s = 0, 1, .. numbering the held-out points in the
 * order of the calls and, inside a call, of their position i:
 *   both         dst_index[s] = lo + i, 0-based;
 *   dense stores (the Float32 matrix and the byte copy a ctx keeps instead of it): dst_points[s][0..D) the point in Float32, bytes widened;
 *   sparse store dst_colptr[s + 1] = the entries of the held-out points 0 .. s (dst_colptr[0] = 0 is written by dpmm_countholdout_begin),
 *                dst_rowval / dst_val [dst_colptr[s] .. dst_colptr[s + 1]) the point's rows (0-based, widened from 16 bits to int32,
 *                strictly increasing) and values as the ctx holds them.
 * The stored points are the longest prefix that satisfies both caps: s <= cap and colptr[s] <= entry_cap.  A point whose entries do not
 * all fit is not stored, and neither is any point behind it; nothing is written at or beyond either cap.  total / total_entries count every
 * held-out point and its entries (dense stores: D per point, and entry_cap is not consulted).
 *
 * Determinism.  No atomics.  The result is a function of the points, the model and the floors alone: the same bits whatever the caps, the
 * cut into uploads, n_valid inside a range, or the budget DPMM_OPT_SCORE_TABLE_MB.  Per range of the table: a class pass leaves one ballot
 * word per wave, the class counts and the 64-bit count of held-out entries of every workgroup of 256 points; one workgroup scans points and
 * entries from running totals kept in device memory and advances them; a gather pass ranks the held-out points of a workgroup from the
 * ballots and copies rows (dense) or, for the sparse store, scans the workgroup's lengths in LDS, writes the colptr slots and copies the
 * entries as one flat range, each output entry finding its column by bisection -- coalesced writes, work balanced whatever the column
 * lengths.  `stored` has one writer: the one workgroup that starts inside both caps and holds a point that does not fit.  Ranges and
 * uploads chain on the ctx stream without a host synchronisation.
 *
 * Limits: the Multinomial prior, every D and point store it takes, K up to DPMM_MAX_CLUSTERS, one ctx.  An NIW ctx is refused
 * (DPMM_EINVAL): it has dpmm_hip_holdout.h.  Only held-out points are collected, no other class; merging a new cluster with an old one is
 * no part of this header or of Predictor.grow_counts.
 *
 * Memory the ctx owns: one 64-bit word per 64 points, four 32-bit and three 64-bit words per 256 points of one range of the score table,
 * eight counters, and with the floor per count 8 bytes per point of one range; allocated by the first call that needs them, freed by
 * dpmm_destroy.  Nothing else of size n.
 */
#ifndef DPMM_HIP_COUNTHOLDOUT_H
#define DPMM_HIP_COUNTHOLDOUT_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    float   *points;         /* dense stores: [cap][D] Float32, point-major and contiguous; NULL for the sparse layout                */
    int64_t *colptr;         /* sparse store: [cap + 1]; NULL for the dense layout                                                   */
    int32_t *rowval;         /* sparse store: [entry_cap]                                                                            */
    float   *val;            /* sparse store: [entry_cap]                                                                            */
    int64_t *index;          /* both: [cap]                                                                                          */
    int64_t  cap;            /* held-out points at most; 0: the points are only counted, every pointer may be NULL                   */
    int64_t  entry_cap;      /* sparse store: entries at most                                                                        */
} dpmm_countholdout_dst;     /* device memory of the ctx's device, checked as dpmm_hip_tensor.h describes */

typedef struct {
    int64_t *total;          /* [1]   held-out points seen since dpmm_countholdout_begin                                      */
    int64_t *total_entries;  /* [1]   their entries (dense stores: D each)                                                    */
    int64_t *stored;         /* [1]   of them written to the destination: the longest prefix inside both caps                 */
    int64_t *stored_entries; /* [1]   the entries of the stored points: dst_colptr[stored]                                    */
    int64_t *skipped;        /* [1]   points with a NaN in their row of parr or M not finite                                  */
    int64_t *incomplete;     /* [1]   points neither skipped nor held out with a value that is not finite                     */
    int64_t *scored;         /* [1]   points that take part: the rest                                                         */
} dpmm_countholdout_out;     /* host memory; every pointer may be NULL */

/* The floor per count of the accumulation dpmm_countstats_begin has just begun: use != 0 holds out every complete point with t_i > 0 and
 * (double)logdens_i < (double)min_logdens_per_count * t_i, beside what the floor of dpmm_countstats_begin holds out; use == 0 switches it
 * off again.  Legal between dpmm_countstats_begin and the first dpmm_countstats_accumulate, else DPMM_ESTATE.  NaN: DPMM_EINVAL.  Without
 * this call nothing new runs and dpmm_countstats_read returns the bits it returned before this header existed. */
int dpmm_countstats_set_per_count(dpmm_ctx *ctx, int use, float min_logdens_per_count);

/* Starts a collection: clears the counters and fixes the floors -- use_floor != 0: points with logdens < min_logdens (min_logdens NaN holds
 * nobody out); use_per_count != 0: the floor per count above; either one holds a point out -- and the destination of every
 * dpmm_countholdout_accumulate that follows (dst == NULL or dst->cap == 0: count only).  dst->points selects the dense layout,
 * dst->colptr the sparse one.  NIW ctx, no floor, a NaN floor per count, cap or entry_cap negative, both or neither layout with cap > 0, a
 * bad pointer: DPMM_EINVAL.  Before dpmm_set_predictive_mult: DPMM_ESTATE. */
int dpmm_countholdout_begin(dpmm_ctx *ctx, int use_floor, float min_logdens, int use_per_count, float min_logdens_per_count, const dpmm_countholdout_dst *dst);

/* Classifies the points 0..n_valid-1 of the ctx's current upload and appends the held-out ones; lo: the global index of point 0 of the
 * upload.  The table is evaluated range by range inside the budget DPMM_OPT_SCORE_TABLE_MB.  n_valid outside 0..n_local, lo < 0 or
 * lo + n_valid beyond 2^62: DPMM_EINVAL.  Without dpmm_countholdout_begin, with another K or other predictive parameters than it saw, or
 * with a destination of the wrong layout for the store that is live: DPMM_ESTATE.  The destination is checked again.  Every refusal comes
 * before any launch.  Returns without waiting for the GPU: the caller's buffers are complete after dpmm_countholdout_read. */
int dpmm_countholdout_accumulate(dpmm_ctx *ctx, int64_t lo, int64_t n_valid);

/* The counters as they stand, written to host memory; reading does not end the collection.  Returns after the ctx stream has been
 * synchronised.  Without dpmm_countholdout_begin: DPMM_ESTATE.  out == NULL: DPMM_EINVAL. */
int dpmm_countholdout_read(dpmm_ctx *ctx, const dpmm_countholdout_out *out);

#ifdef __cplusplus
}
#endif
#endif
