/*
 * dpmm_hip_countstats.h -- optional companion of dpmm_hip.h: the per-cluster sufficient statistics of a batch of count data under the
 * Multinomial model the ctx serves, N[k] = sum_i w_ik and sums[k][d] = sum_i w_ik x_id, accumulated on the GPU in Float64 while the table
 * that the label rule evaluates anyway goes by.  They are what the conjugate Dirichlet update alpha' = alpha + sums needs to fold the
 * batch into the posterior (host/absorb.py: dirichlet_absorb).  The answer is K * (D + 1) doubles; temporary memory does not grow with n
 * or with the number of stored entries and nothing of size n reaches the host.  The NIW counterpart is dpmm_hip_batchstats.h, whose
 * conventions and mode constants this header keeps.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: a Multinomial ctx, the points -- from any of its upload calls: dense host memory, dpmm_upload_points_strided_device,
 * dpmm_upload_points_csc, dpmm_upload_points_csc_device -- and dpmm_set_predictive_mult.  All three point stores are read where they
 * lie: the Float32 matrix, the lossless byte copy a ctx keeps INSTEAD of it when every value is an integer in 0..255, and the
 * compressed sparse columns.
 *
 * Definitions.  parr[k][i], labels, M, S, logdens and probs are exactly those of dpmm_hip_score.h, formed by the same device code
 * (score_device.h) from the table the Multinomial kernels' table mode writes; the sparse store keeps its convention that a feature a
 * point does not store contributes nothing.  Every point 0 .. n_valid - 1 is in exactly one class:
 *   skipped      a NaN in its row of parr, or M not finite (the rule of dpmm_hip_overlap.h / dpmm_hip_batchstats.h); else
 *   held out     use_floor != 0 and logdens_i < min_logdens, logdens_i the Float32 value dpmm_score_points writes; or the floor
 *                per count of include/dpmm_hip_countholdout.h, when it has been set, holds the point out; else
 *   incomplete   one of its values is not finite: of the D features of its row (Float32 store), of its stored values (sparse store);
 *                a point of the byte store never is; else
 *   takes part   and is counted in count[k], k + 1 its label.
 * Only points that take part add to the sums, with the weights
 *   DPMM_BATCHSTATS_HARD   w_ik = 1 if labels_i == k + 1, else 0
 *   DPMM_BATCHSTATS_SOFT   w_ik = (double)p_ik, p_ik the Float32 value probs[i][k], bit-identical to what dpmm_score_points writes
 *   N[k]          sum_i w_ik
 *   sums[k][d]    sum_i w_ik x_id
 * in Float64.  w_ik x_id is the product of two Float32 values and exact in Float64 (24 + 24 bits); it is formed there, never in Float32.
 * In HARD mode N[k] == count[k] exactly.  A sparse point without entries is a legitimate point: it adds to N and count and to no feature.
 *
 * Exactness.  In HARD mode, when every value that takes part is an integer and every true sum is below 2^53, every addition is exact:
 * sums and N are the true sums, identical to the bit whatever the capacity, the table budget, the store or the order of the points.
 * This always holds for the byte store.
 *
 * Error bound otherwise.  With T1[k][d] = sum_i w_ik |x_id|, u = 2^-53 and gamma(m) = m u / (1 - m u): a term is exact and passes
 * through fewer than n additions, whatever their order and whether or not product and addition are fused, so
 * |sums - exact| <= gamma(n) T1 and |N - exact| <= gamma(n) N.  Two such evaluations -- this one and a caller's -- agree within
 * 2 gamma(n + 2) times T1 and N (the bound dpmm_hip_batchstats.h derives for its `sums`).
 *
 * Determinism.  The same points, the same cuts into uploads and the same DPMM_OPT_SCORE_TABLE_MB give the same bits on every run: no
 * floating-point atomics anywhere; a range of the table is cut into chunks whose number depends on the range's length, K, D and the kind
 * of store alone -- never on the number of stored entries; inside a chunk the points with w_ik != 0 are taken in increasing i; every
 * partial sum has one writer -- dense and byte stores: a workgroup per (chunk, 16 clusters, 256 features) on the Float64 matrix pipe;
 * sparse store: a wave per (chunk, cluster, 1792 features) with its accumulators in LDS -- and the chunks are added in increasing
 * order.  Across other cuts or budgets the results agree within the bound (HARD on integers: to the bit); the counters are equal.
 *
 * Limits: the Multinomial prior, every D and point store it takes, K up to DPMM_MAX_CLUSTERS.  An NIW ctx is refused (DPMM_EINVAL): its
 * statistics are those of dpmm_hip_batchstats.h.
 *
 * Memory: the accumulators (K * (D + 1) doubles, 8 * (K + 3) counters), two floats per point of one range of the score table and the
 * chunk partials -- rows of D doubles (dense stores: D rounded up to 256), at most DPMM_COUNTSTATS_PARTIAL_BYTES of them, 64 MiB as for
 * the NIW statistics, plus one double per row: at D = 65536 a row is 512 KiB, so 128 (chunk, cluster) rows still fit and no larger cap is
 * needed; when K rows do not fit, the clusters are taken in groups -- belong to the ctx; dpmm_countstats_begin allocates them (grown
 * when a call needs more, freed by dpmm_destroy), accumulate and read allocate nothing beyond the score table of dpmm_hip_score.h: a
 * second pass of the same shape allocates nothing.  Accumulators that cannot be allocated are an ordinary failure of
 * dpmm_countstats_begin (DPMM_EHIP, dpmm_last_error names the buffer), before any launch.
 */
#ifndef DPMM_HIP_COUNTSTATS_H
#define DPMM_HIP_COUNTSTATS_H

#include "dpmm_hip.h"
#include "dpmm_hip_batchstats.h"      /* DPMM_BATCHSTATS_HARD, DPMM_BATCHSTATS_SOFT */

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_COUNTSTATS_PARTIAL_BYTES (64 << 20)

typedef struct {
    double  *N;              /* [K]        sum_i w_ik over the points that take part                                 */
    double  *sums;           /* [K][D]     sum_i w_ik x_id                                                           */
    int64_t *count;          /* [K]        points that take part with labels == k + 1                                */
    int64_t *skipped;        /* [1]        points with a NaN in their row of parr or M not finite                    */
    int64_t *incomplete;     /* [1]        points neither skipped nor held out with a value that is not finite       */
    int64_t *held_out;       /* [1]        points not skipped with logdens < min_logdens (use_floor != 0)            */
} dpmm_countstats_out;       /* host memory; every pointer may be NULL */

/* Starts an accumulation: clears the ctx-owned N, sums and counters and fixes the weights (mode) and the floor (use_floor != 0:
 * points with logdens < min_logdens are held out; min_logdens NaN holds nobody out) of every dpmm_countstats_accumulate that follows.
 * NIW ctx, another mode than DPMM_BATCHSTATS_HARD / _SOFT: DPMM_EINVAL.  Before dpmm_set_predictive_mult: DPMM_ESTATE. */
int dpmm_countstats_begin(dpmm_ctx *ctx, int mode, int use_floor, float min_logdens);

/* Adds the points 0..n_valid-1 of the ctx's current upload; points at or beyond n_valid are ignored (the zero padding of a short
 * slab is a perfectly good point of some cluster).  The table is evaluated range by range inside the budget DPMM_OPT_SCORE_TABLE_MB,
 * as dpmm_score_points does.  n_valid outside 0..n_local: DPMM_EINVAL.  Without dpmm_countstats_begin, or with another K or other
 * predictive parameters than it saw: DPMM_ESTATE.  Every refusal comes before any launch.  Returns without waiting for the GPU. */
int dpmm_countstats_accumulate(dpmm_ctx *ctx, int64_t n_valid);

/* The sums as they stand, written to host memory; reading does not end the accumulation.  Returns after the ctx stream has been
 * synchronised.  Without dpmm_countstats_begin: DPMM_ESTATE.  out == NULL: DPMM_EINVAL. */
int dpmm_countstats_read(dpmm_ctx *ctx, const dpmm_countstats_out *out);

#ifdef __cplusplus
}
#endif
#endif
