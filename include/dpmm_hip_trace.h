/*
 * dpmm_hip_trace.h -- optional companion of dpmm_hip.h: a trace of label samples kept on the GPU, and what a posterior summary
 * (consensus clustering, per-point confidence) needs of it: contingency tables between pairs of recorded labellings.  Nothing of size
 * n reaches the host per sweep, and no table needs a temporary of size n.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * State needed: labels (dpmm_init_labels, dpmm_set_labels[_device] or a sweep).  Points are not read.
 *
 * Definitions.  A SLOT holds one labelling of the shard: n_local unsigned 16-bit cluster ids z_i, 0-based -- (label_i - 1) of
 * dpmm_get_labels at the moment of dpmm_trace_record -- and the number of clusters K the caller stated for it.  Ids above 65534 are
 * stored as 65535.  Cluster numbers of different slots need not correspond: split, merge and dpmm_remove_empty renumber, and a
 * contingency table does not care.
 *   table of the pair (s, t):  C[a][b] = #{ i < n_local : z_s,i == a and z_t,i == b },  a < K[s], b < K[t].
 * A point whose id is >= K of its slot in either labelling is counted nowhere, as dpmm_contingency ignores it.  Tables are Int64 and
 * sums of integers: the tables of the shards of a data set add up to the table of the whole, in any order, exactly.
 *
 * Memory: the trace (slots rows of n_local ids, each row padded to a multiple of 16 bytes) belongs to the ctx.  dpmm_trace_open
 * allocates it, dpmm_trace_close and dpmm_destroy free it.  The calls below keep a device image of their outputs and of the ratio
 * tables, grown when a call needs more.  All work is queued on the ctx stream.
 */
#ifndef DPMM_HIP_TRACE_H
#define DPMM_HIP_TRACE_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_TRACE_MAX_SLOTS 4096

/* Allocates `slots` empty slots; a trace that is open already is freed first, whatever its size.  n_local == 0 is legal.
 * slots outside 1..DPMM_TRACE_MAX_SLOTS: DPMM_EINVAL. */
int dpmm_trace_open(dpmm_ctx *ctx, int slots);

/* Frees the trace; without one it does nothing. */
int dpmm_trace_close(dpmm_ctx *ctx);

/* Copies the labels in force into `slot` and remembers K for it; a slot in use is overwritten.  One streaming kernel; returns without
 * waiting for the GPU.  Without labels or without dpmm_trace_open: DPMM_ESTATE.  slot outside 0..slots-1 or K outside
 * 1..DPMM_MAX_CLUSTERS: DPMM_EINVAL. */
int dpmm_trace_record(dpmm_ctx *ctx, int slot, int K);

/* pairs: npairs x (s, t) slot numbers; s == t is legal and gives the cluster sizes on the diagonal.  counts: host memory; table p has
 * K[s_p] x K[t_p] cells, counts[off_p + a * K[t_p] + b] = C_p[a][b], off_p the cells of the tables before p: the tables are packed one
 * after another in the order of `pairs`.  The result does not depend on that order, on npairs or on any grid shape.  Returns after the
 * ctx stream has been synchronised.  A pair that names a slot never recorded, or no trace: DPMM_ESTATE.  A slot out of range,
 * npairs < 0 or a null pointer with npairs > 0: DPMM_EINVAL. */
int dpmm_trace_tables(dpmm_ctx *ctx, const int32_t *pairs, int npairs, int64_t *counts);

/* Per local point i, the mean over the listed slots of a table entry chosen by the point's own ids:
 *     out[i] = ( ratio_0[z_anchor,i][z_slots[0],i] + ... + ratio_{nslots-1}[z_anchor,i][z_slots[nslots-1],i] ) / nslots.
 * ratio: host memory, for each listed slot s in order a K[anchor] x K[s] Float32 table, row-major, packed one after another (the
 * posterior summary passes C[a][b] / n_a computed in Float64 from the all-reduced tables and rounded once).  The sum starts from the
 * first term and adds the others in the order listed, in Float32; it is then DIVIDED by (float)nslots, one correctly rounded Float32
 * division.  One thread owns a point: the order is fixed, so the bits are, for any grid shape.  A term whose ids fall outside its
 * table (>= K of the slot) is 0.
 * out_host: host memory [n_local] or NULL.  out_device: device memory [n_local] or NULL, checked as dpmm_hip_tensor.h describes before
 * anything is launched.  Both may be given; both NULL: DPMM_EINVAL, as nslots outside 1..DPMM_TRACE_MAX_SLOTS or a slot out of range.
 * An unrecorded slot: DPMM_ESTATE.  Returns after the ctx stream has been synchronised. */
int dpmm_trace_confidence(dpmm_ctx *ctx, int anchor, const int32_t *slots, int nslots, const float *ratio, float *out_host,
                          void *out_device);

/* The labels of a slot, 1-based Int64 [n_local], to host memory, to device memory (checked as above), or both; both NULL: DPMM_EINVAL.
 * An unrecorded slot: DPMM_ESTATE.  Returns after the ctx stream has been synchronised. */
int dpmm_trace_read(dpmm_ctx *ctx, int slot, int64_t *labels_host, void *labels_device);

#ifdef __cplusplus
}
#endif
#endif
