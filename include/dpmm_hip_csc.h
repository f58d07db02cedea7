/*
 * dpmm_hip_csc.h -- optional companion of dpmm_hip.h and dpmm_hip_tensor.h: sparse points (compressed sparse columns, one column per
 * point; Multinomial contexts) out of DEVICE memory the caller owns -- the three arrays of a torch.sparse_csc tensor of shape (D, N) --
 * with no host staging.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * The contract is the one at the top of dpmm_hip_tensor.h: the work is queued on the ctx stream, which is synchronised before the call
 * returns; every caller pointer is checked before anything is launched (device memory of the ctx's device, aligned for its element type,
 * the extent the call addresses inside its allocation), else DPMM_EINVAL naming the argument, nothing launched, the points in force
 * untouched; DPMM_ENODEVICE without a usable device.
 */
#ifndef DPMM_HIP_CSC_H
#define DPMM_HIP_CSC_H

#include "dpmm_hip_tensor.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The shard's points as compressed sparse columns in device memory, read in place.
 *   d_colptr    the shard's first of n_local + 1 offsets, of type index_dtype (DPMM_DT_I32 or DPMM_DT_I64).  The offsets are ABSOLUTE
 *               into d_rowval / d_nzval: the entries of point i are [colptr[i] - index_base, colptr[i + 1] - index_base).  (The host
 *               call dpmm_upload_points_csc rebases on colptr[0]; here a shard or a slab of a larger matrix is d_colptr + lo with the
 *               same two entry pointers, and no offset is read back to slice.)
 *   d_rowval    feature indices, of type index_dtype;  d_nzval: values, of type value_dtype (any DPMM_DT_*)
 *   nnz_extent  elements addressable behind d_rowval and d_nzval (checked against their allocations)
 *   index_base  0 or 1, for colptr and rowval alike
 * Canonical input only, as for the host call: offsets non-decreasing and inside [index_base, index_base + nnz_extent], rows in range and
 * strictly increasing inside a column.  All of it is checked on the device, a column's offsets before any of its entries is addressed;
 * a violation is DPMM_EINVAL, the message names the first offending point ("point i: row index out of range", "point i: row indices
 * are not strictly increasing (unsorted or duplicate)", "colptr decreases at point i", "colptr points outside rowval / nzval at point
 * i") and the points in force stay in force.  Each value is rounded to Float32 to nearest even; a value that is zero after that is not
 * stored.  Afterwards the ctx is in the state dpmm_upload_points_csc leaves for the same matrix.  Temporary device memory: 4 bytes
 * per point (+ 8 per 2048 points).  Errors: DPMM_EINVAL for a context that is not Multinomial, DPMM_ELIMIT for
 * D > DPMM_MAX_DIM_MULT_SPARSE. */
int dpmm_upload_points_csc_device(dpmm_ctx *ctx, const void *d_colptr, int index_dtype, const void *d_rowval, const void *d_nzval,
                                  int value_dtype, int64_t nnz_extent, int index_base);

#ifdef __cplusplus
}
#endif
#endif
