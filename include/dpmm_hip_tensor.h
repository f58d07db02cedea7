/*
 * dpmm_hip_tensor.h -- optional companion of dpmm_hip.h: points, labels and predictions in and out of DEVICE memory the
 * caller owns (a torch tensor, a buffer of another HIP library), with no host staging.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * Contract of every call below
 *   - all work is queued on the ctx stream and the call returns after that stream has been synchronised: the caller's memory may
 *     be reused, freed or read from any stream afterwards.  The caller must have FINISHED producing an input before the call
 *     (synchronise the producing stream first); there is no event plumbing between foreign streams.
 *   - every caller pointer is checked before anything is launched: it must be device memory of the ctx's device
 *     (hipPointerGetAttributes), aligned for its element type, and the whole extent the call addresses must lie inside the
 *     allocation it belongs to (hipMemGetAddressRange).  Otherwise the call returns DPMM_EINVAL, the message names the argument,
 *     nothing was launched and the state of the ctx -- the points in force included -- is untouched.
 *   - no CPU fallback: without a usable device the calls return DPMM_ENODEVICE.
 */
#ifndef DPMM_HIP_TENSOR_H
#define DPMM_HIP_TENSOR_H

#include "dpmm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* element types of dpmm_upload_points_strided_device */
enum {
    DPMM_DT_F16 = 0,  /* IEEE binary16 */
    DPMM_DT_BF16 = 1, /* bfloat16 */
    DPMM_DT_F32 = 2,
    DPMM_DT_F64 = 3,
    DPMM_DT_U8 = 4,
    DPMM_DT_I16 = 5,
    DPMM_DT_I32 = 6,
    DPMM_DT_I64 = 7
};

/* The shard's points from device memory in the type and layout they have: element (point i, feature d), i < n_local, d < D, sits at
 * d_src + (i * stride_point + d * stride_feature) ELEMENTS; both strides >= 0 (0: the element is shared, torch's `expand`).  The ctx
 * keeps its own Float32 image (point-major); the value stored is the source value rounded to Float32, to nearest
 * even -- what numpy's astype(float32) and torch's .float() give.  NaN stays NaN (nan_to_zero != 0: NaN -> 0, as
 * dpmm_upload_points_npy), +-Inf, -0 and subnormals are kept.  stride_feature == 1 (an (N, D) tensor) and stride_point == 1 (a
 * contiguous (D, N) tensor) are read and written coalesced; any other pair of strides is a gather.  The extent checked is
 * (n_local - 1) * stride_point + (D - 1) * stride_feature + 1 elements from d_src.  Afterwards the ctx is in the state
 * dpmm_upload_points leaves it in for the same values (a Multinomial ctx finds its byte path, parameters in force are re-packed,
 * sparse points are replaced). */
int dpmm_upload_points_strided_device(dpmm_ctx *ctx, const void *d_src, int dtype, int64_t stride_point, int64_t stride_feature,
                                      int nan_to_zero);

/* The points in force as Float32 rows: d_out [n_local][ld_out], ld_out >= D, columns [D, ld_out) are written as 0.  Whatever storage the
 * ctx holds them in: the Float32 image, the byte copy of a Multinomial ctx with counts in [0, 255] (widened), or compressed sparse
 * columns (scattered into zeros). */
int dpmm_get_points_device(dpmm_ctx *ctx, float *d_out, int64_t ld_out);

/* dpmm_get_labels / dpmm_set_labels with device vectors [n_local] (Int64, 1-based).  get: either may be NULL.  set: as dpmm_set_labels
 * (the first call must give both). */
int dpmm_get_labels_device(dpmm_ctx *ctx, int64_t *d_labels, int64_t *d_sub);
int dpmm_set_labels_device(dpmm_ctx *ctx, const int64_t *d_labels, const int64_t *d_sub);

/* dpmm_predict_points into device memory: d_labels [n_local] Int64 1-based, d_probs [n_local][K] Float32 row-major (may be NULL). */
int dpmm_predict_points_device(dpmm_ctx *ctx, int64_t *d_labels, float *d_probs);

#ifdef __cplusplus
}
#endif
#endif
