/*
 * dpmm_hip_project.h -- optional companion of dpmm_hip.h: points WIDER than the worker's dimension, projected to it while they are
 * read.  A NIW ctx of dimension D <= DPMM_MAX_DIM_NIW is given a linear map (W [D_in][D], mu [D_in]) once; the projected uploads
 * then read D_in-wide points (device memory of any of the eight element types and any strides, or host Float32 rows) and leave
 * the ctx with y[i][j] = sum_d x[i][d] W[d][j] - (mu' W)[j] as its points.  Additive: DPMM_ABI_VERSION is unchanged.
 *
 * Contract of every call below (that of dpmm_hip_tensor.h)
 *   - all work is queued on the ctx stream and the call returns after that stream has been synchronised.
 *   - every caller DEVICE pointer is checked before anything is launched (hipPointerGetAttributes, hipMemGetAddressRange): device
 *     memory of the ctx's device, aligned for its element type, the whole extent inside its allocation.  A bad argument returns
 *     DPMM_EINVAL, the message names the argument, nothing was launched and the state of the ctx -- the points in force and the
 *     projection included -- is untouched.
 *   - no CPU fallback: without a usable device the calls return DPMM_ENODEVICE.
 * The projected coordinates are read back with dpmm_get_points_device / dpmm_get_points.
 */
#ifndef DPMM_HIP_PROJECT_H
#define DPMM_HIP_PROJECT_H

#include "dpmm_hip_tensor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DPMM_MAX_DIM_PROJECT_IN 4096

/* The projection of the ctx (NIW only; a Multinomial ctx returns DPMM_EINVAL).  W: HOST [D_in][D] row-major, D the ctx's dimension;
 * mu: HOST [D_in] or NULL (zeros).  1 <= D_in <= DPMM_MAX_DIM_PROJECT_IN (larger: DPMM_ELIMIT); D_in = 0 drops the projection (W and
 * mu are ignored).  A non-finite entry of W or of mu returns DPMM_EINVAL; so does an entry of W whose Float32 rounding, or the bf16
 * rounding of that (magnitudes above 3.39e38), is not finite, and a bias mu' W that overflows Float32.  The call forms in
 * Float64 the three bf16 planes of W -- hi, mid and lo of the Float32 rounding of every entry, each the nearest-even bf16 of what the
 * planes before it leave -- and the bias b = mu' W, rounded to Float32, and keeps both on the device.  The projection belongs to the
 * ctx and survives uploads; setting or dropping it does not change the points in force. */
int dpmm_set_projection(dpmm_ctx *ctx, int D_in, const double *W, const double *mu);

/* The shard's points from device memory, projected: element (point i, feature d), i < n_local, d < D_in, sits at
 * d_src + (i * stride_point + d * stride_feature) ELEMENTS, dtype a DPMM_DT_* code, both strides >= 0; the extent checked is
 * (n_local - 1) * stride_point + (D_in - 1) * stride_feature + 1 elements and nothing outside it is read.  Every source value is first
 * rounded to Float32 to nearest even (as dpmm_upload_points_strided_device does); the ctx's point i becomes
 *     y[i][j] = sum_d x[i][d] W[d][j] - b[j]
 * accumulated in Float32 (from +0; b is subtracted once at the end) on the bf16 matrix pipe from exact plane splits: |y - y64| <= (D_in + 8) 2^-24 sum_d |x_d| |W_dj| + 2^-24 |b_j|
 * against the Float64 value of the same Float32 sources.  A point with ANY non-finite feature gets NaN in all D features (the calls
 * downstream skip and count such points).  Point i's value depends on its own features, W and mu only: it is bitwise the same for every
 * n_local, shard and layout.  stride_feature == 1 is read with wide loads where the rows are aligned for them.  Afterwards the ctx is in
 * the state dpmm_upload_points leaves it in for those Float32 values.  Without a projection set: DPMM_EINVAL. */
int dpmm_upload_points_projected_device(dpmm_ctx *ctx, const void *d_src, int dtype, int64_t stride_point, int64_t stride_feature);

/* The same from HOST Float32 rows h_src [n_local][ld_src], ld_src >= D_in: staged in chunks through one device buffer of at most
 * 64 MiB that the ctx keeps and reuses (never n_local * D_in elements), projected by the same kernel. */
int dpmm_upload_points_projected(dpmm_ctx *ctx, const float *h_src, int64_t ld_src);

#ifdef __cplusplus
}
#endif
#endif
