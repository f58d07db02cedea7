// tensor_io.hip -- points in and out of caller-owned DEVICE memory (include/dpmm_hip_tensor.h): any of eight element types, any
// non-negative strides in, Float32 rows out.  All kernels are elementwise and HBM-bound; index arithmetic is Int64 throughout
// (n * ldx passes 2^31 at N = 1e7, D = 64).
//
//   ingest_strided_kernel<T, MODE>   source element (point i, feature d) at src[i * sp + d * sf]  ->  the ctx image dX[n][ldx] (Float32,
//                                    ldx = roundup(D, 4), pad columns written as 0 here).  The value is the source value rounded to
//                                    Float32 to nearest even (what numpy's astype(float32) / torch's .float() give); NaN stays NaN
//                                    (nan_to_zero: NaN -> 0, the rule of ingest_rows_kernel, labels.hip), +-Inf, -0 and subnormals are kept.
//       INGEST_POINT_MAJOR    sf == 1 and every group of four features of a point is a naturally aligned vector: lanes run along the
//                             features (and on into the next point: with sp == D a wave's read is one contiguous run), one vector
//                             read of four elements and one 16-byte write per lane.
//       INGEST_FEATURE_MAJOR  sp == 1: a tile of 64 points x 64 features goes through LDS -- read with lanes along the points (a feature's
//                             64 points are contiguous), written with lanes along the features (a point's row is contiguous).
//       INGEST_GENERAL        anything else (steps, stride 0, a point-major source that is not vector aligned): a gather, lanes along the
//                             features; correct for every stride pair, coalesced only where sf == 1.
//   points_readback_kernel           the points in force -> out[n][ld_out] Float32 (columns [D, ld_out) = 0): from the Float32 image, or
//                                    widened from the byte copy of a byte-path Multinomial context (mult_sweep.hip u8_convert_kernel);
//   sparse_readback_kernel           ... or the stored entries of sparse points (mult_sparse.hip) scattered into the zero-filled image.
#include "dpmm_kernels.h"
#include "tensor_elem.h"

namespace dpmm {

template <typename T>
__device__ __forceinline__ float ingest_value(T raw, int nan_to_zero) {
    float v = to_f32(raw);
    if (nan_to_zero && v != v) v = 0.f;
    return v;
}

template <typename T>
struct alignas(sizeof(T) * 4 < 16 ? sizeof(T) * 4 : 16) Vec4 { T v[4]; };

constexpr int TIO_BLOCK = 256;
constexpr int TIO_TILE = 64;              // points and features of a transposed tile
constexpr int TIO_PITCH = TIO_TILE + 1;   // floats per LDS row.  Phase 1 (ds_write_b32, lanes along points p, one feature f): word p * 65 + f, bank
                                          // (p + f) % 32 -- the 32 lanes of a half wave hit 32 banks.  Phase 2 (ds_read_b32, lanes along f, one p):
                                          // consecutive words.  Neither phase has a conflict.

// MODE INGEST_POINT_MAJOR / INGEST_GENERAL: one thread per group of four output columns; the grid-stride loop carries (point, column group)
// instead of dividing in every round.  MODE INGEST_FEATURE_MAJOR: tiles of 64 points x 64 features through LDS, a grid-stride loop over tiles.
template <typename T, int MODE>
__global__ __launch_bounds__(TIO_BLOCK) void ingest_strided_kernel(float *__restrict__ dst, int64_t ldx, const T *__restrict__ src, int64_t sp,
                                                                   int64_t sf, int64_t n, int D, int nan_to_zero) {
    if constexpr (MODE == INGEST_FEATURE_MAJOR) {
        __shared__ float tile[TIO_TILE * TIO_PITCH];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;      // four waves
        const int64_t ptiles = (n + TIO_TILE - 1) / TIO_TILE;
        const int ftiles = (D + TIO_TILE - 1) / TIO_TILE;
        const int64_t tiles = ptiles * ftiles;
        constexpr int PER = TIO_TILE / 4;                                 // features (phase 1) / points (phase 2) per wave
        for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int64_t pt = t / ftiles;
            const int f0 = (int)(t - pt * ftiles) * TIO_TILE;
            const int64_t i0 = pt * TIO_TILE;
            const int np = (int)(n - i0 < TIO_TILE ? n - i0 : TIO_TILE);
            const int nf = D - f0 < TIO_TILE ? D - f0 : TIO_TILE;
            // phase 1: lane = point, this wave's features wave, wave + 4, ...; all reads are issued before the first LDS write
            T r[PER];
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int f = wave + 4 * j;
                r[j] = (lane < np && f < nf) ? src[(int64_t)(f0 + f) * sf + i0 + lane] : T{};
            }
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int f = wave + 4 * j;
                if (lane < np && f < nf) tile[lane * TIO_PITCH + f] = ingest_value(r[j], nan_to_zero);
            }
            __syncthreads();
            // phase 2: lane = feature, this wave's points wave, wave + 4, ...: exactly the words phase 1 wrote are read; the columns
            // [D, ldx) behind the last feature tile are written as 0
            const int nw = (int)((f0 + TIO_TILE >= D ? ldx : (int64_t)(f0 + TIO_TILE)) - f0);      // columns this tile writes
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int p = wave + 4 * j;
                if (p < np && lane < nw) dst[(i0 + p) * ldx + f0 + lane] = lane < nf ? tile[p * TIO_PITCH + lane] : 0.f;
            }
            __syncthreads();
        }
    } else {
        const int64_t W = ldx >> 2;                                       // column groups per point
        const int64_t step = (int64_t)gridDim.x * TIO_BLOCK;
        const int64_t q0 = (int64_t)blockIdx.x * TIO_BLOCK + threadIdx.x;
        const int64_t di = step / W, dc = step - di * W;
        int64_t i = q0 / W, c = q0 - i * W;
        while (i < n) {
            const int d0 = (int)(c << 2);
            float o[4];
            if (MODE == INGEST_POINT_MAJOR && d0 + 4 <= D) {
                const Vec4<T> r = *reinterpret_cast<const Vec4<T> *>(src + i * sp + d0);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = ingest_value(r.v[j], nan_to_zero);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = d0 + j < D ? ingest_value(src[i * sp + (int64_t)(d0 + j) * sf], nan_to_zero) : 0.f;
            }
            *reinterpret_cast<float4 *>(dst + i * ldx + d0) = make_float4(o[0], o[1], o[2], o[3]);
            i += di; c += dc;
            if (c >= W) { c -= W; i += 1; }
        }
    }
}

static inline int tio_grid(int64_t items) {
    int64_t g = (items + TIO_BLOCK - 1) / TIO_BLOCK;
    if (g > 256 * 16) g = 256 * 16;
    if (g < 1) g = 1;
    return (int)g;
}

template <typename T>
static hipError_t launch_ingest_t(float *dst, int64_t ldx, const void *src, int64_t sp, int64_t sf, int64_t n, int D, int nan_to_zero, int mode,
                                  hipStream_t s) {
    const T *p = static_cast<const T *>(src);
    if (mode == INGEST_FEATURE_MAJOR) {
        const int64_t tiles = ((n + TIO_TILE - 1) / TIO_TILE) * ((D + TIO_TILE - 1) / TIO_TILE);
        const int grid = (int)(tiles < 256 * 16 ? tiles : 256 * 16);
        DPMM_LAUNCH((ingest_strided_kernel<T, INGEST_FEATURE_MAJOR>), dim3(grid), dim3(TIO_BLOCK), 0, s, dst, ldx, p, sp, sf, n, D, nan_to_zero);
    } else if (mode == INGEST_POINT_MAJOR) {
        DPMM_LAUNCH((ingest_strided_kernel<T, INGEST_POINT_MAJOR>), dim3(tio_grid(n * (ldx >> 2))), dim3(TIO_BLOCK), 0, s, dst, ldx, p, sp, sf, n, D,
                    nan_to_zero);
    } else {
        DPMM_LAUNCH((ingest_strided_kernel<T, INGEST_GENERAL>), dim3(tio_grid(n * (ldx >> 2))), dim3(TIO_BLOCK), 0, s, dst, ldx, p, sp, sf, n, D,
                    nan_to_zero);
    }
    return hipGetLastError();
}

size_t ingest_elem_size(int dtype) {
    switch (dtype) {
        case 0: case 1: case 5: return 2;
        case 2: case 6: return 4;
        case 3: case 7: return 8;
        case 4: return 1;
        default: return 0;
    }
}

int ingest_mode(const void *src, int dtype, int64_t sp, int64_t sf, int64_t n, int D) {
    const size_t es = ingest_elem_size(dtype);
    const size_t va = es * 4 < 16 ? es * 4 : 16;                      // alignment of Vec4<T>
    if (sf == 1 && D >= 4 && (reinterpret_cast<uintptr_t>(src) % va) == 0 && ((size_t)sp * es) % va == 0) return INGEST_POINT_MAJOR;
    if (sp == 1 && n > 1) return INGEST_FEATURE_MAJOR;
    return INGEST_GENERAL;
}

hipError_t launch_ingest_strided(float *dst, int64_t ldx, const void *src, int dtype, int64_t sp, int64_t sf, int64_t n, int D, int nan_to_zero,
                                 hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int mode = ingest_mode(src, dtype, sp, sf, n, D);
    switch (dtype) {
        case 0: return launch_ingest_t<f16_bits>(dst, ldx, src, sp, sf, n, D, nan_to_zero, mode, s);
        case 1: return launch_ingest_t<bf16_bits>(dst, ldx, src, sp, sf, n, D, nan_to_zero, mode, s);
        case 2: return launch_ingest_t<float>(dst, ldx, src, sp, sf, n, D, nan_to_zero, mode, s);
        case 3: return launch_ingest_t<double>(dst, ldx, src, sp, sf, n, D, nan_to_zero, mode, s);
        case 4: return launch_ingest_t<uint8_t>(dst, ldx, src, sp, sf, n, D, nan_to_zero, mode, s);
        case 5: return launch_ingest_t<int16_t>(dst, ldx, src, sp, sf, n, D, nan_to_zero, mode, s);
        case 6: return launch_ingest_t<int32_t>(dst, ldx, src, sp, sf, n, D, nan_to_zero, mode, s);
        case 7: return launch_ingest_t<int64_t>(dst, ldx, src, sp, sf, n, D, nan_to_zero, mode, s);
        default: return hipErrorInvalidValue;
    }
}

// ---- read-back
// X != null: the Float32 image; else X8 != null: the byte copy; else: zeros (the canvas the sparse entries are scattered into)
__global__ __launch_bounds__(TIO_BLOCK) void points_readback_kernel(float *__restrict__ out, int64_t ld_out, const float *__restrict__ X, int64_t ldx,
                                                                    const uint8_t *__restrict__ X8, int64_t ld8, int64_t n, int D) {
    const int64_t step = (int64_t)gridDim.x * TIO_BLOCK;
    const int64_t q0 = (int64_t)blockIdx.x * TIO_BLOCK + threadIdx.x;
    const int64_t di = step / ld_out, dc = step - di * ld_out;
    int64_t i = q0 / ld_out, d = q0 - i * ld_out;
    while (i < n) {
        float v = 0.f;
        if (d < D) {
            if (X) v = X[i * ldx + d];
            else if (X8) v = (float)X8[i * ld8 + d];
        }
        out[i * ld_out + d] = v;
        i += di; d += dc;
        if (d >= ld_out) { d -= ld_out; i += 1; }
    }
}

// one wave per point: lanes over the point's stored entries
__global__ __launch_bounds__(TIO_BLOCK) void sparse_readback_kernel(float *__restrict__ out, int64_t ld_out, const int64_t *__restrict__ cp,
                                                                    const uint16_t *__restrict__ ri, const float *__restrict__ val, int64_t n) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (TIO_BLOCK / 64);
    for (int64_t i = (int64_t)blockIdx.x * (TIO_BLOCK / 64) + (threadIdx.x >> 6); i < n; i += waves) {
        const int64_t a = cp[i], b = cp[i + 1];
        for (int64_t e = a + lane; e < b; e += 64) out[i * ld_out + ri[e]] = val[e];
    }
}

hipError_t launch_points_readback(float *out, int64_t ld_out, const float *X, int64_t ldx, const uint8_t *X8, int64_t ld8, int64_t n, int D,
                                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    DPMM_LAUNCH(points_readback_kernel, dim3(tio_grid(n * ld_out)), dim3(TIO_BLOCK), 0, s, out, ld_out, X, ldx, X8, ld8, n, D);
    return hipGetLastError();
}

hipError_t launch_sparse_readback(float *out, int64_t ld_out, const int64_t *cp, const uint16_t *ri, const float *val, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    DPMM_LAUNCH(sparse_readback_kernel, dim3(tio_grid(n * 64)), dim3(TIO_BLOCK), 0, s, out, ld_out, cp, ri, val, n);
    return hipGetLastError();
}

}  // namespace dpmm
