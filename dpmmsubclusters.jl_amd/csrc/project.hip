// project.hip -- wide points in, the worker's own D <= 256 Float32 image out (include/dpmm_hip_project.h): y[i][j] = sum_d x[i][d] W[d][j] - b[j],
// the one path of a projected fit that scales with N.  The product runs on the bf16 matrix pipe (16x16x32) through the exact plane splits of
// niw_b3.h: W is held as the three bf16 planes of its Float32 rounding, the source is split as its type needs (bfloat16, uint8: one plane,
// exact; float16: two; everything else: the three planes of its Float32 rounding), and the plane products whose indices sum to <= 2 are
// kept -- 3 / 5 / 6 matrix instructions per (16 points, 16 columns, 32 features), the small terms first, accumulated in Float32 from +0; b[j]
// is subtracted once at the end.  (An accumulator that starts at -b[j] rounds every matrix instruction's result on the scale of |b|: with
// |b| >> sum |x||W| that is (3 .. 6) ceil(D_in / 32) roundings of 2^-25 |b|, and the error bound allows 2^-24 |b| for the bias in all --
// half of which its own rounding to Float32 takes.  One subtraction is one such rounding.)
//
//   Operands.  A = W' (rows: 16 output columns, k: 32 features), B = x (columns: 16 points, k: 32 features): lane l of a wave holds the 8
//   features 32 s + 8 (l >> 4) .. + 7 of point l & 15 -- 16 contiguous bytes of a bf16 row, read straight from the source in its own type
//   (no Float32 copy of the source exists anywhere) -- and of the result the 4 columns 16 jb + 4 (l >> 4) .. + 3 of that point: one 16-byte
//   store into the point-major image.
//   W image (host-made, dpmm_set_projection): [k-step s][column block jb < NJB][plane p][lane] 16 bytes, zero for d >= D_in and j >= D, so a
//   k-step's slab is one straight copy into LDS and every fragment read is 64 consecutive 16-byte words (no bank conflict).
//   Tile.  A workgroup (4 waves) owns 64 MB points and all NJB column blocks; a wave holds MB x NJB accumulators (128 registers):
//     D <= 64: NJB 4, MB 8, 512 points;  D <= 128: NJB 8, MB 4, 256 points;  D <= 256: NJB 16, MB 2, 128 points.
//   The workgroup pulls every byte of the W image through L2 exactly once (the slab goes through LDS, shared by its waves).
//   Point i's value is a function of its own features, W and b only: the k-steps and the plane products come in one fixed order, a matrix
//   instruction treats its 16 columns alike, and nothing is accumulated across lanes or workgroups (no atomics).
//   A point with a non-finite feature (after the rounding to Float32) is tested on the SOURCE values and written as NaN in all D columns;
//   columns of B are independent, so its neighbours in the tile are untouched.  Lanes without a point read the shard's last point and
//   store nothing; features >= D_in are never read (the index is not formed) and enter as 0.
#include "dpmm_kernels.h"
#include "niw_b3.h"
#include "tensor_elem.h"

namespace dpmm {

template <typename T> struct proj_planes { static constexpr int n = 3; };
template <> struct proj_planes<bf16_bits> { static constexpr int n = 1; };
template <> struct proj_planes<uint8_t> { static constexpr int n = 1; };
template <> struct proj_planes<f16_bits> { static constexpr int n = 2; };

template <typename T, int BYTES> struct alignas(BYTES) ProjVec { T v[BYTES / sizeof(T)]; };

// the lane's 8 features d0 .. d0 + 7 of one point as Float32.  wide (wave-uniform): every row start is aligned for the vector loads.
template <typename T>
__device__ __forceinline__ void proj_load8(const T *__restrict__ row, int64_t sf, int d0, int D_in, bool wide, float (&v)[8]) {
    if (wide && d0 + 8 <= D_in) {
        constexpr int VB = sizeof(T) * 8 < 16 ? sizeof(T) * 8 : 16;          // bytes per load
        constexpr int PER = VB / sizeof(T), NV = 8 / PER;
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const ProjVec<T, VB> r = *reinterpret_cast<const ProjVec<T, VB> *>(row + d0 + q * PER);
#pragma unroll
            for (int e = 0; e < PER; ++e) v[q * PER + e] = to_f32(r.v[e]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = d0 + e < D_in ? to_f32(row[(int64_t)(d0 + e) * sf]) : 0.f;
    }
}

template <typename T, int NJB>
__global__ __launch_bounds__(PROJ_BLOCK) void project_kernel(float *__restrict__ dst, int64_t ldx, int D, const T *__restrict__ src, int64_t sp, int64_t sf,
                                                             int64_t n, int D_in, const u32x4_t *__restrict__ Wimg, const float *__restrict__ bias, int wide_i) {
    constexpr int MB = 32 / NJB;                 // groups of 16 points per wave
    constexpr int NPX = proj_planes<T>::n;
    constexpr int SLAB = NJB * 3 * 64;           // 16-byte words of a k-step's slab
    __shared__ u32x4_t Ws[SLAB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ci = lane & 15, g = lane >> 4;
    const bool wide = wide_i != 0;
    const int64_t i0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * MB);
    const T *row[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int64_t i = i0 + 16 * m + ci;
        row[m] = src + (i < n ? i : n - 1) * sp;
    }
    f32x4 acc[MB][NJB];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb)
#pragma unroll
        for (int m = 0; m < MB; ++m) acc[m][jb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    bool bad[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) bad[m] = false;

    const int ksteps = (D_in + 31) >> 5;
    for (int s = 0; s < ksteps; ++s) {
        // this k-step's B operands: the source values, tested, split into planes
        u32x4_t Z[MB][NPX];
        const int d0 = 32 * s + 8 * g;
#pragma unroll
        for (int m = 0; m < MB; ++m) {
            float v[8];
            proj_load8(row[m], sf, d0, D_in, wide, v);
            uint32_t P[3][4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bad[m] = bad[m] || !(__builtin_fabsf(v[2 * e]) < INFINITY) || !(__builtin_fabsf(v[2 * e + 1]) < INFINITY);
                b3_split_pair(v[2 * e], v[2 * e + 1], P[0][e], P[1][e], P[2][e]);
            }
#pragma unroll
            for (int p = 0; p < NPX; ++p) Z[m][p] = (u32x4_t){P[p][0], P[p][1], P[p][2], P[p][3]};
        }
        __syncthreads();                         // the previous k-step's fragment reads are done
        {
            const u32x4_t *G = Wimg + (size_t)s * SLAB;
#pragma unroll
            for (int q = 0; q < SLAB / PROJ_BLOCK; ++q) Ws[q * PROJ_BLOCK + tid] = G[q * PROJ_BLOCK + tid];
        }
        __syncthreads();
#pragma unroll
        for (int jb = 0; jb < NJB; ++jb) {
            u32x4_t A[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) A[p] = Ws[(jb * 3 + p) * 64 + lane];
#pragma unroll
            for (int m = 0; m < MB; ++m) {
                f32x4 a = acc[m][jb];
                // plane products (W plane, x plane) with index sum <= 2, small terms first: niw_b3.h's order, the absent planes of x left out
                auto mf = [&](int pw, int px) {
                    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, A[pw]), __builtin_bit_cast(bf16x8_t, Z[m][px < NPX ? px : 0]), a, 0, 0, 0);
                };
                mf(2, 0);
                if constexpr (NPX == 3) mf(0, 2);
                if constexpr (NPX >= 2) mf(1, 1);
                mf(1, 0);
                if constexpr (NPX >= 2) mf(0, 1);
                mf(0, 0);
                acc[m][jb] = a;
            }
        }
    }
    const float qnan = __uint_as_float(0x7fc00000u);
    f32x4 b4[NJB];
#pragma unroll
    for (int jb = 0; jb < NJB; ++jb) b4[jb] = *reinterpret_cast<const f32x4 *>(bias + 16 * jb + 4 * g);
#pragma unroll
    for (int m = 0; m < MB; ++m) {
        const int64_t i = i0 + 16 * m + ci;
        const bool b = (__ballot(bad[m]) >> ci & 0x0001000100010001ull) != 0ull;      // any of the four lanes that hold features of this point
        if (i < n) {
#pragma unroll
            for (int jb = 0; jb < NJB; ++jb) {
                const int j = 16 * jb + 4 * g;
                if (j < ldx) {
                    f32x4 o = acc[m][jb] - b4[jb];          // ONE rounding on the bias' scale (see the head of the file)
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = j + e < D ? (b ? qnan : o[e]) : 0.f;
                    *reinterpret_cast<f32x4 *>(dst + i * ldx + j) = o;
                }
            }
        }
    }
}

int proj_njb(int D) { return D <= 64 ? 4 : D <= 128 ? 8 : 16; }
int proj_tile_points(int D) { return 64 * (32 / proj_njb(D)); }

template <typename T>
static hipError_t launch_project_t(float *dst, int64_t ldx, int D, const void *src, int64_t sp, int64_t sf, int64_t n, int D_in, const void *Wimg,
                                   const float *bias, hipStream_t s) {
    const T *p = static_cast<const T *>(src);
    constexpr size_t VB = sizeof(T) * 8 < 16 ? sizeof(T) * 8 : 16;
    const int wide = sf == 1 && D_in >= 8 && reinterpret_cast<uintptr_t>(src) % VB == 0 && ((size_t)sp * sizeof(T)) % VB == 0;
    const int njb = proj_njb(D);
    const int64_t tile = proj_tile_points(D);
    const dim3 grid((unsigned)((n + tile - 1) / tile)), block(PROJ_BLOCK);
    const u32x4_t *W = static_cast<const u32x4_t *>(Wimg);
    if (njb == 4) DPMM_LAUNCH((project_kernel<T, 4>), grid, block, 0, s, dst, ldx, D, p, sp, sf, n, D_in, W, bias, wide);
    else if (njb == 8) DPMM_LAUNCH((project_kernel<T, 8>), grid, block, 0, s, dst, ldx, D, p, sp, sf, n, D_in, W, bias, wide);
    else DPMM_LAUNCH((project_kernel<T, 16>), grid, block, 0, s, dst, ldx, D, p, sp, sf, n, D_in, W, bias, wide);
    return hipGetLastError();
}

hipError_t launch_project(float *dst, int64_t ldx, int D, const void *src, int dtype, int64_t sp, int64_t sf, int64_t n, int D_in, const void *Wimg,
                          const float *bias, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    switch (dtype) {
        case 0: return launch_project_t<f16_bits>(dst, ldx, D, src, sp, sf, n, D_in, Wimg, bias, s);
        case 1: return launch_project_t<bf16_bits>(dst, ldx, D, src, sp, sf, n, D_in, Wimg, bias, s);
        case 2: return launch_project_t<float>(dst, ldx, D, src, sp, sf, n, D_in, Wimg, bias, s);
        case 3: return launch_project_t<double>(dst, ldx, D, src, sp, sf, n, D_in, Wimg, bias, s);
        case 4: return launch_project_t<uint8_t>(dst, ldx, D, src, sp, sf, n, D_in, Wimg, bias, s);
        case 5: return launch_project_t<int16_t>(dst, ldx, D, src, sp, sf, n, D_in, Wimg, bias, s);
        case 6: return launch_project_t<int32_t>(dst, ldx, D, src, sp, sf, n, D_in, Wimg, bias, s);
        case 7: return launch_project_t<int64_t>(dst, ldx, D, src, sp, sf, n, D_in, Wimg, bias, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace dpmm
