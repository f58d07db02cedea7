// tensor_elem.h -- the eight element types of caller-owned device memory (DPMM_DT_*, include/dpmm_hip_tensor.h) and their conversion to
// Float32.  One definition for every kernel that reads such memory (tensor_io.hip, csc_io.hip): the rounding is the same code.
#pragma once
#include "dpmm_kernels.h"

namespace dpmm {

// ---- element types: each converts ONE element to Float32 exactly as the host conversions do
struct f16_bits { uint16_t u; };
struct bf16_bits { uint16_t u; };

__device__ __forceinline__ float to_f32(f16_bits h) {      // integer arithmetic only: independent of the wave's denormal mode
    const uint32_t s = ((uint32_t)h.u & 0x8000u) << 16, e = (h.u >> 10) & 0x1Fu, m = h.u & 0x3FFu;
    if (e == 0u) {                                          // +-0 and the subnormals m * 2^-24 (exact: m < 2^10, the product is a normal Float32)
        const float v = (float)m * 0x1p-24f;
        return __uint_as_float(__float_as_uint(v) | s);
    }
    if (e == 31u) return __uint_as_float(s | 0x7F800000u | (m << 13));      // +-Inf, NaN (payload kept)
    return __uint_as_float(s | ((e + 112u) << 23) | (m << 13));
}
__device__ __forceinline__ float to_f32(bf16_bits h) { return __uint_as_float((uint32_t)h.u << 16); }
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(double v) { return (float)v; }       // v_cvt_f32_f64: round to nearest even
__device__ __forceinline__ float to_f32(uint8_t v) { return (float)v; }
__device__ __forceinline__ float to_f32(int16_t v) { return (float)v; }
__device__ __forceinline__ float to_f32(int32_t v) { return (float)v; }      // v_cvt_f32_i32: round to nearest even
__device__ __forceinline__ float to_f32(int64_t v) { return (float)v; }      // (the compiler's Int64 sequence rounds once, to nearest even)

}  // namespace dpmm
