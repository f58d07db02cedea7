// project_image.h -- host side of dpmm_set_projection (include/dpmm_hip_project.h): the bf16 plane image of W and the bias, formed in
// Float64 / exact Float32 arithmetic.  Plain C++ with no HIP in it, so that a stand-alone program can exercise it on a CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace dpmm {

// nearest-even bf16 of a finite Float32 (the rounding of v_cvt_pk_bf16_f32, which niw_b3.h's b3_split_pair uses on the device)
inline uint16_t proj_bf16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float proj_bf16_value(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
// hi, mid, lo of the Float32 w: each plane the bf16 of what the planes before it leave (both remainders are exact in Float32)
inline void proj_split3(float w, uint16_t (&p)[3]) {
    p[0] = proj_bf16_rne(w);
    const float r = w - proj_bf16_value(p[0]);
    p[1] = proj_bf16_rne(r);
    const float s = r - proj_bf16_value(p[1]);
    p[2] = proj_bf16_rne(s);
}

// img: [ceil(D_in / 32)][njb][3][64 lanes][8] bf16 -- lane l, element e: W[32 s + 8 (l >> 4) + e][16 jb + (l & 15)], zero outside [D_in][D];
// bias: [16 njb], (float)(mu' W)[j], +0 for j >= D.
// Returns 0, or 1 / 2 / 3: a non-finite entry of W / of mu / of the bias; *where = its index.
inline int proj_build_image(int D_in, int D, int njb, const double *W, const double *mu, std::vector<uint16_t> &img, std::vector<float> &bias,
                            int64_t *where) {
    const int ksteps = (D_in + 31) / 32;
    img.assign((size_t)ksteps * njb * 3 * 64 * 8, 0);
    bias.assign((size_t)16 * njb, 0.f);
    for (int d = 0; d < D_in; ++d) {
        if (mu && !std::isfinite(mu[d])) { *where = d; return 2; }
        for (int j = 0; j < D; ++j) {
            const double w = W[(size_t)d * D + j];
            const float w32 = (float)w;
            if (!std::isfinite(w) || !std::isfinite(w32)) { *where = (int64_t)d * D + j; return 1; }
            uint16_t p[3];
            proj_split3(w32, p);
            if (!std::isfinite(proj_bf16_value(p[0]))) { *where = (int64_t)d * D + j; return 1; }      // (beyond the largest bf16)
            const int s = d >> 5, g = (d & 31) >> 3, e = d & 7, jb = j >> 4, lane = 16 * g + (j & 15);
            for (int q = 0; q < 3; ++q) img[((((size_t)s * njb + jb) * 3 + q) * 64 + lane) * 8 + e] = p[q];
        }
    }
    for (int j = 0; j < D; ++j) {
        double b = 0.0;
        if (mu) for (int d = 0; d < D_in; ++d) b += mu[d] * W[(size_t)d * D + j];
        const float b32 = (float)b;
        if (!std::isfinite(b32)) { *where = j; return 3; }
        bias[j] = b32;
    }
    return 0;
}

}  // namespace dpmm
