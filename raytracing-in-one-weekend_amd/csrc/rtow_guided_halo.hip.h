// rtow_guided_halo.hip.h - the neighbourhood statistic rtowEstimateMomentsDevice and rtowRectifyHistoryDevice share (rtow_moments_temporal.hip,
// rtow_rectify_history.hip): W, S1, S2 and the tap count of L(q) over the guide-weighted (2 r + 1)^2 neighbourhood of a pixel, as include/rtow.h gives it for both
// entry points.  A 64 x 4 pixel workgroup stages its 70 x 10 halo region into LDS once - L(q) with NaN for "invalid or outside the image", entity, distance and normal,
// 24 bytes per pixel as six planes of 700 words (16800 bytes: 9 workgroups per CU, so LDS does not cap the 8 waves per SIMD) - and the taps run from there.  A wave
// reads 64 consecutive words of a plane per tap: no bank conflict, no padding.  L(q) is computed once per pixel by the operations the specification gives, so staging
// changes no bit.  The staging and the tap loop exist once, here; tests/temporal_moments_reference.py and tests/rectify_history_reference.py each restate them.
//
// The kernels declare the __shared__ planes themselves and place the barriers: one after stage(), and one before the planes are staged again.
#pragma once
#include "rtow_denoise_taps.hip.h"
#include "rtow_guide_weight.hip.h"

namespace rtow {
namespace halo {

constexpr int kMaxRadius = 3;                   // 7 x 7 taps
constexpr int kHaloW = taps::kGroupW + 2 * kMaxRadius, kHaloH = taps::kGroupH + 2 * kMaxRadius, kHalo = kHaloW * kHaloH;      // 70 x 10; (0, 0) is the pixel (x0 - 3, y0 - 3)

// the six planes of kHalo words each
struct Planes {
    float* L;
    int* E;
    float *T, *Nx, *Ny, *Nz;
};
static_assert(kHalo == 700 && 5 * sizeof(float) + sizeof(int) == 24,
              "70 x 10 words a plane, 24 bytes a pixel: the LDS figure of tests/test_temporal_moments_isa.py and tests/test_rectify_history_isa.py");

// the guides of the word k for guide::weight
struct Tap {
    const Planes& P;
    int k;
    __device__ __forceinline__ int entity() const { return P.E[k]; }
    __device__ __forceinline__ float distance() const { return P.T[k]; }
    __device__ __forceinline__ void normal(float& x, float& y, float& z) const { x = P.Nx[k]; y = P.Ny[k]; z = P.Nz[k]; }
};

// the word of the workgroup's own pixel (lx, ly)
__device__ __forceinline__ int centre_of(int lx, int ly) { return (ly + kMaxRadius) * kHaloW + lx + kMaxRadius; }

// Stages the part of the planes that `radius` reads for the tile at (x0, y0): (64 + 2 r) x (4 + 2 r) words from (3 - r, 3 - r).  Whole rows are walked, so that the row
// and the column of a word come from divisions by constants.  Outside the image only L is written.
__device__ __forceinline__ void stage(const Planes& P, int x0, int y0, int width, int height, int radius, const float* color, const int32_t* entity,
                                      const float* distance, const float* normal)
{
    const int c0 = kMaxRadius - radius, c1 = kHaloW - c0, end = (kHaloH - c0) * kHaloW;
#pragma unroll 1
    for (int s = c0 * kHaloW + (int)threadIdx.x; s < end; s += taps::kGroupW * taps::kGroupH) {
        const int cx = s % kHaloW, cy = s / kHaloW;
        if (cx < c0 || cx >= c1) continue;
        const int qx = x0 - kMaxRadius + cx, qy = y0 - kMaxRadius + cy;
        float l = __builtin_nanf("");                                     // outside the image: skipped like an invalid L
        if (qx >= 0 && qx < width && qy >= 0 && qy < height) {
            const size_t q = (size_t)qy * (size_t)width + (size_t)qx;
            l = taps::luminance_or_nan(color, q);
            P.E[s] = entity[q];
            P.T[s] = distance[q];
            const taps::P3 n = taps::ld3(normal, q);
            P.Nx[s] = n.x; P.Ny[s] = n.y; P.Nz[s] = n.z;
        }
        P.L[s] = l;
    }
}

struct Sums {
    float W, S1, S2;
    int taps;
};

// The sums over the taps of the pixel staged at `centre`, in the specification's order (j outer, i inner).  The pixel's own L is valid: it is inside the image, so its
// guides are staged.
__device__ __forceinline__ Sums neighbourhood(const Planes& P, int centre, int radius, int matchEntity, float depthTolerance, int normalSharpness)
{
    const int e = P.E[centre];
    const float t = P.T[centre], nx = P.Nx[centre], ny = P.Ny[centre], nz = P.Nz[centre];
    Sums r{0.0f, 0.0f, 0.0f, 0};
#pragma unroll 1
    for (int j = -radius; j <= radius; ++j) {
#pragma unroll 1
        for (int i = -radius; i <= radius; ++i) {
            const int k = centre + j * kHaloW + i;
            const float l = P.L[k];
            if (l != l) continue;                                         // outside the image, or L(q) invalid
            const float w = (i == 0 && j == 0) ? 1.0f                     // the centre consults no guide
                                               : guide::weight(e, t, nx, ny, nz, matchEntity, depthTolerance, normalSharpness, Tap{P, k});
            if (!(w > 0.0f)) continue;                                    // NaN included
            r.W = r.W + w;
            r.S1 = r.S1 + w * l;
            r.S2 = r.S2 + w * (l * l);
            ++r.taps;
        }
    }
    return r;
}

}  // namespace halo
}  // namespace rtow
