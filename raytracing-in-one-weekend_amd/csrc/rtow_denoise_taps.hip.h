// rtow_denoise_taps.hip.h - what the image-space post passes share.  The a-trous filters (rtow_denoise.hip: rtowDenoiseDevice; rtow_denoise_variance.hip:
// rtowDenoiseVarianceDevice): albedo (de)modulation, the B3 taps, the normal weight.  Those two and the moments passes (rtow_denoise_variance.hip:
// rtowAccumulateMomentsDevice; rtow_moments_temporal.hip, rtow_rectify_history.hip through rtow_guided_halo.hip.h; rtow_noise_mask.hip): the packed float3 / float4
// access, the luminance and L(q), and the grid of 64 x 4 pixel workgroup tiles their launchers size.  The tap rules of include/rtow.h exist once, here; every device
// function is one float32 operation of the specification after the other (the units are compiled without contraction).
#pragma once
#include <hip/hip_runtime.h>

namespace rtow {
namespace taps {

// float3 at a 4-byte aligned address (the buffers are tightly packed float3; a caller may pass views that start 4 bytes into an allocation)
struct __attribute__((packed, aligned(4))) P3 { float x, y, z; };
__device__ __forceinline__ P3 ld3(const float* p, size_t index) { return reinterpret_cast<const P3*>(p)[index]; }
// float4 likewise (an accumulator colour buffer, possibly a view that starts 4 bytes into an allocation)
struct __attribute__((packed, aligned(4))) P4 { float x, y, z, w; };
__device__ __forceinline__ P4 ld4(const float* p, size_t index) { return reinterpret_cast<const P4*>(p)[index]; }

constexpr float kDemodMin = 0.0009765625f;      // 2^-10

__device__ __forceinline__ bool finite3(P3 c) { return __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z); }
__device__ __forceinline__ bool zero3(P3 n) { return n.x == 0.0f && n.y == 0.0f && n.z == 0.0f; }
__device__ __forceinline__ float dist2(P3 a, P3 b)
{
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return (dx * dx + dy * dy) + dz * dz;
}
__device__ __forceinline__ P3 demod(P3 c, P3 a)
{
    return P3{a.x >= kDemodMin ? c.x / a.x : c.x, a.y >= kDemodMin ? c.y / a.y : c.y, a.z >= kDemodMin ? c.z / a.z : c.z};
}
__device__ __forceinline__ P3 remod(P3 r, P3 a)
{
    return P3{a.x >= kDemodMin ? r.x * a.x : r.x, a.y >= kDemodMin ? r.y * a.y : r.y, a.z >= kDemodMin ? r.z * a.z : r.z};
}
// B3 spline tap h(i), i = -2..2: exact binary fractions, so h(i) * h(j) is exact
__device__ __forceinline__ float b3(int i) { return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f; }

// wn: 1 between two exactly-zero normals (sky beside sky), 0 between a zero and a non-zero one, else max(0, n.n')^(2^sharpness) by repeated squaring
__device__ __forceinline__ float normalWeight(P3 np, bool npZero, P3 nq, int sharpness)
{
    const bool nqZero = zero3(nq);
    if (npZero || nqZero) return (npZero && nqZero) ? 1.0f : 0.0f;
    float d = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
    d = d > 0.0f ? d : 0.0f;
    for (int e = 0; e < sharpness; ++e) d = d * d;
    return d;
}

// Rec. 709 luminance, in this association (rtowAccumulateMomentsDevice and the colour term of rtowDenoiseVarianceDevice)
__device__ __forceinline__ float lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

// L(q) of the specification: the luminance of the accumulator colour's mean, NaN when invalid (a valid L is finite, so NaN is free to mean "no luminance")
__device__ __forceinline__ float luminance_or_nan(const float* color, size_t q)
{
    const P4 c = ld4(color, q);
    if (!(c.w > 0.0f)) return __builtin_nanf("");          // no successful sample (NaN included)
    const float l = lum(c.x / c.w, c.y / c.w, c.z / c.w);
    return __builtin_isfinite(l) ? l : __builtin_nanf("");
}

// The workgroup of the tiled passes is kGroupW x kGroupH pixels, a wave being 64 pixels of one row.  Host: the tiles that cover a width x height frame.
constexpr int kGroupW = 64, kGroupH = 4;
static_assert(kGroupW == 64 && kGroupW * kGroupH == 256, "the kernels split threadIdx.x of a 256-lane workgroup by & 63 and >> 6");
struct TileGrid { unsigned tilesX, tiles; };          // per row / in all
inline TileGrid tileGrid(int width, int height)
{
    const unsigned tilesX = ((unsigned)width + kGroupW - 1) / kGroupW;
    return TileGrid{tilesX, (unsigned)((uint64_t)tilesX * (((uint64_t)height + kGroupH - 1) / kGroupH))};      // (w / 64 + 1) (h / 4 + 1) < 2^30 for w h < 2^31
}

}  // namespace taps
}  // namespace rtow
