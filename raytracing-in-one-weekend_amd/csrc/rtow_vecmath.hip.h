// rtow_vecmath.hip.h - the float3 helpers and the exact-math macros of the path's float program: V3 and its operations, normalize / reflect, Unity.Mathematics' min / max /
// saturate / sign, half -> float, quaternion rotation, the three-way IEEE division.  Each helper spells out the reference's evaluation order (-ffp-contract=off, IEEE
// division and square root through the exhaustively checked short forms of rtow_exactmath.hip.h).
// Included by rtow_hit_tests.hip.h and rtow_surface.hip.h (and through them by the sample kernel, the walk and the shade pass), by rtow_kernels.hip, and by
// rtow_reproject.hip / rtow_upsample.hip for the packed buffer records at its end.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rtow.h"
#include "rtow_exactmath.hip.h"

// IEEE 1 / x and sqrt(x) of the path's float program: the exhaustively checked short forms of rtow_exactmath.hip.h (same result for every
// operand; RTOW_EXACT_MATH=0 builds the compiler's expansions instead, for A/B timing).
#ifndef RTOW_EXACT_MATH
#define RTOW_EXACT_MATH 1
#endif
#if RTOW_EXACT_MATH
#define RTOW_RCP(x) rtow::exact_rcp(x)
#define RTOW_RCP_NAN_TO_INF(x) rtow::exact_rcp_nan_to_inf(x)
#define RTOW_SQRT(x) rtow::exact_sqrt(x)
#ifndef RTOW_EXACT_DIV3
#define RTOW_EXACT_DIV3 1
#endif
#else
#define RTOW_RCP(x) (1.0f / (x))
#define RTOW_RCP_NAN_TO_INF(x) ([](float r_) { return r_ != r_ ? __builtin_inff() : r_; }(1.0f / (x)))
#define RTOW_SQRT(x) __builtin_sqrtf(x)
#define RTOW_EXACT_DIV3 0
#endif

namespace rtow {

namespace {

// ------------------------------------------------------------------------------------------------------------
// small float3 helpers; each spells out the reference's evaluation order
// ------------------------------------------------------------------------------------------------------------
struct V3 { float x, y, z; };
// (the helpers marked __host__ __device__ here and in rtow_hit_tests.hip.h - vectors, um_min / um_max, scene access, sphere_at, sphere_hit, general_hit - are also what rtowProbeNearestHit walks its one
// ray with on the host: rtow_probe.hip; the host pass evaluates the same expressions with the IEEE operations the device's short forms stand for)

__host__ __device__ __forceinline__ V3 v3(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__host__ __device__ __forceinline__ V3 v3(const RtowFloat3& a) { return v3(a.x, a.y, a.z); }
__host__ __device__ __forceinline__ V3 add(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__host__ __device__ __forceinline__ V3 sub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__host__ __device__ __forceinline__ V3 neg(V3 a) { return v3(-a.x, -a.y, -a.z); }
__host__ __device__ __forceinline__ V3 scale(float s, V3 a) { return v3(s * a.x, s * a.y, s * a.z); }
__host__ __device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// math.normalize(v) = rsqrt(dot(v, v)) * v with rsqrt(x) = 1 / sqrt(x)
__device__ __forceinline__ V3 normalize(V3 v) { const float r = RTOW_RCP(RTOW_SQRT(dot(v, v))); return scale(r, v); }
// math.reflect(i, n) = i - 2f * n * dot(i, n)
__device__ __forceinline__ V3 reflect(V3 i, V3 n)
{
    const float d = dot(i, n);
    return v3(i.x - (2.0f * n.x) * d, i.y - (2.0f * n.y) * d, i.z - (2.0f * n.z) * d);
}
// math.min / math.max return the FIRST operand when the second is NaN
__host__ __device__ __forceinline__ float um_min(float x, float y) { return (y != y || x < y) ? x : y; }
__host__ __device__ __forceinline__ float um_max(float x, float y) { return (y != y || x > y) ? x : y; }
__device__ __forceinline__ float um_saturate(float x) { return um_max(0.0f, um_min(1.0f, x)); }

constexpr float kPi = 3.14159265f; // math.PI

// Unity.Mathematics.half -> float (exact)
__device__ __forceinline__ float half_bits_to_float(unsigned h)
{
    const unsigned sign = (h & 0x8000u) << 16;
    const unsigned exp = (h >> 10) & 0x1fu, man = h & 0x3ffu;
    if (exp == 0) return __uint_as_float(__float_as_uint((float)man * 5.9604644775390625e-8f) | sign);   // zero / subnormal: man * 2^-24, exact
    if (exp == 31) return __uint_as_float(sign | 0x7f800000u | (man << 13));
    return __uint_as_float(sign | ((exp + 112u) << 23) | (man << 13));
}

// (p.x / d, p.y / d, p.z / d): three IEEE divisions by one divisor (a sphere's outward normal, r.GetPoint(t) / radius, RT/HitTests.cs:56)
__host__ __device__ __forceinline__ V3 div3(V3 p, float d)
{
#if RTOW_EXACT_DIV3
    V3 q;
    rtow::exact_div3(p.x, p.y, p.z, d, q.x, q.y, q.z);
    return q;
#else
    return v3(p.x / d, p.y / d, p.z / d);
#endif
}

__host__ __device__ __forceinline__ V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
// math.mul(quaternion q, float3 v): t = 2 * cross(q.xyz, v); v + q.w * t + cross(q.xyz, t)
__host__ __device__ __forceinline__ V3 rotate(float4 q, V3 v)
{
    const V3 qv = v3(q.x, q.y, q.z);
    const V3 t = scale(2.0f, cross(qv, v));
    const V3 c = cross(qv, t);
    return v3(v.x + q.w * t.x + c.x, v.y + q.w * t.y + c.y, v.z + q.w * t.z + c.z);
}
__host__ __device__ __forceinline__ float um_sign(float x) { return (x > 0.0f ? 1.0f : 0.0f) - (x < 0.0f ? 1.0f : 0.0f); }

// the callers' tightly packed buffers at 4-byte aligned addresses (a caller may pass a view that starts anywhere in an allocation): float3, float4 and RtowRay
struct __attribute__((packed, aligned(4))) P3 { float x, y, z; };
struct __attribute__((packed, aligned(4))) P4 { float x, y, z, w; };
struct __attribute__((packed, aligned(4))) Ray8 { float ox, oy, oz, time, dx, dy, dz, pad; };
static_assert(sizeof(Ray8) == sizeof(RtowRay), "RtowRay is eight floats");

} // namespace

} // namespace rtow
