// rtow_hit_tests.hip.h - scene access and the exact primitive tests: SceneRefs / load_node / section (LDS image first, HBM / L2 for whatever did not fit), sphere_at,
// sphere_hit / sphere_hit_tmin, general_hit (Rect / Box / Triangle / transformed spheres) and the compact-record triangle test tri_hit_hot / tri_normal_cold.
// The helpers marked __host__ __device__ are also what the host probe walks its one ray with (rtow_probe.hip).
// Included by rtow_sample_kernel.hip.h (TEST, HIT and VOL stages, the tie resolver), rtow_walk.hip.h (the nearest-hit walk of the probe and the trace calls) and
// rtow_shade.hip (a named triangle's texture coordinates).
#pragma once
#include "rtow_kernels.h"
#include "rtow_vecmath.hip.h"

#ifndef RTOW_SPLIT_NODE_LOADS
#define RTOW_SPLIT_NODE_LOADS 1   // 0: A/B build with one flat load per node quad (the base chosen per lane) in the kernels whose tree does not fit LDS
#endif

namespace rtow {

namespace {

// ------------------------------------------------------------------------------------------------------------
// scene access: LDS image first, HBM/L2 for whatever did not fit
// ------------------------------------------------------------------------------------------------------------
struct SceneRefs {
    const uint8_t* lds;     // LDS copy of the blob prefix
    const uint8_t* glob;    // full blob in HBM
    uint32_t ldsNodeCount;
};
// the scene from global memory only (the probe's host image; the device queries and post passes, which stage nothing)
__host__ __device__ __forceinline__ SceneRefs global_scene(const uint8_t* blob) { return SceneRefs{nullptr, blob, 0u}; }

template <bool ALL_LDS, bool SPLIT = false>
__host__ __device__ __forceinline__ void load_node(const SceneRefs& sc, const SceneLayout& L, int idx, float4& q0, float4& q1, float4& q2, int& c0, int& c1)
{
    const uint32_t off = L.nodeOffset + (uint32_t)idx * 64u;
#if defined(__HIP_DEVICE_COMPILE__) && RTOW_SPLIT_NODE_LOADS
    if (!ALL_LDS && SPLIT) {
        // A tree that does not fit LDS keeps its first ldsNodeCount nodes (the top levels) there; the blob in memory holds every node.  Selecting the BASE per lane makes
        // every node load a flat_load (address-space check per lane, both memory counters, seven instructions to build the generic pointer), and a wave waits for its
        // slowest lane anyway: so the wave reads from LDS when ALL its walking lanes are in the top levels and through L1 / L2 otherwise - ds_read or global_load
        // (scalar base + 32-bit offset), never flat.  (Per-lane branches - ds_read under one EXEC mask, global_load under the other - make the compiler wait for the
        // first group before it issues the second: both write the same registers.)  SPLIT = the walk of the kernels with 16-bit codes: 10 000 spheres +0.6 %, same box,
        // three alternating runs each, every run above the other side's best.  The wide-code kernels keep the flat loads: their trees' lower levels miss L1 and L2, and
        // the lanes in the top levels are better off in LDS whatever the others do (250 882 triangles: -5 % with the split; profiles/r05q_node_loads.json).
        typedef __attribute__((address_space(3))) const uint8_t* LdsBytes;
        typedef __attribute__((address_space(1))) const uint8_t* GlobalBytes;
        if (__ballot((uint32_t)idx >= sc.ldsNodeCount) == 0ull) {      // wave-uniform: every lane that walks right now is in the top levels
            LdsBytes b = (LdsBytes)sc.lds + off;
            q0 = *(__attribute__((address_space(3))) const float4*)(b);
            q1 = *(__attribute__((address_space(3))) const float4*)(b + 16);
            q2 = *(__attribute__((address_space(3))) const float4*)(b + 32);
            // the two child codes through an asm statement (with its own wait: the compiler's wait-count bookkeeping does not see into it): as an ordinary load the
            // compiler sinks one of the two dwords behind the branch - as a flat load through a phi of both pointers, one more memory instruction per node visit
            typedef int i2 __attribute__((ext_vector_type(2)));
            i2 c;
            asm volatile("ds_read_b64 %0, %1 offset:48\n\ts_waitcnt lgkmcnt(0)" : "=v"(c) : "v"((unsigned)(uintptr_t)b) : "memory");
            c0 = c.x; c1 = c.y;
        } else {
            GlobalBytes b = (GlobalBytes)sc.glob + off;
            q0 = *(__attribute__((address_space(1))) const float4*)(b);
            q1 = *(__attribute__((address_space(1))) const float4*)(b + 16);
            q2 = *(__attribute__((address_space(1))) const float4*)(b + 32);
            const int2 c = *(__attribute__((address_space(1))) const int2*)(b + 48);
            c0 = c.x; c1 = c.y;
        }
        return;
    }
#endif
    const uint8_t* base = (ALL_LDS || (uint32_t)idx < sc.ldsNodeCount) ? sc.lds : sc.glob;
    const float4* p = reinterpret_cast<const float4*>(base + off);
    q0 = p[0];
    q1 = p[1];
    q2 = p[2];
    const int2 c = *reinterpret_cast<const int2*>(base + off + 48);
    c0 = c.x;
    c1 = c.y;
}

template <bool ALL_LDS>
__host__ __device__ __forceinline__ const uint8_t* section(const SceneRefs& sc, uint32_t offset)
{
    return (ALL_LDS ? sc.lds : sc.glob) + offset;
}

// centre of primitive `i` at ray time `time` (Entity.TransformAtTime, RT/Entity.cs:124-127) and its signed radius
template <bool ALL_LDS, bool HAS_MOTION>
__host__ __device__ __forceinline__ void sphere_at(const SceneRefs& sc, const SceneLayout& L, int i, float time, V3& c, float& radius)
{
    const float4 s = *reinterpret_cast<const float4*>(section<ALL_LDS>(sc, L.sphereOffset) + (uint32_t)i * 16u);
    c = v3(s.x, s.y, s.z);
    radius = s.w;
    if (HAS_MOTION) {
        const uint8_t* mp = section<ALL_LDS>(sc, L.motionOffset) + (uint32_t)i * 32u;
        const float4 m0 = *reinterpret_cast<const float4*>(mp);      // dx dy dz t0
        const float2 m1 = *reinterpret_cast<const float2*>(mp + 16); // t1 moving
        if (__builtin_bit_cast(int, m1.y) != 0) {
            // clamp(unlerp(t0, t1, t), 0, 1); when every moving entity shares one TimeRange (L.commonTimeRange) `time` already IS that value:
            // the sample's ray time goes through the expression once, in REGEN, instead of once per sphere test (same operands, same result)
            const float f = L.commonTimeRange ? time : um_max(0.0f, um_min(1.0f, (time - m0.w) / (m1.x - m0.w)));
            c = v3(c.x + m0.x * f, c.y + m0.y * f, c.z + m0.z * f);
        }
    }
}

// HitTests.Hit(Sphere) (RT/HitTests.cs:23-60) in entity space (oc = origin - centre), tMin = 0, tMax = +inf
__host__ __device__ __forceinline__ bool sphere_hit(V3 oc, V3 d, float a, float radius, float& tOut)
{
    const float b = dot(oc, d);
    const float c = dot(oc, oc) - radius * radius;
    const float disc = b * b - a * c;
    if (disc > 0) {
        // t = (-b -+ sq) / a with a = dot(d, d) >= 0: a numerator that is not positive gives a quotient that is not positive (or NaN) and
        // fails `t > 0` whatever a is, so its IEEE division is skipped - bit-identical, and the common "sphere behind the origin" case
        // (every ray leaving the ground sphere) costs no division at all.
        const float sq = RTOW_SQRT(disc);
        const float n0 = -b - sq;
        if (n0 > 0) {
            const float t = n0 / a;
            if (t < __builtin_inff() && t > 0) { tOut = t; return true; }
        }
        const float n1 = -b + sq;
        if (n1 > 0) {
            const float t = n1 / a;
            if (t < __builtin_inff() && t > 0) { tOut = t; return true; }
        }
    }
    return false;
}

// The quotient of sphere_hit for a run of tests that share the ray (TEST of the sphere kernels): the divisor a = dot(d, d) is the run's, so its correctly rounded
// reciprocal ya = RN(1 / a) and the range test aOk (exact_div3's bOk: positive, biased exponent in [96, 159]) are formed once per run and a candidate pays three instructions
// for t = n / a instead of the IEEE expansion (exact_div_step, enumerated over every mantissa pair by tests/native/exactdiv_parity.hip).
//  * One quotient a candidate.  sphere_hit's decision tree on sphere_hit's operands, with the root picked before the division: n0 > 0 takes the first root, anything
//    else the second (n1 >= n0, so a positive n0 has a positive n1 behind it).  Only a first root whose quotient fails `t < inf && t > 0` goes on to the second one,
//    as there - a cold region: the quotient of a positive numerator fails only by overflow, underflow to zero or a degenerate a.
//  * The quotient from the reciprocal where exact_div3's ranges hold: a in [2^-31, 2^33) and n in [2^-63, 2^65) (the numerators' range of exact_div3, positive only).
//    Then the quotient lies in (2^-96, 2^96): positive, finite and normal, so `t < inf && t > 0` holds and is not evaluated.  Anything else takes n / a and both tests.
// n0 and n1 as sphere_hit forms them; tests/native/sphere_quotient_parity.hip compares the two functions bit for bit.
__device__ __forceinline__ bool sphere_root_quotient(float n0, float n1, float a, float ya, bool aOk, float& tOut)
{
    const bool first = n0 > 0;
    const float n = first ? n0 : n1;
    // Straight-line for the lanes in range: the short quotient is formed for every lane (on other operands it is a value nobody reads) and ONE rare region redoes
    // the lanes with a positive numerator outside the ranges.  bits(n) in [0x20000000, 0x60000000) says positive AND biased exponent in [64, 191] in one unsigned
    // compare; `&`, not `&&`: a scalar AND of two lane masks, no region for the second test.  tOut is written without a hit too (that same unread value, or the
    // quotient that failed its tests): callers read it behind the returned flag only, as they do sphere_hit's.
    bool hit = RTOW_EXACT_DIV3 && (aOk & ((__float_as_uint(n) - 0x20000000u) < 0x40000000u));
    float t = exact_div_step(n, a, ya);
    if (__builtin_expect(n > 0 && !hit, 0)) {
        t = n / a;
        hit = t < __builtin_inff() && t > 0;
        if (!hit && first && n1 > 0) {
            t = n1 / a;
            hit = t < __builtin_inff() && t > 0;
        }
    }
    tOut = t;
    return hit;
}

// sphere_hit with the run's reciprocal: the same operands, the same result for every operand (device only: the host probe keeps sphere_hit)
__device__ __forceinline__ bool sphere_hit_shared_rcp(V3 oc, V3 d, float a, float ya, bool aOk, float radius, float& tOut)
{
    const float b = dot(oc, d);
    const float c = dot(oc, oc) - radius * radius;
    const float disc = b * b - a * c;
    if (disc > 0) {
        const float sq = RTOW_SQRT(disc);
        return sphere_root_quotient(-b - sq, -b + sq, a, ya, aOk, tOut);
    }
    return false;
}

// the same test with an arbitrary tMin (strict: t > tMin), RT/HitTests.cs:40,49
__host__ __device__ __forceinline__ bool sphere_hit_tmin(V3 oc, V3 d, float a, float radius, float tMin, float& tOut)
{
    const float b = dot(oc, d);
    const float c = dot(oc, oc) - radius * radius;
    const float disc = b * b - a * c;
    if (disc > 0) {
        const float sq = RTOW_SQRT(disc);                    // tMin >= 0 here: the numerator shortcut of sphere_hit applies unchanged
        const float n0 = -b - sq;
        if (n0 > 0) {
            const float t = n0 / a;
            if (t < __builtin_inff() && t > tMin) { tOut = t; return true; }
        }
        const float n1 = -b + sq;
        if (n1 > 0) {
            const float t = n1 / a;
            if (t < __builtin_inff() && t > tMin) { tOut = t; return true; }
        }
    }
    return false;
}

// ------------------------------------------------------------------------------------------------------------
// general entities (SCENE_KIND_GENERAL): Rect / Box / Triangle and rotated or moving transforms, RT/Entity.cs:58-127
// ------------------------------------------------------------------------------------------------------------
// Entity.HitInternal + HitContent for primitive `i` (RT/Entity.cs:74-122) with tMax = +inf (tMin = 0 except for the exit-hit
// probe of volume hulls, JOBS/SampleBatchJob.cs:465).
// Returns the distance, the entity-space normal and the rotation that takes it to world space.
template <bool ALL_LDS, bool TRIANGLES_ONLY = false>
__host__ __device__ __forceinline__ bool general_hit(const SceneRefs& sc, const SceneLayout& L, int i, unsigned type, V3 ro, V3 rd, float time, float tMin,
                                            float& tOut, V3& nLocal, float4& rot, float2* texCoord = nullptr)
{
    const float4* p = reinterpret_cast<const float4*>(section<ALL_LDS>(sc, L.primOffset) + (uint32_t)i * 128u);
    if (texCoord) *texCoord = make_float2(0, 0);       // only triangles have texture coordinates (RT/Entity.cs:108, RT/HitTests.cs:123)
    if (TRIANGLES_ONLY || type == RTOW_ENTITY_TRIANGLE) {       // TRIANGLES_ONLY (SCENE_KIND_TRIANGLES): the other primitives' code is not compiled in
        // HitTests.Hit(Triangle) (RT/HitTests.cs:115-150); triangles are tested in world space (RT/Entity.cs:91-93)
        // the first three quads (edges, v0, first normal) decide the test; the rest of the record - its second cache line when it is read from HBM -
        // is only fetched for a hit
        const float4 a0 = p[0], a1 = p[1], a2 = p[2];
        const V3 e0 = v3(a0.x, a0.y, a0.z), e1 = v3(a0.w, a1.x, a1.y), v0 = v3(a1.z, a1.w, a2.x);
        const V3 pvec = cross(rd, e0);
        const float det = dot(e1, pvec);
        if (det == 0) return false;
        const float invDet = RTOW_RCP(det);
        const V3 tvec = sub(ro, v0);
        const float u = dot(tvec, pvec) * invDet;
        if (u < 0 || u > 1) return false;
        const V3 qvec = cross(tvec, e1);
        const float v = dot(rd, qvec) * invDet;
        if (v < 0 || u + v > 1) return false;
        const float dist = dot(e0, qvec) * invDet;
        if (dist < tMin || dist > __builtin_inff()) return false;
        const float b0 = 1 - u - v;
        const float4 a3 = p[3], a4 = p[4];
        rot = p[6];
        const V3 n0 = v3(a2.y, a2.z, a2.w), n1 = v3(a3.x, a3.y, a3.z), n2 = v3(a3.w, a4.x, a4.y);
        nLocal = v3(n0.x * b0 + n1.x * u + n2.x * v, n0.y * b0 + n1.y * u + n2.y * v, n0.z * b0 + n1.z * u + n2.z * v);
        if (texCoord) {                                  // mul(tri.TextureCoordinates, barycentricCoords) (:148): float2x3 columns t0 t1 t2
            const float4 a5 = p[5];
            *texCoord = make_float2(a4.z * b0 + a5.x * u + a5.z * v, a4.w * b0 + a5.y * u + a5.w * v);
        }
        tOut = dist;
        return true;
    }
    rot = p[0];
    const float4 invRot = p[1], q2 = p[2], q3 = p[3], q4 = p[4], q5 = p[5];
    V3 invT = v3(q4.y, q4.z, q4.w);
    if (__builtin_bit_cast(int, q2.w) != 0) {
        // TransformAtTime (RT/Entity.cs:124-127) and its inverse (:87-88): invTranslation = mul(invRot, -pos(t))
        const float f = um_max(0.0f, um_min(1.0f, (time - q3.w) / (q4.x - q3.w)));
        const V3 pt = v3(q2.x + q3.x * f, q2.y + q3.y * f, q2.z + q3.z * f);
        invT = rotate(invRot, neg(pt));
    }
    const V3 oL = add(rotate(invRot, ro), invT);     // transform(inverseTransform, ray.Origin)
    const V3 dL = rotate(invRot, rd);                // rotate(inverseTransform, ray.Direction)
    if (type == RTOW_ENTITY_SPHERE) {
        float t;
        if (!sphere_hit_tmin(oL, dL, dot(dL, dL), q5.x, tMin, t)) return false;
        nLocal = div3(v3(oL.x + t * dL.x, oL.y + t * dL.y, oL.z + t * dL.z), q5.x);
        tOut = t;
        return true;
    }
    if (type == RTOW_ENTITY_RECT) {
        // HitTests.Hit(Rect) (RT/HitTests.cs:62-78)
        if (dL.z >= 0) return false;
        const float t = -oL.z / dL.z;
        if (t < tMin || t > __builtin_inff()) return false;
        const float x = oL.x + t * dL.x, y = oL.y + t * dL.y;
        if (x < q5.x || y < q5.y || x > q5.z || y > q5.w) return false;
        nLocal = v3(0, 0, 1);
        tOut = t;
        return true;
    }
    // HitTests.Hit(Box) (RT/HitTests.cs:80-113): the origin is first advanced by tMin (origin + direction * tMin)
    const float4 q6 = p[6];
    const V3 ext = v3(q5.x, q5.y, q5.z), invExt = v3(q5.w, q6.x, q6.y);
    const V3 o = v3(oL.x + dL.x * tMin, oL.y + dL.y * tMin, oL.z + dL.z * tMin);
    const float winding = um_max(um_max(__builtin_fabsf(o.x) * invExt.x, __builtin_fabsf(o.y) * invExt.y), __builtin_fabsf(o.z) * invExt.z) < 1 ? -1.0f : 1.0f;
    V3 sgn = v3(-um_sign(dL.x), -um_sign(dL.y), -um_sign(dL.z));
    const V3 dtp = v3((ext.x * winding * sgn.x - o.x) / dL.x, (ext.y * winding * sgn.y - o.y) / dL.y, (ext.z * winding * sgn.z - o.z) / dL.z);
    const bool tx = dtp.x >= 0 && __builtin_fabsf(o.y + dL.y * dtp.x) < ext.y && __builtin_fabsf(o.z + dL.z * dtp.x) < ext.z;
    const bool ty = dtp.y >= 0 && __builtin_fabsf(o.z + dL.z * dtp.y) < ext.z && __builtin_fabsf(o.x + dL.x * dtp.y) < ext.x;
    const bool tz = dtp.z >= 0 && __builtin_fabsf(o.x + dL.x * dtp.z) < ext.x && __builtin_fabsf(o.y + dL.y * dtp.z) < ext.y;
    sgn = tx ? v3(sgn.x, 0, 0) : ty ? v3(0, sgn.y, 0) : v3(0, 0, tz ? sgn.z : 0);
    if (!(sgn.x != 0 || sgn.y != 0 || sgn.z != 0)) return false;
    float dist = sgn.x != 0 ? dtp.x : sgn.y != 0 ? dtp.y : dtp.z;
    dist += tMin;
    if (dist > __builtin_inff()) return false;
    nLocal = sgn;
    tOut = dist;
    return true;
}

// HitTests.Hit(Triangle) (RT/HitTests.cs:115-150) on the compact record of an all-triangle scene (GpuTriHot, rtow_scene.h): the same expressions as general_hit's triangle
// branch on the same operands, up to the distance; the barycentric (u, v) are handed back instead of the blended normal, which only the ray's nearest hit needs (tri_normal_cold)
template <bool ALL_LDS>
__host__ __device__ __forceinline__ bool tri_hit_hot(const SceneRefs& sc, const SceneLayout& L, int i, V3 ro, V3 rd, float tMin, float& tOut, float& uOut, float& vOut)
{
    const float4* p = reinterpret_cast<const float4*>(section<ALL_LDS>(sc, L.triHotOffset) + (uint32_t)i * (uint32_t)sizeof(GpuTriHot));
    const float4 a0 = p[0], a1 = p[1];
    const float a2x = *reinterpret_cast<const float*>(p + 2);
    const V3 e0 = v3(a0.x, a0.y, a0.z), e1 = v3(a0.w, a1.x, a1.y), v0 = v3(a1.z, a1.w, a2x);
    const V3 pvec = cross(rd, e0);
    const float det = dot(e1, pvec);
    if (det == 0) return false;
    const float invDet = RTOW_RCP(det);
    const V3 tvec = sub(ro, v0);
    const float u = dot(tvec, pvec) * invDet;
    if (u < 0 || u > 1) return false;
    const V3 qvec = cross(tvec, e1);
    const float v = dot(rd, qvec) * invDet;
    if (v < 0 || u + v > 1) return false;
    const float dist = dot(e0, qvec) * invDet;
    if (dist < tMin || dist > __builtin_inff()) return false;
    tOut = dist;
    uOut = u;
    vOut = v;
    return true;
}
// the rest of that test for the hit that won: mul(tri.Normals, barycentricCoords) (RT/HitTests.cs:140-146) from the GpuTriCold record, and the entity's rotation
template <bool ALL_LDS>
__host__ __device__ __forceinline__ V3 tri_normal_cold(const SceneRefs& sc, const SceneLayout& L, int i, float u, float v, float4& rot)
{
    const float4* p = reinterpret_cast<const float4*>(section<ALL_LDS>(sc, L.triColdOffset) + (uint32_t)i * (uint32_t)sizeof(GpuTriCold));
    const float4 c0 = p[0], c1 = p[1];
    const float c2x = *reinterpret_cast<const float*>(p + 2);
    rot = p[3];
    const float b0 = 1 - u - v;
    const V3 n0 = v3(c0.x, c0.y, c0.z), n1 = v3(c0.w, c1.x, c1.y), n2 = v3(c1.z, c1.w, c2x);
    return v3(n0.x * b0 + n1.x * u + n2.x * v, n0.y * b0 + n1.y * u + n2.y * v, n0.z * b0 + n1.z * u + n2.z * v);
}

} // namespace

} // namespace rtow
