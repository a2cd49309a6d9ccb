// rtow_reproject_steps.hip.h - steps 1 to 3 of the reprojection specification (include/rtow.h next to RtowReprojectParams), shared by the two kernels that carry the
// previous view's accumulators to a moved camera: rtowReprojectAccumDevice's (rtow_reproject.hip, one nearest previous pixel) and
// rtowReprojectAccumBilinearDevice's (rtow_reproject_bilinear.hip, four taps).  project_point is steps 1 and 2 up to fx, fy and their in-frame test; tap_matches is
// step 3 at one previous pixel (tap_matches_unbranched: the same, both words always read).  Each spells out the specification's evaluation order (-ffp-contract=off, correctly rounded `/`, exact_sqrt).
#pragma once
#include "rtow_kernels.h"

#include "rtow_vecmath.hip.h"

namespace rtow {

namespace {

constexpr int kReprojectBlock = 256;                      // four 8 x 8 tiles
constexpr unsigned kReprojectMaxBlocks = 4096;            // two rounds of the 2048 workgroups an MI355X holds at 8 waves per SIMD; tile groups beyond this (frames from
                                                          // about 1024 x 1024) are walked by the grid-stride loop

struct ReprojectArgs {
    int width, height;
    unsigned tilesX, tiles;             // 8 x 8 pixel tiles per row / in all
    RtowFloat3 origin, forward, right, up;      // of previousView
    ReprojectConstants k;
    float depthTolerance, maxHistory;   // (float)maxHistory
    int matchEntity;
    const RtowRay* rays;
    const float* distance;
    const int32_t* entity;
    const float* prevDistance;
    const int32_t* prevEntity;
    const float *prevColor, *prevNormal, *prevAlbedo, *prevScw;
    float *outColor, *outNormal, *outAlbedo, *outScw;
    int32_t* outSource;
};

inline ReprojectArgs reprojectArgs(const RtowReprojectParams& p, const ReprojectConstants& k, const RtowRay* rays, const RtowHitBuffers& hits,
                                   const RtowHitBuffers& previousHits, const RtowAccumBuffers& previous, const RtowAccumBuffers& out, int32_t* outSource)
{
    ReprojectArgs A{};
    A.width = p.width;
    A.height = p.height;
    A.tilesX = ((unsigned)p.width + 7u) / 8u;
    A.tiles = (unsigned)((uint64_t)A.tilesX * (((uint64_t)p.height + 7u) / 8u));      // (w / 8 + 1) (h / 8 + 1) < 2^29 for w h < 2^31
    A.origin = p.previousView.origin;
    A.forward = p.previousView.forward;
    A.right = p.previousView.right;
    A.up = p.previousView.up;
    A.k = k;
    A.depthTolerance = p.depthTolerance;
    A.maxHistory = (float)p.maxHistory;
    A.matchEntity = (p.flags & RTOW_REPROJECT_MATCH_ENTITY) != 0;
    A.rays = rays;
    A.distance = hits.distance;
    A.entity = hits.entityIndex;
    A.prevDistance = previousHits.distance;
    A.prevEntity = previousHits.entityIndex;
    A.prevColor = previous.color; A.prevNormal = previous.normal; A.prevAlbedo = previous.albedo; A.prevScw = previous.sampleCountWeight;
    A.outColor = out.color; A.outNormal = out.normal; A.outAlbedo = out.albedo; A.outScw = out.sampleCountWeight;
    A.outSource = outSource;
    return A;
}

// workgroups of four tiles, capped: the kernels walk the rest by a grid-stride loop
inline unsigned reprojectBlocks(const ReprojectArgs& A)
{
    const unsigned groups = (A.tiles + kReprojectBlock / 64 - 1) / (kReprojectBlock / 64);
    return groups < kReprojectMaxBlocks ? groups : kReprojectMaxBlocks;
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, RtowFloat3 b) { return (ax * b.x + ay * b.y) + az * b.z; }

// steps 1 and 2: where pixel `i`'s first hit lies in the previous view.  False: nothing is carried.  Otherwise (fx, fy) in [0, W) x [0, H), the hit's entity e (< 0:
// sky) and its distance r from the previous camera (0 for sky).
__device__ __forceinline__ bool project_point(const ReprojectArgs& A, size_t i, float& fx, float& fy, int& e, float& r)
{
    const Ray8 ray = reinterpret_cast<const Ray8*>(A.rays)[i];
    const float t = A.distance[i];
    e = A.entity[i];
    float wx = ray.dx, wy = ray.dy, wz = ray.dz;
    r = 0.0f;
    if (e >= 0) {
        const float px = ray.ox + t * ray.dx, py = ray.oy + t * ray.dy, pz = ray.oz + t * ray.dz;
        wx = px - A.origin.x; wy = py - A.origin.y; wz = pz - A.origin.z;
        r = exact_sqrt((wx * wx + wy * wy) + wz * wz);
    }
    const float s = dot3(wx, wy, wz, A.forward) / A.k.LF;
    if (!(s > 0.0f)) return false;
    const float u = (dot3(wx, wy, wz, A.right) / s - A.k.LR) / A.k.HR;
    const float v = (dot3(wx, wy, wz, A.up) / s - A.k.LU) / A.k.VU;
    const float sizeX = (float)A.width, sizeY = (float)A.height;
    fx = u * sizeX;
    fy = v * sizeY;
    return fx >= 0.0f && fx < sizeX && fy >= 0.0f && fy < sizeY;          // NaN fails
}

// step 3: does previous pixel q show what the new pixel's first hit (e, r) is
__device__ __forceinline__ bool tap_matches(const ReprojectArgs& A, int q, int e, float r)
{
    const int pe = A.prevEntity[q];
    if (e < 0) return pe < 0;
    if (pe < 0 || (A.matchEntity && pe != e)) return false;
    const float pt = A.prevDistance[q];
    return __builtin_fabsf(pt - r) <= A.depthTolerance * r;
}

// step 3 again, the same rule without a branch: both words of q are read whatever the entity says.  For the four-tap kernel, whose tap loop sits inside the
// grid-stride loop with every kernel argument live: each divergent region nested there holds two more scalar registers, and the branches of tap_matches are what took
// that kernel past the scalar registers that 8 waves per SIMD leave it.
__device__ __forceinline__ bool tap_matches_unbranched(const ReprojectArgs& A, int q, int e, float r)
{
    const int pe = A.prevEntity[q];
    const float pt = A.prevDistance[q];
    const bool hit = pe >= 0 && !(A.matchEntity && pe != e) && __builtin_fabsf(pt - r) <= A.depthTolerance * r;
    return e < 0 ? pe < 0 : hit;
}

}  // namespace

}  // namespace rtow
