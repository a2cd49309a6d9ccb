// rtow_walk.hip.h - the walk of one ray through the scene image, shared by the host probe (rtow_probe.hip: rtowProbeNearestHit / rtowProbeNearestHitInterval) and the device
// queries (rtow_trace.hip: rtowTraceRaysDevice / rtowTraceViewDevice; rtow_trace_interval.hip: rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice).  One text (`walk`,
// below) for the open form (0, +inf) and the two interval forms, compiled for the host and for gfx950, so that none of them can drift apart.
//
// What the reference's recursion (HitTests.Hit(BvhNode), RT/HitTests.cs:152-196) computes: the smallest Entity.Hit distance (tMin 0, tMax +inf) over the entities of the
// leaves it reaches, and it reaches a leaf iff the ray passes the box of every node above it under AxisAlignedBoundingBox.Hit (RT/HitTests.cs:9-21).  A box that encloses
// another passes whenever the inner one does (subtraction, multiplication, min and max are monotone in binary32), so that set is "the entities whose own box the ray passes" -
// what the leaf children of this library's tree carry (the reference's own entity boxes under the reference's own slab test; the leaf's box where the host forced a leaf at
// MaxBvhDepth).  The walk visits them with the sample kernel's own hit tests (sphere_at / sphere_hit / general_hit of rtow_hit_tests.hip.h: the same expressions in the
// same order, IEEE division and square root, no contraction), pruning inner boxes by the best distance so far with the kernel's 2^-12 of slack.
// Hits at bit-identical distance: the entity that comes first in the reference tree's leaf order (what the sample path shades).
//
// The interval forms: Entity.Hit(r, tMin, tMax) instead of Entity.Hit(r, 0, +inf).  The caller has checked 0 <= tMin <= tMax (interval_is_traced; tMax may be +inf).
//  * tMin goes to the helpers that already take it (sphere_hit_tmin: strict; general_hit: Rect / Triangle inclusive, Box advances the origin by it).  tMax is applied to
//    their result: t < tMax for a sphere (RT/HitTests.cs:40,49), !(t > tMax) for Rect / Box / Triangle (:68,108,135).  For a sphere the helper returns the far root only when
//    the near one failed `t > tMin`; a near root that passes tMin and fails tMax leaves a far root (the same division of a numerator that is no smaller) that fails tMax too,
//    so "the helper's root, then tMax" is the reference's "near root under both bounds, else far root under both".
//  * The leaf gate is the open form's: AxisAlignedBoundingBox.Hit knows nothing of the query interval.  Inner boxes are pruned by min(best, tMax) with the same 2^-12 of slack:
//    what lies wholly beyond tMax is rejected by every test above, as what lies beyond the best hit loses to it.  Nothing is pruned on the tMin side: an entity that the ray
//    meets beyond tMin can sit in a padded box whose slab interval, in binary32, ends below tMin * (1 - 2^-12) only if that bound were proven - it is not, so it is left out.
//  * WALK_ANY ends at the first accepted hit (bestPrim names it, bestT is its distance - some hit, not the nearest).  Otherwise the nearest, ties by `rank` as above.
//  * A distance that is not below +inf (the reference's Triangle test lets +inf and NaN through) never wins in any form (best starts at +inf), so that "occluded" and "the
//    nearest form names an entity" are one predicate.
// WALK_OPEN is the same text with the bounded branches compiled out - not (0, +inf) passed at run time: min(best, +inf) does not fold under IEEE NaN rules, and the open
// kernels would pay for the bounds.
//
// Stack: where the pending far children live.  `bool push(int)` (false: no room - the walk then reports overflow instead of dropping a subtree silently), `int pop()`,
// `bool empty()`.  The host keeps a growing array; the device a column of an LDS array (rtow_trace_lanes.hip.h).
#pragma once
#include "rtow_hit_tests.hip.h"

#include <type_traits>

namespace rtow {

namespace {

// v_min_f32 / v_max_f32 in IEEE mode as the kernels' slab tests use them: a NaN operand yields the other operand.  On the device that is the instruction itself (minnum /
// maxnum); the host spells it out.  (The two may differ in the sign of a zero result, which no comparison below can see.)
__host__ __device__ __forceinline__ float hmin(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fminf(a, b);
#else
    return a != a ? b : (b != b ? a : (a < b ? a : b));
#endif
}
__host__ __device__ __forceinline__ float hmax(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmaxf(a, b);
#else
    return a != a ? b : (b != b ? a : (a > b ? a : b));
#endif
}

// BASE -> the walk's template argument at run time: f(std::integral_constant<int, BASE>) with SCENE_KIND_SPHERES, SCENE_KIND_SPHERES_MOTION, or SCENE_KIND_GENERAL for
// every kind that keeps GpuPrim records.  Host only: the probe's walks and the query kernels' launchers.
template <typename F>
inline void for_scene_base(uint32_t sceneKind, F&& f)
{
    if (sceneKind == SCENE_KIND_SPHERES) f(std::integral_constant<int, SCENE_KIND_SPHERES>{});
    else if (sceneKind == SCENE_KIND_SPHERES_MOTION) f(std::integral_constant<int, SCENE_KIND_SPHERES_MOTION>{});
    else f(std::integral_constant<int, SCENE_KIND_GENERAL>{});
}

enum WalkForm {
    WALK_OPEN,      // Entity.Hit(r, 0, +inf), nearest; tMin / tMax are not read
    WALK_NEAREST,   // Entity.Hit(r, tMin, tMax), nearest
    WALK_ANY,       // Entity.Hit(r, tMin, tMax), the first accepted hit
};

// BASE: as for_scene_base hands it out.  blob: the scene image with the derived entity transforms in place (the device's own copy, or the host image rtowUploadScene copied
// them back into).  bestPrim: the PRIMITIVE number (CompiledScene.entityOfPrim takes it to the host's entity index), -1 on a miss; bestT then stays +inf.  rtimeOut: the ray
// time as sphere_at expects it (for the caller that derives the winner's normal).  Returns false if the stack refused a push (the result is then not to be used).
template <int BASE, WalkForm FORM, typename Stack>
__host__ __device__ __forceinline__ bool walk(const uint8_t* blob, const SceneLayout& L, V3 ro, V3 rd, float time, float tMin, float tMax, Stack& stack, float& bestT, int& bestPrim,
                                              float& rtimeOut)
{
    constexpr bool GENERAL = BASE >= SCENE_KIND_GENERAL;
    constexpr bool HAS_MOTION = BASE == SCENE_KIND_SPHERES_MOTION;
    constexpr bool BOUNDED = FORM != WALK_OPEN;
    constexpr bool ANY = FORM == WALK_ANY;
    const SceneRefs sc = global_scene(blob);
    float rtime = time;
    if (HAS_MOTION) { if (L.commonTimeRange) rtime = um_max(0.0f, um_min(1.0f, (rtime - L.commonT0) / (L.commonT1 - L.commonT0))); }     // what sphere_at expects (the kernel's REGEN does the same)
    const V3 inv = v3(exact_rcp_nan_to_inf(rd.x), exact_rcp_nan_to_inf(rd.y), exact_rcp_nan_to_inf(rd.z));
    const float a = dot(rd, rd);
    const unsigned* rank = reinterpret_cast<const unsigned*>(blob + L.rankOffset);
    const bool twoChildren = L.sphereCount > 1u;
    float best = __builtin_inff();
    int prim = -1;
    bool ok = true;
    int cur = 0;
    while (cur >= 0) {
        float4 q0, q1, q2;
        int c0, c1;
        load_node<false>(sc, L, cur, q0, q1, q2, c0, c1);
        const float bestPrune = (BOUNDED ? hmin(best, tMax) : best) * 1.000244140625f;
        int next[2];
        float entry[2];
        int inner = 0;
        for (int side = 0; side < 2; side++) {
            if (side == 1 && !twoChildren) break;
            const int child = side ? c1 : c0;
            const float lox = side ? q0.y : q0.x, loy = side ? q0.w : q0.z, loz = side ? q1.y : q1.x;
            const float hix = side ? q1.w : q1.z, hiy = side ? q2.y : q2.x, hiz = side ? q2.w : q2.z;
            const float tlx = (lox - ro.x) * inv.x, thx = (hix - ro.x) * inv.x;
            const float tly = (loy - ro.y) * inv.y, thy = (hiy - ro.y) * inv.y;
            const float tlz = (loz - ro.z) * inv.z, thz = (hiz - ro.z) * inv.z;
            const float tmin = hmax(hmax(hmin(tlx, thx), hmin(tly, thy)), hmax(hmin(tlz, thz), 0.0f));
            const float tfar = hmin(hmin(hmax(tlx, thx), hmax(tly, thy)), hmax(tlz, thz));
            if (child >= 0) {
                if (tmin <= hmin(tfar, bestPrune)) { next[inner] = child; entry[inner] = tmin; inner++; }      // padded inner box: conservative, pruned by the nearest hit so far (and tMax)
                continue;
            }
            if (!(tmin < tfar)) continue;                                      // AxisAlignedBoundingBox.Hit on the entity's own box (RT/HitTests.cs:15-20)
            const int i = ~child;
            float t;
            bool hit;
            if (GENERAL) {
                const unsigned type = *reinterpret_cast<const unsigned*>(blob + L.matIndexOffset + (uint32_t)i * 4u) >> kPrimTypeShift;
                V3 nl; float4 rq;
                hit = general_hit<false>(sc, L, i, type, ro, rd, rtime, BOUNDED ? tMin : 0.0f, t, nl, rq);
                if (BOUNDED && hit) hit = type == RTOW_ENTITY_SPHERE ? t < tMax : !(t > tMax);
            } else {
                V3 c; float r;
                sphere_at<false, HAS_MOTION>(sc, L, i, rtime, c, r);
                hit = BOUNDED ? sphere_hit_tmin(sub(ro, c), rd, a, r, tMin, t) && t < tMax : sphere_hit(sub(ro, c), rd, a, r, t);
            }
            if (!hit) continue;
            if (ANY) {
                if (t < __builtin_inff()) { best = t; prim = i; break; }
            } else if (t < best || (t == best && prim >= 0 && rank[i] < rank[prim])) { best = t; prim = i; }
        }
        if (ANY && prim >= 0) {
            cur = -1;                                                          // the answer is in: leave through the loop's one exit (a second exit costs every visit mask bookkeeping)
        } else if (inner == 2) {
            const int far = entry[1] < entry[0] ? 0 : 1;                       // near child first
            if (!stack.push(next[far])) ok = false;                            // (cannot happen for a tree within its own depth bound; never drop a subtree silently)
            cur = next[1 - far];
        } else if (inner == 1) {
            cur = next[0];
        } else {
            cur = stack.empty() ? -1 : stack.pop();
        }
    }
    bestT = best;
    bestPrim = prim;
    rtimeOut = rtime;
    return ok;
}

// the intervals the interval calls trace (NaN fails): everything else reports a miss
__host__ __device__ __forceinline__ bool interval_is_traced(float tMin, float tMax) { return 0.0f <= tMin && tMin <= tMax; }

} // namespace

} // namespace rtow
