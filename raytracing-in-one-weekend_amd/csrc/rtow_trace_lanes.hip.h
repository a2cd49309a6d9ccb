// rtow_trace_lanes.hip.h - what one lane of a device ray query needs besides the walk: its column of the workgroup's LDS stack, the ray record at a 4-byte aligned
// address and the winner's world-space normal.  Shared by rtow_trace.hip (rtowTraceRaysDevice / rtowTraceViewDevice) and rtow_trace_interval.hip
// (rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice): one launch shape, DESIGN.md 4.2.
#pragma once
#include "rtow_walk.hip.h"

#include "rtow_bvh.h"

namespace rtow {

namespace {

constexpr int kTraceBlock = 256;
constexpr int kTraceStackEntries = RTOW_STACK_CAPACITY + 2;

// a lane's column of the workgroup's [entry][lane] LDS array
struct LdsStack {
    int* col;
    int sp;
    __device__ __forceinline__ bool push(int x)
    {
        if (sp >= kTraceStackEntries) return false;
        col[sp * kTraceBlock] = x;
        sp++;
        return true;
    }
    __device__ __forceinline__ int pop() { sp--; return col[sp * kTraceBlock]; }
    __device__ __forceinline__ bool empty() const { return sp == 0; }
};

// a ray at a 4-byte aligned address (a caller may pass a view that starts anywhere in an allocation)
struct __attribute__((packed, aligned(4))) Ray8 { float ox, oy, oz, time, dx, dy, dz, pad; };
static_assert(sizeof(Ray8) == sizeof(RtowRay), "RtowRay is eight floats");

// HitRecord.Normal of primitive `prim` hit at distance t: what the sample kernel's HIT stage derives (RT/Entity.cs:62-66) - the winner's test once more (with the tMin the
// walk gave it: a sphere's far root or a box's exit face are the winner's only under that tMin) for its entity-space normal, rotated out and normalised; spheres of the
// sphere kinds: r.GetPoint(t) / radius, normalised
template <int BASE>
__device__ __forceinline__ V3 hit_normal(const SceneRefs& sc, const SceneLayout& L, int prim, V3 ro, V3 rd, float rtime, float tMin, float t)
{
    if (BASE >= SCENE_KIND_GENERAL) {
        const unsigned mi = *reinterpret_cast<const unsigned*>(section<false>(sc, L.matIndexOffset) + (uint32_t)prim * 4u);
        float t2; V3 nLocal; float4 rq;
        (void)general_hit<false>(sc, L, prim, mi >> kPrimTypeShift, ro, rd, rtime, tMin, t2, nLocal, rq);
        return normalize(rotate(rq, nLocal));
    }
    V3 c; float radius;
    sphere_at<false, BASE == SCENE_KIND_SPHERES_MOTION>(sc, L, prim, rtime, c, radius);
    const V3 oc = sub(ro, c);
    const V3 nLocal = div3(v3(oc.x + t * rd.x, oc.y + t * rd.y, oc.z + t * rd.z), radius);
    return normalize(nLocal);
}

} // namespace

} // namespace rtow
