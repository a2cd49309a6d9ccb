// rtow_trace_lanes.hip.h - what one lane of a device ray query needs besides the walk: its column of the workgroup's LDS stack, the winner's world-space normal and the
// store of its result - and the launcher's part that does not depend on the kernel.  Shared by rtow_trace.hip (rtowTraceRaysDevice / rtowTraceViewDevice) and
// rtow_trace_interval.hip (rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice): one launch shape, DESIGN.md 4.2.
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

// A lane's result into the caller's buffers A.hits: the distance, the host's entity index (A.entityOfPrim: primitive -> entity, or null for the same number) and the normal
// of the hit the walk found in A.blob / A.layout under `tMin` (0 for the open form); a miss stores +inf, -1 and a zero normal.  Args: the kernel's argument struct.
template <int BASE, typename Args>
__device__ __forceinline__ void store_hit(const Args& A, size_t index, V3 ro, V3 rd, float rtime, float tMin, float t, int prim)
{
    if (A.hits.distance) A.hits.distance[index] = t;
    if (A.hits.entityIndex) A.hits.entityIndex[index] = prim >= 0 && A.entityOfPrim ? A.entityOfPrim[prim] : prim;
    if (A.hits.normal) {
        V3 n = v3(0, 0, 0);
        if (prim >= 0) n = hit_normal<BASE>(global_scene(A.blob), A.layout, prim, ro, rd, rtime, tMin, t);
        float* o = A.hits.normal + index * 3u;
        o[0] = n.x; o[1] = n.y; o[2] = n.z;
    }
}

// The launch of a query kernel on `blocks` workgroups of kTraceBlock lanes: launchKernel(base, grid, block) launches the unit's kernel for BASE = decltype(base)::value
template <typename F>
hipError_t launch_query(const SceneLayout& L, unsigned long long blocks, F&& launchKernel)
{
    if (L.bvhDepth + 2u > (unsigned)kTraceStackEntries) return hipErrorInvalidValue;      // compileScene builds to RTOW_STACK_CAPACITY: not reachable
    if (blocks == 0ull) return hipSuccess;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(kTraceBlock);
    for_scene_base(L.sceneKind, [&](auto base) { launchKernel(base, grid, block); });
    return hipGetLastError();
}

} // namespace

} // namespace rtow
