// rtow_probe.hip - rtowProbeNearestHit / rtowProbeNearestHitInterval: one ray against the resident scene, walked on the HOST.
//
// Replaces the host's HitWorld (UNITY/Raytracer.cs:1353: BvhRoot->Hit(r, 0, +inf, out hitRec) -> the recursive HitTests.Hit(BvhNode), RT/HitTests.cs:152-196), which
// ScheduleSample calls with the camera's centre ray before every batch to set the focus distance (UNITY/Raytracer.cs:608-609) - the one reason a host that has handed
// its scene to this library would still keep its own serial RebuildBvh alive (UNITY/Raytracer.cs:1306-1351).
//
// Why not a launch: ScheduleSample runs while the previous batch is still tracing (two in flight, UNITY/Raytracer.cs:586-596), and the sample kernel owns every CU's
// register file and LDS until it ends - a probe kernel would start when that batch is over, and the host, waiting for it, could not queue the next batch in time.  One ray
// is microseconds of CPU work on the tree this library already built; the image of the scene (CompiledScene.blob, the very bytes the kernels read, with the derived
// transforms copied back after the device computed them) stays on the host for it.
//
// The walk itself (what it computes and why that is what the reference's recursion computes) is rtow_walk.hip.h: one text for this host walk and for the device queries of
// rtow_trace.hip.  HitWorld's own recursion prefers its right subtree on a tie of bit-identical distances; the walk names the entity that comes first in the reference
// tree's leaf order (what the sample path shades) - the host only reads the distance.
#include "rtow_walk.hip.h"

#include <vector>

namespace rtow {

namespace {

// one entry per inner level of the tree that was built (never more pending far children than that); grows rather than refuse
struct HostStack {
    std::vector<int> v;
    size_t sp = 0;
    explicit HostStack(size_t n) : v(n) {}
    bool push(int x) { if (sp == v.size()) v.resize(v.size() * 2); v[sp++] = x; return true; }
    int pop() { return v[--sp]; }
    bool empty() const { return sp == 0; }
};

// the walk of rtow_walk.hip.h in the form and for the scene kind that are known at run time only
template <bool BOUNDED>
void walkHost(const uint8_t* blob, const SceneLayout& L, V3 ro, V3 rd, float time, float tMin, float tMax, bool any, float& bestT, int& bestPrim)
{
    for_scene_base(L.sceneKind, [&](auto base) {
        constexpr int BASE = decltype(base)::value;
        HostStack stack((size_t)L.bvhDepth + 2u);
        float rtime;
        if (!BOUNDED) (void)walk<BASE, WALK_OPEN>(blob, L, ro, rd, time, tMin, tMax, stack, bestT, bestPrim, rtime);
        else if (any) (void)walk<BASE, WALK_ANY>(blob, L, ro, rd, time, tMin, tMax, stack, bestT, bestPrim, rtime);
        else (void)walk<BASE, WALK_NEAREST>(blob, L, ro, rd, time, tMin, tMax, stack, bestT, bestPrim, rtime);
    });
}

} // namespace

// blob: the HOST image of the scene, derived entity transforms included (rtowUploadScene copies them back).  entityOfPrim: CompiledScene.entityOfPrim (all-triangle scenes
// number their primitives in leaf order) or null.  Returns false on a miss.
bool probeNearestHitHost(const uint8_t* blob, const SceneLayout& L, const int32_t* entityOfPrim, const float origin[3], const float direction[3], float time, float* distance, int* entity)
{
    const V3 ro = v3(origin[0], origin[1], origin[2]), rd = v3(direction[0], direction[1], direction[2]);
    float t = __builtin_inff();
    int prim = -1;
    walkHost<false>(blob, L, ro, rd, time, 0.0f, 0.0f, false, t, prim);
    *distance = t;
    *entity = prim >= 0 && entityOfPrim ? entityOfPrim[prim] : prim;
    return prim >= 0;
}


// The interval form (rtowProbeNearestHitInterval): Entity.Hit(r, tMin, tMax) through the walk's interval forms.  any: stop at the first accepted hit - *distance and *entity are then
// that hit's, not the nearest's.  An interval that is not traced (interval_is_traced) is a miss.
bool probeIntervalHost(const uint8_t* blob, const SceneLayout& L, const int32_t* entityOfPrim, const float origin[3], const float direction[3], float time, float tMin, float tMax,
                       bool any, float* distance, int* entity)
{
    const V3 ro = v3(origin[0], origin[1], origin[2]), rd = v3(direction[0], direction[1], direction[2]);
    float t = __builtin_inff();
    int prim = -1;
    if (interval_is_traced(tMin, tMax)) walkHost<true>(blob, L, ro, rd, time, tMin, tMax, any, t, prim);
    *distance = t;
    *entity = prim >= 0 && entityOfPrim ? entityOfPrim[prim] : prim;
    return prim >= 0;
}

} // namespace rtow
