// rtow_trace_interval.hip - rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice: ray queries with a parameter interval (tMin, tMax) against the resident scene, on the device.
//
// The many-ray form of rtowProbeNearestHitInterval: the interval forms of `walk` (rtow_walk.hip.h, the text the host probe compiles), one lane per ray, on the device image of the scene.
//  * nearest (ANY = false): distance, the host's entity index and the world-space normal of the nearest Entity.Hit(r, tMin, tMax) - with (0, +inf) what rtow_trace.hip's
//    ray form stores, bit for bit;
//  * occlusion (ANY = true): one byte per ray, 1 if any entity has Entity.Hit(r, tMin, tMax) - the walk returns at the first accepted hit.
// A ray whose interval is not traced (interval_is_traced: 0 <= tMin <= tMax, NaN fails) reports a miss / 0 without a walk.
//
// Launch shape: rtow_trace.hip's ray form - 256-lane workgroups, one lane per ray, no barrier, no scratch, tree and primitives from HBM / L2, the
// [entry][lane] LDS stack of rtow_trace_lanes.hip.h (26 x 256 x 4 B).  A lane that has its answer leaves the loop; its wave goes on until its last lane has.
#include "rtow_trace_lanes.hip.h"

namespace rtow {

namespace {

// an interval at a 4-byte aligned address
struct __attribute__((packed, aligned(4))) Interval2 { float tMin, tMax; };
static_assert(sizeof(Interval2) == sizeof(RtowRayInterval), "RtowRayInterval is two floats");

struct IntervalArgs {
    SceneBinding scene;             // device image of the scene, entity map, layout (rtow_kernels.h)
    const RtowRay* rays;
    const RtowRayInterval* intervals;   // null: (0, +inf) for every ray
    long long count;
    RtowHitBuffers hits;            // nearest form
    uint8_t* occluded;              // occlusion form
};

template <int BASE, bool ANY>
__global__ void __launch_bounds__(kTraceBlock) interval_kernel(IntervalArgs A)
{
    __shared__ int stackRows[kTraceStackEntries * kTraceBlock];
    const long long i = (long long)blockIdx.x * kTraceBlock + threadIdx.x;
    if (i >= A.count) return;
    const size_t index = (size_t)i;
    V3 ro, rd;
    float time;
    load_ray(A.rays, index, ro, rd, time);
    float tMin = 0.0f, tMax = __builtin_inff();
    if (A.intervals) {
        const Interval2 iv = reinterpret_cast<const Interval2*>(A.intervals)[index];
        tMin = iv.tMin;
        tMax = iv.tMax;
    }
    float t = __builtin_inff(), rtime = time;
    int prim = -1;
    if (interval_is_traced(tMin, tMax)) {
        LdsStack stack;
        stack.col = stackRows + threadIdx.x;
        stack.sp = 0;
        (void)walk<BASE, ANY ? WALK_ANY : WALK_NEAREST>(A.scene.blob, A.scene.layout, ro, rd, time, tMin, tMax, stack, t, prim, rtime);      // (the launcher refuses a tree deeper than the stack: push cannot fail)
    }
    if (ANY) {
        A.occluded[index] = prim >= 0 ? 1 : 0;
        return;
    }
    store_hit<BASE>(A, index, ro, rd, rtime, tMin, t, prim);
}

template <bool ANY>
hipError_t launch(const IntervalArgs& A, hipStream_t stream)
{
    return launch_query(A.scene.layout, ((unsigned long long)A.count + kTraceBlock - 1) / kTraceBlock,
                        [&](auto base, dim3 grid, dim3 block) { hipLaunchKernelGGL((interval_kernel<decltype(base)::value, ANY>), grid, block, 0, stream, A); });
}

}  // namespace

hipError_t launchTraceRaysInterval(const QueryScene& scene, int64_t count, const RtowRay* rays, const RtowRayInterval* intervals, const RtowHitBuffers& hits, hipStream_t stream)
{
    IntervalArgs A{};
    A.scene = scene.binding;
    A.rays = rays;
    A.intervals = intervals;
    A.count = count;
    A.hits = hits;
    return launch<false>(A, stream);
}

hipError_t launchTraceOcclusion(const QueryScene& scene, int64_t count, const RtowRay* rays, const RtowRayInterval* intervals, uint8_t* occluded, hipStream_t stream)
{
    IntervalArgs A{};
    A.scene = scene.binding;      // (the entity map travels along unread: the occlusion form stores no entity)
    A.rays = rays;
    A.intervals = intervals;
    A.count = count;
    A.occluded = occluded;
    return launch<true>(A, stream);
}

}  // namespace rtow
