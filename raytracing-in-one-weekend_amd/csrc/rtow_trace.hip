// rtow_trace.hip - rtowTraceRaysDevice / rtowTraceViewDevice: batched nearest-hit queries against the resident scene, on the device.
//
// The many-ray form of rtowProbeNearestHit: the same walk (rtow_walk.hip.h, the text the host probe compiles) with the same hit tests, one lane per ray, on the device image
// of the scene.  Per ray: HitRecord.Distance, the host's entity index and the world-space HitRecord.Normal of the nearest Entity.Hit (tMin 0, tMax +inf).
//
// Launch shape:
//  * a plain grid of 256-lane workgroups, one lane per ray, no workgroup barrier - a lane that has no ray leaves at once;
//  * tree and primitives come from HBM / L2 (load_node<false>, general_hit<false>): the rays of a query are arbitrary and the kernel is short, staging the scene into LDS
//    per workgroup would cost more than it saves;
//  * the traversal stack (at most one pending far child per inner level of the tree: RTOW_STACK_CAPACITY, + 2 as the host probe reserves) is an LDS array [entry][lane]:
//    a lane's entries are 1 KB apart, the 64 lanes of a wave read 64 consecutive dwords - no bank conflict, no scratch; 26 x 256 x 4 B = 26 KB per workgroup, so LDS admits
//    six workgroups (24 waves) per CU; the kernels' register counts admit that too, but for the general ray form (90 VGPRs: five waves per SIMD;
//    tests/test_trace_rays_isa.py prints the counts);
//  * the view form maps a wave's 64 lanes to an 8 x 8 pixel tile, so that the rays of a wave stay together in the tree; its rays are the sample kernel's REGEN expressions with
//    SubPixelJitter off and LensRadius 0.
#include "rtow_trace_lanes.hip.h"

namespace rtow {

namespace {

struct TraceArgs {
    SceneBinding scene;             // device image of the scene, entity map, layout (rtow_kernels.h)
    RtowHitBuffers hits;
    // ray form
    const RtowRay* rays;
    long long count;
    // view form
    RtowRay* outRays;
    RtowView view;
    float time, sizeX, sizeY;
    int width, height;
    unsigned tilesX;
    unsigned long long tiles;
};

template <int BASE, bool VIEW>
__global__ void __launch_bounds__(kTraceBlock) trace_kernel(TraceArgs A)
{
    __shared__ int stackRows[kTraceStackEntries * kTraceBlock];
    size_t index;
    V3 ro, rd;
    float time;
    if (VIEW) {
        const unsigned long long tile = view_tile();
        if (tile >= A.tiles) return;
        int cx, cy;
        view_pixel(A, tile, cx, cy);
        if (cx >= A.width || cy >= A.height) return;
        view_ray(A, cx, cy, index, ro, rd, time);
        if (A.outRays) {
            reinterpret_cast<Ray8*>(A.outRays)[index] = Ray8{ro.x, ro.y, ro.z, time, rd.x, rd.y, rd.z, 0.0f};
        }
    } else {
        const long long i = (long long)blockIdx.x * kTraceBlock + threadIdx.x;
        if (i >= A.count) return;
        index = (size_t)i;
        load_ray(A.rays, index, ro, rd, time);
    }
    LdsStack stack;
    stack.col = stackRows + threadIdx.x;
    stack.sp = 0;
    float t, rtime;
    int prim;
    (void)walk<BASE, WALK_OPEN>(A.scene.blob, A.scene.layout, ro, rd, time, 0.0f, 0.0f, stack, t, prim, rtime);      // (the launcher refuses a tree deeper than the stack: push cannot fail)
    store_hit<BASE>(A, index, ro, rd, rtime, 0.0f, t, prim);
}

template <bool VIEW>
hipError_t launch(const TraceArgs& A, unsigned long long blocks, hipStream_t stream)
{
    return launch_query(A.scene.layout, blocks, [&](auto base, dim3 grid, dim3 block) { hipLaunchKernelGGL((trace_kernel<decltype(base)::value, VIEW>), grid, block, 0, stream, A); });
}

}  // namespace

hipError_t launchTraceRays(const QueryScene& scene, int64_t count, const RtowRay* rays, const RtowHitBuffers& hits, hipStream_t stream)
{
    TraceArgs A{};
    A.scene = scene.binding;
    A.hits = hits;
    A.rays = rays;
    A.count = count;
    return launch<false>(A, ((unsigned long long)count + kTraceBlock - 1) / kTraceBlock, stream);
}

hipError_t launchTraceView(const QueryScene& scene, const RtowTraceViewParams& p, const RtowHitBuffers& hits, RtowRay* outRays, hipStream_t stream)
{
    TraceArgs A{};
    A.scene = scene.binding;
    A.hits = hits;
    A.outRays = outRays;
    return launch<true>(A, set_view(A, p), stream);
}

}  // namespace rtow
