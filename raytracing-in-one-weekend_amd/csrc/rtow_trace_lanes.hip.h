// rtow_trace_lanes.hip.h - what one lane of a device ray query needs besides the walk: its column of the workgroup's LDS stack, its ray of the caller's array (load_ray) or the camera
// ray of its pixel (view forms), the winner's world-space normal and the store of its result - and the launcher's part that does not depend on the kernel.  Shared by rtow_trace.hip (rtowTraceRaysDevice /
// rtowTraceViewDevice), rtow_trace_interval.hip (rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice) and rtow_guides.hip (rtowTraceGuideRaysDevice /
// rtowTraceGuideViewDevice): one launch shape, DESIGN.md 4.2.
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

// Ray `index` of a caller's array: origin, direction and Ray.Time
__device__ __forceinline__ void load_ray(const RtowRay* rays, size_t index, V3& ro, V3& rd, float& time)
{
    const Ray8 r = reinterpret_cast<const Ray8*>(rays)[index];
    ro = v3(r.ox, r.oy, r.oz);
    time = r.time;
    rd = v3(r.dx, r.dy, r.dz);
}

// The camera ray of pixel (cx, cy): REGEN of the sample kernel (JOBS/SampleBatchJob.cs:134, RT/View.cs:38-47) with the jitter at the pixel centre and no lens offset
__device__ __forceinline__ V3 view_direction(const RtowView& VW, int cx, int cy, float frameX, float frameY)
{
    const V3 viewLLC = v3(VW.lowerLeftCorner), viewH = v3(VW.horizontal), viewV = v3(VW.vertical);
    const float jx = 0.5f, jy = 0.5f;
    const float u = ((float)cx + jx) / frameX;
    const float v = ((float)cy + jy) / frameY;
    return normalize(v3(viewLLC.x + u * viewH.x + v * viewV.x,
                        viewLLC.y + u * viewH.y + v * viewV.y,
                        viewLLC.z + u * viewH.z + v * viewV.z));
}

// The view forms' lane -> pixel map: wave = 8 x 8 pixel tile (view_tile: the wave's; a kernel leaves when it is not below A.tiles), lane = (lane & 7, lane >> 3) inside
// it (view_pixel; a kernel leaves when the pixel is outside the frame), and that pixel's index and ray (view_ray).  Args: the kernel's argument struct with the fields
// set_view fills.  (Three steps with the two exits left to the kernel: as one function that returns "no pixel" the view kernels compile to more registers.)
__device__ __forceinline__ unsigned long long view_tile() { return (unsigned long long)blockIdx.x * (kTraceBlock / 64) + (threadIdx.x >> 6); }
template <typename Args>
__device__ __forceinline__ void view_pixel(const Args& A, unsigned long long tile, int& cx, int& cy)
{
    cx = (int)(tile % A.tilesX) * 8 + (int)(threadIdx.x & 7u);
    cy = (int)(tile / A.tilesX) * 8 + (int)((threadIdx.x >> 3) & 7u);
}
template <typename Args>
__device__ __forceinline__ void view_ray(const Args& A, int cx, int cy, size_t& index, V3& ro, V3& rd, float& time)
{
    index = (size_t)cy * (size_t)A.width + (size_t)cx;
    ro = v3(A.view.origin);
    rd = view_direction(A.view, cx, cy, A.sizeX, A.sizeY);
    time = A.time;
}

// the view fields of a view form's argument struct; returns the workgroups of its launch
template <typename Args>
unsigned long long set_view(Args& A, const RtowTraceViewParams& p)
{
    A.view = p.view;
    A.time = p.time;
    A.sizeX = (float)p.width;       // SampleBatchJob.Size is a float2 (JOBS/SampleBatchJob.cs:24)
    A.sizeY = (float)p.height;
    A.width = p.width;
    A.height = p.height;
    A.tilesX = ((unsigned)p.width + 7u) / 8u;
    A.tiles = (unsigned long long)A.tilesX * (((unsigned long long)p.height + 7u) / 8u);
    return (A.tiles + kTraceBlock / 64 - 1) / (kTraceBlock / 64);
}

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

// A lane's result into the caller's buffers A.hits: the distance and the host's entity index (A.scene.entityOfPrim: primitive -> entity, or null for the same number) of the
// hit the walk found; a miss stores +inf and -1.  Args: the kernel's argument struct, whose member `scene` is the launch's SceneBinding (rtow_kernels.h).
template <typename Args>
__device__ __forceinline__ void store_hit_place(const Args& A, size_t index, float t, int prim)
{
    if (A.hits.distance) A.hits.distance[index] = t;
    if (A.hits.entityIndex) A.hits.entityIndex[index] = prim >= 0 && A.scene.entityOfPrim ? A.scene.entityOfPrim[prim] : prim;
}
// ... and its normal, for a caller who asked for it (A.hits.normal is not null)
template <typename Args>
__device__ __forceinline__ void store_hit_normal(const Args& A, size_t index, V3 n)
{
    float* o = A.hits.normal + index * 3u;
    o[0] = n.x; o[1] = n.y; o[2] = n.z;
}

// The whole result of a query lane: the hit the walk found in A.scene under `tMin` (0 for the open form), the normal derived only where the caller asks for
// it; a miss stores +inf, -1 and a zero normal
template <int BASE, typename Args>
__device__ __forceinline__ void store_hit(const Args& A, size_t index, V3 ro, V3 rd, float rtime, float tMin, float t, int prim)
{
    store_hit_place(A, index, t, prim);
    if (A.hits.normal) {
        V3 n = v3(0, 0, 0);
        if (prim >= 0) n = hit_normal<BASE>(global_scene(A.scene.blob), A.scene.layout, prim, ro, rd, rtime, tMin, t);
        store_hit_normal(A, index, n);
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
