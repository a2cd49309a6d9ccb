// rtow_api_query.hip - the ray-query entry points of the C ABI (include/rtow.h): the two host probes, the trace calls, the shade pass and the guide calls.  A device
// query refuses what needs no device (its own null checks over the predicates of rtow_validate.h), then beginQuery: the context's lock, the scene, the device and the
// stream; then its empty count, if it has one, and its launch over the one description of the resident scene, queryScene (rtow_context.h).  A bad call therefore
// hears of its arguments first, then of a missing scene, then succeeds on an empty count.  rtowRecordPathsDevice, which is fed by the batch planner, is in rtow_api.hip.
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/rtow.h"
#include "rtow_context.h"

using namespace rtow;

namespace {

// The two probes.  The host image of the scene has a lock of its own (held here and while rtowUploadScene swaps the image in): the blocking entry points hold ctx->mu
// for a whole batch, and a probe from another thread must not wait for them.  No device work: batches in flight are neither waited for nor disturbed
int probe(RtowContext ctx, const RtowFloat3* origin, const RtowFloat3* direction, float time, bool interval, float tMin, float tMax, float* distance, int32_t* entityIndex)
{
    if (!ctx || !origin || !direction) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->sceneMu);
    if (!ctx->haveScene) return RTOW_ERROR_NO_SCENE;
    const float o[3] = {origin->x, origin->y, origin->z}, d[3] = {direction->x, direction->y, direction->z};
    float t = 0.0f;
    int prim = -1;
    if (interval) (void)probeIntervalHost(ctx->scene.blob.data(), ctx->scene.layout, entityMapHost(ctx), o, d, time, tMin, tMax, false, &t, &prim);
    else (void)probeNearestHitHost(ctx->scene.blob.data(), ctx->scene.layout, entityMapHost(ctx), o, d, time, &t, &prim);
    if (distance) *distance = t;
    if (entityIndex) *entityIndex = prim;
    return RTOW_SUCCESS;
}

// What every device query does between its argument check and its launch: the lock, RTOW_ERROR_NO_SCENE without a scene, this thread on the context's device and the
// stream the work goes to (useDevice)
int beginQuery(RtowContext ctx, std::unique_lock<std::mutex>& lock, void* stream, hipStream_t* s)
{
    lock = std::unique_lock<std::mutex>(ctx->mu);
    if (!ctx->haveScene) return RTOW_ERROR_NO_SCENE;
    return useDevice(ctx, stream, s);
}

} // namespace

extern "C" {

RTOW_API int rtowProbeNearestHit(RtowContext ctx, const RtowFloat3* origin, const RtowFloat3* direction, float time, float* distance, int32_t* entityIndex)
{
    return probe(ctx, origin, direction, time, false, 0.0f, 0.0f, distance, entityIndex);
}

RTOW_API int rtowProbeNearestHitInterval(RtowContext ctx, const RtowFloat3* origin, const RtowFloat3* direction, float time, float tMin, float tMax, float* distance,
                                         int32_t* entityIndex)
{
    return probe(ctx, origin, direction, time, true, tMin, tMax, distance, entityIndex);
}

RTOW_API int rtowTraceRaysDevice(RtowContext ctx, int32_t count, const RtowRay* rays, const RtowHitBuffers* hits, void* stream)
{
    if (!ctx || !rays || !hits || count < 0) return RTOW_ERROR_INVALID_VALUE;
    if (!anyHitBuffer(*hits)) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginQuery(ctx, lock, stream, &s));
    if (count == 0) return RTOW_SUCCESS;
    HIP_TRY(ctx, launchTraceRays(queryScene(ctx), count, rays, *hits, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowTraceViewDevice(RtowContext ctx, const RtowTraceViewParams* params, const RtowHitBuffers* hits, RtowRay* outRays, void* stream)
{
    if (!ctx || !params || !hits) return RTOW_ERROR_INVALID_VALUE;
    if (!anyHitBuffer(*hits)) return RTOW_ERROR_INVALID_VALUE;
    if (!viewSizeValid(*params)) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginQuery(ctx, lock, stream, &s));
    HIP_TRY(ctx, launchTraceView(queryScene(ctx), *params, *hits, outRays, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowTraceRaysIntervalDevice(RtowContext ctx, int32_t count, const RtowRay* rays, const RtowRayInterval* intervals, const RtowHitBuffers* hits, void* stream)
{
    if (!ctx || !rays || !hits || count < 0) return RTOW_ERROR_INVALID_VALUE;
    if (!anyHitBuffer(*hits)) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginQuery(ctx, lock, stream, &s));
    if (count == 0) return RTOW_SUCCESS;
    HIP_TRY(ctx, launchTraceRaysInterval(queryScene(ctx), count, rays, intervals, *hits, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowTraceOcclusionDevice(RtowContext ctx, int32_t count, const RtowRay* rays, const RtowRayInterval* intervals, uint8_t* occluded, void* stream)
{
    if (!ctx || !rays || !occluded || count < 0) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginQuery(ctx, lock, stream, &s));
    if (count == 0) return RTOW_SUCCESS;
    HIP_TRY(ctx, launchTraceOcclusion(queryScene(ctx), count, rays, intervals, occluded, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowShadeHitsDevice(RtowContext ctx, const RtowShadeHitsParams* params, int32_t count, const RtowRay* rays, const int32_t* entityIndex,
                                 const RtowSurfaceBuffers* surface, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateShadeHits(params, count, rays, entityIndex, surface));
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginQuery(ctx, lock, stream, &s));
    if (count == 0) return RTOW_SUCCESS;
    if (!ctx->scene.entityOfPrim.empty() && !ctx->dPrimOfEntity) return RTOW_ERROR_INTERNAL;      // (an upload that failed half way: the old scene's description, no map)
    HIP_TRY(ctx, launchShadeHits(queryScene(ctx), params->environment, count, rays, entityIndex, *surface, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowTraceGuideRaysDevice(RtowContext ctx, const RtowGuideParams* params, int32_t count, const RtowRay* rays, const RtowGuideBuffers* out, void* stream)
{
    if (!ctx || !rays || count < 0 || !guideArgumentsValid(params, out)) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginQuery(ctx, lock, stream, &s));
    if (count == 0) return RTOW_SUCCESS;
    HIP_TRY(ctx, launchTraceGuideRays(queryScene(ctx), params->maxBounces, count, rays, *out, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowTraceGuideViewDevice(RtowContext ctx, const RtowGuideParams* params, const RtowTraceViewParams* view, const RtowGuideBuffers* out, void* stream)
{
    if (!ctx || !view || !guideArgumentsValid(params, out)) return RTOW_ERROR_INVALID_VALUE;
    if (!viewSizeValid(*view)) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginQuery(ctx, lock, stream, &s));
    HIP_TRY(ctx, launchTraceGuideView(queryScene(ctx), params->maxBounces, *view, *out, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

} // extern "C"
