// rtow_api_post.hip - the post-pass entry points of the C ABI (include/rtow.h): metrics, combine / finalize, the denoisers, moments, reprojection, rectification,
// noise mask, upsampling, pixel lists, bloom, exposure and tone mapping.  Each one refuses (rtow_validate.h: every check that needs no device), takes the context's lock,
// and launches on the caller's stream.  The tails are written out: HIP_TRY logs the text of the expression that failed.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "../../include/rtow.h"
#include "rtow_context.h"

using namespace rtow;

extern "C" {

RTOW_API int rtowReduceMetricsDevice(RtowContext ctx, int32_t pixelCount, const void* diagnostics, int32_t diagnosticsStride, const float* color,
                                     const float* sampleCountWeight, void* stream, RtowMetrics* outMetrics)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateReduceMetrics(pixelCount, diagnostics, diagnosticsStride, color, sampleCountWeight, outMetrics));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    if (ctx->haveMetricsDone) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evMetricsDone, 0), RTOW_ERROR_LAUNCH_FAILURE);      // an asynchronous reduction may still be folding the partials
    HIP_TRY(ctx, launchReduceMetrics(pixelCount, (const uint8_t*)diagnostics, diagnosticsStride, color, sampleCountWeight, ctx->dPartials, s),
            RTOW_ERROR_LAUNCH_FAILURE);
    // the per-block partials are folded on the device and the 40-byte record lands in pinned host memory by the time the stream is idle: no 8 KB copy of the partials, no
    // DMA of its own (round 4 copied and folded them on the host: 44.6 us per call at 1920 x 1080 against 18.6 us of kernels)
    HIP_TRY(ctx, launchFoldMetrics(ctx->dPartials, ctx->dMetricsRecord, s), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipStreamSynchronize(s), RTOW_ERROR_LAUNCH_FAILURE);
    memcpy(outMetrics, (const void*)ctx->hMetricsRecord, sizeof(RtowMetrics));
    return RTOW_SUCCESS;
}

RTOW_API int rtowCombineDevice(RtowContext ctx, const RtowCombineParams* params, const float* inColor, const float* inNormal, const float* inAlbedo,
                               float* outColor, float* outNormal, float* outAlbedo, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateCombine(params, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchCombine(*params, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowFinalizeDevice(RtowContext ctx, int32_t pixelCount, const float* inColor, const float* inNormal, const float* inAlbedo,
                                uint8_t* outColor, uint8_t* outNormal, uint8_t* outAlbedo, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateFinalize(pixelCount, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchFinalize(pixelCount, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo, ctx->dByteThresholds, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowDenoiseDevice(RtowContext ctx, const RtowDenoiseParams* params, const float* inColor, const float* inNormal, const float* inAlbedo,
                               void* scratch, float* outColor, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateDenoise(params, inColor, inNormal, inAlbedo, scratch, outColor));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchDenoise(*params, inColor, inNormal, inAlbedo, (float*)scratch, outColor, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowAccumulateMomentsDevice(RtowContext ctx, int32_t pixelCount, int32_t count, const float* const* colors, const float* inMoments, float* outMoments,
                                         void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateAccumulateMoments(pixelCount, count, colors, inMoments, outMoments));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchAccumulateMoments(pixelCount, count, colors, inMoments, outMoments, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowDenoiseVarianceDevice(RtowContext ctx, const RtowDenoiseParams* params, const float* inColor, const float* inNormal, const float* inAlbedo,
                                       const float* moments, void* scratch, float* outColor, float* outVariance, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateDenoiseVariance(params, inColor, inNormal, inAlbedo, moments, scratch, outColor, outVariance));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchDenoiseVariance(*params, inColor, inNormal, inAlbedo, moments, (float*)scratch, outColor, outVariance, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowReprojectAccumDevice(RtowContext ctx, const RtowReprojectParams* params, const RtowRay* rays, const RtowHitBuffers* hits, const RtowHitBuffers* previousHits,
                                      const RtowAccumBuffers* previous, const RtowAccumBuffers* out, int32_t* outSource, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    ReprojectConstants k;
    RTOW_TRY(validateReproject(params, rays, hits, previousHits, previous, out, nullptr, nullptr, outSource, &k));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchReproject(*params, k, rays, *hits, *previousHits, *previous, *out, outSource, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowReprojectAccumBilinearDevice(RtowContext ctx, const RtowReprojectParams* params, const RtowRay* rays, const RtowHitBuffers* hits,
                                              const RtowHitBuffers* previousHits, const RtowAccumBuffers* previous, const RtowAccumBuffers* out,
                                              const float* previousMoments, int32_t maxBatches, float* outMoments, int32_t* outSource, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    ReprojectConstants k;
    RTOW_TRY(validateReprojectBilinear(params, rays, hits, previousHits, previous, out, previousMoments, maxBatches, outMoments, outSource, &k));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchReprojectBilinear(*params, k, rays, *hits, *previousHits, *previous, *out, previousMoments, maxBatches, outMoments, outSource, s),
            RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowReprojectMomentsDevice(RtowContext ctx, int32_t pixelCount, const int32_t* source, const float* previousMoments, int32_t maxBatches, float* outMoments,
                                        void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateReprojectMoments(pixelCount, source, previousMoments, maxBatches, outMoments));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchReprojectMoments(pixelCount, source, previousMoments, maxBatches, outMoments, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowEstimateMomentsDevice(RtowContext ctx, const RtowEstimateMomentsParams* params, const float* color, const RtowHitBuffers* hits, const float* inMoments,
                                       float* outMoments, uint8_t* outFilled, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateEstimateMoments(params, color, hits, inMoments, outMoments, outFilled));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchEstimateMoments(*params, color, *hits, inMoments, outMoments, outFilled, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowNoiseMaskDevice(RtowContext ctx, const RtowNoiseMaskParams* params, const float* moments, uint8_t* outMask, float* outError, RtowNoiseStats* outStats,
                                 void* scratch, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateNoiseMask(params, moments, outMask, outError, outStats, scratch));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchNoiseMask(*params, moments, outMask, outError, outStats, scratch, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowRectifyHistoryDevice(RtowContext ctx, const RtowRectifyParams* params, const RtowAccumBuffers* history, const float* fresh, const RtowHitBuffers* hits,
                                      const float* inMoments, const RtowAccumBuffers* out, float* outMoments, float* outKeep, RtowRectifyStats* outStats, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateRectifyHistory(params, history, fresh, hits, inMoments, out, outMoments, outKeep, outStats));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchRectifyHistory(*params, *history, fresh, *hits, inMoments, *out, outMoments, outKeep, outStats, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowUpsampleDevice(RtowContext ctx,const RtowUpsampleParams* params, const float* srcColor, const RtowHitBuffers* srcHits, const float* srcAlbedo,
                                const RtowHitBuffers* dstHits, const float* dstAlbedo, float* outColor, uint8_t* outStage, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateUpsample(params, srcColor, srcHits, srcAlbedo, dstHits, dstAlbedo, outColor, outStage));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    const bool guided = params->mode == RTOW_UPSAMPLE_GUIDED;      // the other modes read no hit set: theirs may be null
    const RtowHitBuffers none{};
    HIP_TRY(ctx, launchUpsample(*params, srcColor, guided ? *srcHits : none, srcAlbedo, guided ? *dstHits : none, dstAlbedo, outColor, outStage, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowBuildPixelListDevice(RtowContext ctx, const RtowPixelListParams* params, const float* color, const uint8_t* mask, void* scratch, const RtowPixelList* list,
                                      void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateBuildPixelList(params, color, mask, scratch, list));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchBuildPixelList(*params, color, mask, (unsigned*)scratch, list->words, list->capacity, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowAddAccumDevice(RtowContext ctx, int32_t pixelCount, const RtowAccumBuffers* dst, const RtowAccumBuffers* src, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateAddAccum(pixelCount, dst, src));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    float* const d[4] = {dst->color, dst->normal, dst->albedo, dst->sampleCountWeight};
    const float* const q[4] = {src->color, src->normal, src->albedo, src->sampleCountWeight};
    HIP_TRY(ctx, launchAddAccum((size_t)pixelCount, d, q, s), RTOW_ERROR_LAUNCH_FAILURE);      // one launch for the four buffers
    return RTOW_SUCCESS;
}

RTOW_API int rtowCombineFinalizeDevice(RtowContext ctx, const RtowCombineParams* params, const float* inColor, const float* inNormal, const float* inAlbedo,
                                       uint8_t* outColor, uint8_t* outNormal, uint8_t* outAlbedo, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateCombine(params, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchCombineFinalize(*params, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo, ctx->dByteThresholds, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowMeterExposureDevice(RtowContext ctx, const RtowExposureParams* params, const float* inColor, void* scratch, RtowExposureState* state, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateMeterExposure(params, inColor, scratch, state));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchMeterExposure(*params, inColor, scratch, state, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowFinalizeToneMappedDevice(RtowContext ctx, const RtowToneMapParams* params, const RtowExposureState* state, const float* inColor, const float* inNormal,
                                          const float* inAlbedo, uint8_t* outColor, uint8_t* outNormal, uint8_t* outAlbedo, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateFinalizeToneMapped(params, state, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchFinalizeToneMapped(*params, state, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo, ctx->dByteThresholds, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowBloomDevice(RtowContext ctx, const RtowBloomParams* params, const RtowExposureState* state, const float* inColor, void* scratch, float* outColor,
                             void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateBloom(params, state, inColor, scratch, outColor));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    HIP_TRY(ctx, launchBloom(*params, state, inColor, scratch, outColor, s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowReduceMetricsDeviceAsync(RtowContext ctx, int32_t pixelCount, const void* diagnostics, int32_t diagnosticsStride, const float* color,
                                          const float* sampleCountWeight, void* stream, RtowMetrics* outMetrics)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateReduceMetrics(pixelCount, diagnostics, diagnosticsStride, color, sampleCountWeight, outMetrics));
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    // where the record goes: memory registered with rtowRegisterHostBuffer (the device writes it over PCIe), else a device pointer (any HIP allocation)
    RtowMetrics* target = (RtowMetrics*)mappedHost(ctx, outMetrics, sizeof(RtowMetrics));
    if (!target) {
        hipPointerAttribute_t attr{};
        if (hipPointerGetAttributes(&attr, outMetrics) != hipSuccess) { (void)hipGetLastError(); return RTOW_ERROR_INVALID_VALUE; }   // plain pageable host memory: the device cannot write it
        if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeHost && attr.type != hipMemoryTypeManaged) return RTOW_ERROR_INVALID_VALUE;
        target = attr.type == hipMemoryTypeHost && attr.devicePointer ? (RtowMetrics*)attr.devicePointer : outMetrics;
    }
    // the partials are one block per context: this reduction starts after the previous one's fold has read them
    if (ctx->haveMetricsDone) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evMetricsDone, 0), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, launchReduceMetrics(pixelCount, (const uint8_t*)diagnostics, diagnosticsStride, color, sampleCountWeight, ctx->dPartials, s), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, launchFoldMetrics(ctx->dPartials, target, s), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventRecord(ctx->evMetricsDone, s), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->haveMetricsDone = true;
    return RTOW_SUCCESS;
}

} // extern "C"
