// rtow_validate.cpp - the argument checks of the C ABI (rtow_validate.h).  Host only: no HIP header, no device, nothing dereferenced but the parameter structs.
// Per pass, what is specific is the list of buffers with their bytes per pixel; the rules are aliasingOk and the predicates of the header.
#include "rtow_validate.h"

#include <initializer_list>

namespace rtow {

namespace {
constexpr int kBad = RTOW_ERROR_INVALID_VALUE;
template <int N> constexpr int countOf(const Range (&)[N]) { return N; }
}

bool aliasingOk(const Range* written, int nWritten, const Range* read, int nRead, const Range* same, int nSame)
{
    for (int i = 0; i < nWritten; ++i) {
        for (int r = 0; r < nRead; ++r)
            if (overlaps(written[i], read[r])) return false;
        for (int k = 0; k < nSame; ++k)
            if (!(i == k && written[i].base == same[k].base) && overlaps(written[i], same[k])) return false;
        for (int j = i + 1; j < nWritten; ++j)
            if (overlaps(written[i], written[j])) return false;
    }
    return true;
}

bool denoiseParamsValid(const RtowDenoiseParams& p)
{
    if (!frameSizeValid(p.width, p.height)) return false;
    if (p.iterations < 1 || p.iterations > 8 || !normalSharpnessValid(p.normalSharpness)) return false;
    if (!finiteNonNegative(p.colorSigma) || !finiteNonNegative(p.albedoSigma)) return false;
    return flagsValid(p.flags, RTOW_DENOISE_DEMODULATE_ALBEDO, p.reserved);
}

int validateParams(const RtowSampleParams* p)
{
    if (!p) return RTOW_ERROR_INVALID_VALUE;
    // Size is a float2 whose fraction is honoured; the frame is (int) Size.  NaN, an infinity, anything below 1 or from 2^31 on is refused before the cast sees it
    for (const float s : {p->size.x, p->size.y})
        if (!(s >= 1.0f && s < 2147483648.0f)) return RTOW_ERROR_INVALID_VALUE;
    const int w = (int)p->size.x, h = (int)p->size.y;
    if (w <= 0 || h <= 0 || (long long)w * h > 0x7fffffffLL) return RTOW_ERROR_INVALID_VALUE;
    if (p->sliceDivider < 1 || p->sliceOffset < 0 || p->sliceOffset >= p->sliceDivider) return RTOW_ERROR_INVALID_VALUE;
    if (p->traceDepth < 1 || p->traceDepth > 64) return p->traceDepth < 1 ? RTOW_ERROR_INVALID_VALUE : RTOW_ERROR_CAPACITY;
    if (p->noiseColor < RTOW_NOISE_WHITE || p->noiseColor > RTOW_NOISE_SPATIOTEMPORAL_BLUE) return RTOW_ERROR_INVALID_VALUE;
    if (p->rngPolicy != RTOW_RNG_REFERENCE && p->rngPolicy != RTOW_RNG_PER_SAMPLE && p->rngPolicy != RTOW_RNG_PER_SAMPLE_XOROSHIRO) return RTOW_ERROR_INVALID_VALUE;
    if (p->rngPolicy != RTOW_RNG_REFERENCE && p->noiseColor != RTOW_NOISE_WHITE) return RTOW_ERROR_INVALID_VALUE;   // the texture walks are per pixel by construction
    if (p->environment.skyType < RTOW_SKY_NONE || p->environment.skyType > RTOW_SKY_CUBEMAP) return RTOW_ERROR_INVALID_VALUE;
    if (p->diagnosticsStride != 4 && p->diagnosticsStride != 16) return RTOW_ERROR_INVALID_VALUE;
    return RTOW_SUCCESS;
}

bool viewSizeValid(const RtowTraceViewParams& v) { return frameSizeValid(v.width, v.height) && v.reserved == 0; }

bool guideArgumentsValid(const RtowGuideParams* params, const RtowGuideBuffers* out)
{
    if (!params || !out) return false;
    if (params->maxBounces < 0 || params->maxBounces > RTOW_GUIDE_MAX_BOUNCES || params->flags != 0 || params->reserved != 0) return false;
    return anyHitBuffer(out->hits) || out->rays || out->throughput || out->pathDistance || out->bounces || out->end;
}

int validateShadeHits(const RtowShadeHitsParams* params, int32_t count, const RtowRay* rays, const int32_t* entityIndex, const RtowSurfaceBuffers* surface)
{
    if (!params || !rays || !entityIndex || !surface || count < 0) return kBad;
    if (!surface->albedo && !surface->emission && !surface->texCoord && !surface->metallicGlossiness && !surface->materialIndex && !surface->materialInfo) return kBad;
    if (params->flags != 0 || params->reserved != 0) return kBad;
    const int32_t sky = params->environment.skyType;
    if (sky != RTOW_SKY_NONE && sky != RTOW_SKY_GRADIENT && sky != RTOW_SKY_CUBEMAP) return kBad;
    return RTOW_SUCCESS;
}

int validateRecordPaths(const RtowSampleParams* batch, const RtowRecordPathsParams* params, const RtowPixelList* list, const float* inColor,
                        const float* inSampleCountWeight, const RtowPathSummary* summaries, const RtowPathSegment* segments)
{
    if (!batch || !params || !list || !list->words || !inColor || !inSampleCountWeight || !summaries) return kBad;
    const int v = validateParams(batch);
    if (v != RTOW_SUCCESS) return v;
    if (batch->sliceOffset != 0 || batch->sliceDivider != 1) return kBad;                                     // the list alone says which pixels
    const uint64_t n = (uint64_t)(int)batch->size.x * (uint64_t)(int)batch->size.y;
    if (n > (uint64_t)RTOW_PIXEL_LIST_MAX_PIXELS) return kBad;
    if (params->select != RTOW_PATH_SELECT_INDEX && params->select != RTOW_PATH_SELECT_BRIGHTEST) return kBad;
    if (params->sampleIndex < 0 || (params->select == RTOW_PATH_SELECT_BRIGHTEST && params->sampleIndex != 0)) return kBad;
    if (params->flags != 0 || params->reserved != 0) return kBad;
    if (batch->rngPolicy != RTOW_RNG_REFERENCE) return RTOW_ERROR_UNSUPPORTED;
    // capacity <= 2^32 - 1 and traceDepth <= 64: the products fit 64 bits; what does not fit behind its base address is refused, not wrapped
    const uint64_t capacity = list->capacity;
    const uint64_t summaryBytes = capacity * sizeof(RtowPathSummary), segmentBytes = capacity * (uint64_t)batch->traceDepth * sizeof(RtowPathSegment);
    if (summaryBytes > UINTPTR_MAX - (uintptr_t)summaries) return kBad;
    if (segments && segmentBytes > UINTPTR_MAX - (uintptr_t)segments) return kBad;
    // every lane writes its own slots while others read the list and the accumulators
    const Range written[] = {{summaries, (size_t)summaryBytes}, {segments, (size_t)segmentBytes}};                 // segments may be null
    const Range read[] = {{list->words, RTOW_PIXEL_LIST_BYTES(list->capacity)}, {inColor, (size_t)n * 16}, {inSampleCountWeight, (size_t)n * 4}};
    return aliasingOk(written, countOf(written), read, countOf(read)) ? RTOW_SUCCESS : kBad;
}

int validateReduceMetrics(int32_t pixelCount, const void* diagnostics, int32_t diagnosticsStride, const float* color, const float* sampleCountWeight,
                          const RtowMetrics* outMetrics)
{
    if (!diagnostics || !color || !sampleCountWeight || !outMetrics || pixelCount <= 0) return kBad;
    if (diagnosticsStride != 4 && diagnosticsStride != 16) return kBad;
    return RTOW_SUCCESS;
}

int validateCombine(const RtowCombineParams* params, const float* inColor, const float* inNormal, const float* inAlbedo, const void* outColor, const void* outNormal,
                    const void* outAlbedo)
{
    if (!params || !inColor || !inNormal || !inAlbedo || !outColor || !outNormal || !outAlbedo) return kBad;
    if (!frameSizeValid(params->width, params->height)) return kBad;      // the kernels index pixels in int: width * height beyond INT32_MAX would wrap to an empty launch
    return RTOW_SUCCESS;
}

int validateFinalize(int32_t pixelCount, const float* inColor, const float* inNormal, const float* inAlbedo, const uint8_t* outColor, const uint8_t* outNormal,
                     const uint8_t* outAlbedo)
{
    if (pixelCount <= 0 || !inColor || !inNormal || !inAlbedo || !outColor || !outNormal || !outAlbedo) return kBad;
    return RTOW_SUCCESS;
}

int validateAddAccum(int32_t pixelCount, const RtowAccumBuffers* dst, const RtowAccumBuffers* src)
{
    if (!dst || !src || pixelCount <= 0) return kBad;
    if (!accumBuffersGiven(*dst) || !accumBuffersGiven(*src)) return kBad;
    return RTOW_SUCCESS;
}

int validateDenoise(const RtowDenoiseParams* params, const float* inColor, const float* inNormal, const float* inAlbedo, const void* scratch, const float* outColor)
{
    if (!params || !inColor || !inNormal || !inAlbedo || !outColor) return kBad;
    const RtowDenoiseParams& p = *params;
    if (!denoiseParamsValid(p)) return kBad;
    if (!scratch && p.iterations > 1) return kBad;
    // the levels write outColor and scratch while they read the inputs and each other
    const size_t bytes = RTOW_DENOISE_SCRATCH_BYTES(p.width, p.height);      // the one length every buffer is checked with
    const Range written[] = {{outColor, bytes}, {scratch, bytes}};
    const Range read[] = {{inColor, bytes}, {inNormal, bytes}, {inAlbedo, bytes}};
    return aliasingOk(written, countOf(written), read, countOf(read)) ? RTOW_SUCCESS : kBad;
}

int validateAccumulateMoments(int32_t pixelCount, int32_t count, const float* const* colors, const float* inMoments, const float* outMoments)
{
    if (!colors || !outMoments || pixelCount <= 0 || count < 1 || count > kMomentsMaxBatches) return kBad;
    // a lane reads its own pixel of every buffer before it writes its own moments: the only overlap that is safe is inMoments == outMoments
    const Range written[] = {{outMoments, (size_t)pixelCount * 12}}, same[] = {{inMoments, (size_t)pixelCount * 12}};
    Range read[kMomentsMaxBatches];
    for (int k = 0; k < count; ++k) {
        if (!colors[k]) return kBad;
        read[k] = {colors[k], (size_t)pixelCount * 16};
    }
    return aliasingOk(written, 1, read, count, same, 1) ? RTOW_SUCCESS : kBad;
}

int validateDenoiseVariance(const RtowDenoiseParams* params, const float* inColor, const float* inNormal, const float* inAlbedo, const float* moments, const void* scratch,
                            const float* outColor, const float* outVariance)
{
    if (!params || !inColor || !inNormal || !inAlbedo || !moments || !scratch || !outColor) return kBad;
    const RtowDenoiseParams& p = *params;
    if (!denoiseParamsValid(p)) return kBad;
    // the levels write outColor, outVariance and the scratch while they read the inputs and each other
    const size_t n = (size_t)p.width * (size_t)p.height;
    const Range written[] = {{outColor, n * 12}, {scratch, RTOW_DENOISE_VARIANCE_SCRATCH_BYTES(p.width, p.height)}, {outVariance, n * 4}};     // outVariance may be null
    const Range read[] = {{inColor, n * 12}, {inNormal, n * 12}, {inAlbedo, n * 12}, {moments, n * 12}};
    return aliasingOk(written, countOf(written), read, countOf(read)) ? RTOW_SUCCESS : kBad;
}

int validateReproject(const RtowReprojectParams* params, const RtowRay* rays, const RtowHitBuffers* hits, const RtowHitBuffers* previousHits,
                      const RtowAccumBuffers* previous, const RtowAccumBuffers* out, const float* previousMoments, const float* outMoments, const int32_t* outSource,
                      ReprojectConstants* k)
{
    if (!params || !rays || !hits || !previousHits || !previous || !out) return kBad;
    if (!hits->distance || !hits->entityIndex || !previousHits->distance || !previousHits->entityIndex) return kBad;
    if (!accumBuffersGiven(*previous) || !accumBuffersGiven(*out)) return kBad;
    const RtowReprojectParams& p = *params;
    if (!frameSizeValid(p.width, p.height)) return kBad;
    if (!finiteNonNegative(p.depthTolerance) || p.maxHistory < 1) return kBad;
    if (!flagsValid(p.flags, RTOW_REPROJECT_MATCH_ENTITY, p.reserved)) return kBad;
    *k = reprojectConstants(p.previousView);
    for (const float d : {k->LF, k->HR, k->VU})
        if (!(d != 0.0f && d >= -FLT_MAX && d <= FLT_MAX)) return kBad;      // the divisors of the projection
    // every pixel gathers from arbitrary pixels of the previous frame: no byte the pass writes may be one it gathers from, or another output's
    const size_t n = (size_t)p.width * (size_t)p.height;
    const Range written[] = {{out->color, n * 16}, {out->normal, n * 12}, {out->albedo, n * 12}, {out->sampleCountWeight, n * 4}, {outSource, n * 4}, {outMoments, n * 12}};
    const Range gathered[] = {{previous->color, n * 16}, {previous->normal, n * 12}, {previous->albedo, n * 12}, {previous->sampleCountWeight, n * 4},
                              {previousHits->distance, n * 4}, {previousHits->entityIndex, n * 4}, {previousMoments, n * 12}};
    return aliasingOk(written, countOf(written), gathered, countOf(gathered)) ? RTOW_SUCCESS : kBad;
}

int validateReprojectBilinear(const RtowReprojectParams* params, const RtowRay* rays, const RtowHitBuffers* hits, const RtowHitBuffers* previousHits,
                              const RtowAccumBuffers* previous, const RtowAccumBuffers* out, const float* previousMoments, int32_t maxBatches, const float* outMoments,
                              const int32_t* outSource, ReprojectConstants* k)
{
    if ((previousMoments == nullptr) != (outMoments == nullptr) || (outMoments && maxBatches < 1)) return kBad;
    return validateReproject(params, rays, hits, previousHits, previous, out, previousMoments, outMoments, outSource, k);
}

int validateReprojectMoments(int32_t pixelCount, const int32_t* source, const float* previousMoments, int32_t maxBatches, const float* outMoments)
{
    if (!source || !previousMoments || !outMoments || pixelCount <= 0 || maxBatches < 1) return kBad;
    // every pixel gathers from an arbitrary pixel of the previous moments
    const Range written[] = {{outMoments, (size_t)pixelCount * 12}};
    const Range read[] = {{source, (size_t)pixelCount * 4}, {previousMoments, (size_t)pixelCount * 12}};
    return aliasingOk(written, countOf(written), read, countOf(read)) ? RTOW_SUCCESS : kBad;
}

int validateEstimateMoments(const RtowEstimateMomentsParams* params, const float* color, const RtowHitBuffers* hits, const float* inMoments, const float* outMoments,
                            const uint8_t* outFilled)
{
    if (!params || !color || !hits || !outMoments) return kBad;
    if (!allHitBuffers(*hits)) return kBad;
    const RtowEstimateMomentsParams& p = *params;
    if (!frameSizeValid(p.width, p.height)) return kBad;
    if (p.minBatches < 1 || p.minTaps < 2 || p.minTaps > 49 || !normalSharpnessValid(p.normalSharpness)) return kBad;
    if (!finiteNonNegative(p.depthTolerance)) return kBad;
    if (!flagsValid(p.flags, RTOW_ESTIMATE_MOMENTS_MATCH_ENTITY, p.reserved)) return kBad;
    // a pixel reads the colour and the guides of its neighbourhood, the moments only at itself: the one overlap that is safe is inMoments == outMoments
    const size_t n = (size_t)p.width * (size_t)p.height;
    const Range written[] = {{outMoments, n * 12}, {outFilled, n}};      // outFilled may be null
    const Range same[] = {{inMoments, n * 12}};
    const Range read[] = {{color, n * 16}, {hits->distance, n * 4}, {hits->entityIndex, n * 4}, {hits->normal, n * 12}};
    return aliasingOk(written, countOf(written), read, countOf(read), same, countOf(same)) ? RTOW_SUCCESS : kBad;
}

int validateNoiseMask(const RtowNoiseMaskParams* params, const float* moments, const uint8_t* outMask, const float* outError, const RtowNoiseStats* outStats,
                      const void* scratch)
{
    if (!params || !moments || !outMask || !scratch) return kBad;
    const RtowNoiseMaskParams& p = *params;
    if (!frameSizeValid(p.width, p.height)) return kBad;
    if (!(p.errorThreshold > 0.0f && p.errorThreshold <= FLT_MAX) || !finiteNonNegative(p.luminanceFloor)) return kBad;   // NaN fails both
    if (p.dilate < 0 || p.dilate > 3 || p.maxQualifying < 0) return kBad;
    if (!flagsValid(p.flags, RTOW_NOISE_MASK_ABSOLUTE | RTOW_NOISE_MASK_UNKNOWN_QUALIFIES, p.reserved)) return kBad;
    // a pixel reads the moments of its neighbourhood while other pixels are written, and the record is filled by atomics
    const size_t n = (size_t)p.width * (size_t)p.height;
    const Range written[] = {{outMask, n}, {outError, n * 4}, {outStats, sizeof(RtowNoiseStats)}, {scratch, RTOW_NOISE_MASK_SCRATCH_BYTES}};      // outError / outStats may be null
    const Range read[] = {{moments, n * 12}};
    return aliasingOk(written, countOf(written), read, countOf(read)) ? RTOW_SUCCESS : kBad;
}

int validateRectifyHistory(const RtowRectifyParams* params, const RtowAccumBuffers* history, const float* fresh, const RtowHitBuffers* hits, const float* inMoments,
                           const RtowAccumBuffers* out, const float* outMoments, const float* outKeep, const RtowRectifyStats* outStats)
{
    if (!params || !history || !fresh || !hits || !out) return kBad;
    if (!allHitBuffers(*hits)) return kBad;
    if (!accumBuffersGiven(*history) || !accumBuffersGiven(*out)) return kBad;
    const RtowRectifyParams& p = *params;
    if (!frameSizeValid(p.width, p.height)) return kBad;
    if (p.radius < 1 || p.radius > 3 || p.minTaps < 2 || p.minTaps > (2 * p.radius + 1) * (2 * p.radius + 1)) return kBad;
    if (!normalSharpnessValid(p.normalSharpness)) return kBad;
    if (!finiteNonNegative(p.depthTolerance) || !finiteNonNegative(p.sigmaScale) || !finiteNonNegative(p.relativeTolerance)) return kBad;
    if (!flagsValid(p.flags, RTOW_RECTIFY_MATCH_ENTITY, p.reserved)) return kBad;
    if ((inMoments == nullptr) != (outMoments == nullptr)) return kBad;
    // a pixel reads the fresh colour and the guides of its neighbourhood, the history and the moments only at itself, before it writes them: the overlaps that are safe
    // are an output that IS the matching input (written[k] and same[k])
    const size_t n = (size_t)p.width * (size_t)p.height;
    const Range written[] = {{out->color, n * 16}, {out->normal, n * 12}, {out->albedo, n * 12}, {out->sampleCountWeight, n * 4}, {outMoments, n * 12},
                             {outKeep, n * 4}, {outStats, sizeof(RtowRectifyStats)}};      // outKeep / outStats may be null
    const Range same[] = {{history->color, n * 16}, {history->normal, n * 12}, {history->albedo, n * 12}, {history->sampleCountWeight, n * 4}, {inMoments, n * 12}};
    const Range read[] = {{fresh, n * 16}, {hits->distance, n * 4}, {hits->entityIndex, n * 4}, {hits->normal, n * 12}};
    return aliasingOk(written, countOf(written), read, countOf(read), same, countOf(same)) ? RTOW_SUCCESS : kBad;
}

int validateUpsample(const RtowUpsampleParams* params, const float* srcColor, const RtowHitBuffers* srcHits, const float* srcAlbedo, const RtowHitBuffers* dstHits,
                     const float* dstAlbedo, const float* outColor, const uint8_t* outStage)
{
    if (!params || !srcColor || !outColor) return kBad;
    const RtowUpsampleParams& p = *params;
    for (const int32_t size : {p.srcWidth, p.srcHeight, p.dstWidth, p.dstHeight})
        if (size < 1 || size > 16384) return kBad;
    if (p.mode != RTOW_UPSAMPLE_POINT && p.mode != RTOW_UPSAMPLE_BILINEAR && p.mode != RTOW_UPSAMPLE_GUIDED) return kBad;
    if (!normalSharpnessValid(p.normalSharpness) || !finiteNonNegative(p.depthTolerance)) return kBad;
    if (!flagsValid(p.flags, RTOW_UPSAMPLE_MATCH_ENTITY | RTOW_UPSAMPLE_DEMODULATE_ALBEDO, p.reserved)) return kBad;
    const bool guided = p.mode == RTOW_UPSAMPLE_GUIDED, demod = (p.flags & RTOW_UPSAMPLE_DEMODULATE_ALBEDO) != 0;
    if (p.mode == RTOW_UPSAMPLE_POINT && p.flags != 0) return kBad;
    if (!guided && (p.flags & RTOW_UPSAMPLE_MATCH_ENTITY) != 0) return kBad;
    if (guided && (!srcHits || !dstHits || !allHitBuffers(*srcHits) || !allHitBuffers(*dstHits))) return kBad;
    if (demod && (!srcAlbedo || !dstAlbedo)) return kBad;
    // a dst pixel reads src pixels and dst guides of other lanes' neighbourhoods: what is read depends on the mode
    const size_t ns = (size_t)p.srcWidth * (size_t)p.srcHeight, nd = (size_t)p.dstWidth * (size_t)p.dstHeight;
    const Range written[] = {{outColor, nd * 12}, {outStage, nd}};
    Range read[9] = {{srcColor, ns * 12}};
    int reads = 1;
    if (guided) {
        read[reads++] = {srcHits->distance, ns * 4}; read[reads++] = {srcHits->entityIndex, ns * 4}; read[reads++] = {srcHits->normal, ns * 12};
        read[reads++] = {dstHits->distance, nd * 4}; read[reads++] = {dstHits->entityIndex, nd * 4}; read[reads++] = {dstHits->normal, nd * 12};
    }
    if (demod) { read[reads++] = {srcAlbedo, ns * 12}; read[reads++] = {dstAlbedo, nd * 12}; }
    return aliasingOk(written, countOf(written), read, reads) ? RTOW_SUCCESS : kBad;
}

int validateBuildPixelList(const RtowPixelListParams* params, const float* color, const uint8_t* mask, const void* scratch, const RtowPixelList* list)
{
    if (!params || !list || !list->words || !scratch) return kBad;
    const RtowPixelListParams& p = *params;
    if (p.width <= 0 || p.height <= 0 || (int64_t)p.width * p.height > RTOW_PIXEL_LIST_MAX_PIXELS) return kBad;
    if (p.sliceDivider < 1 || p.sliceOffset < 0 || p.sliceOffset >= p.sliceDivider) return kBad;
    if (color && !(p.minSampleCount >= 0.0f)) return kBad;                                  // NaN fails
    if (p.flags != 0 || p.reserved != 0) return kBad;
    // the launches write the list and the scratch while they read the inputs and each other
    const size_t n = (size_t)p.width * (size_t)p.height;
    const Range written[] = {{list->words, RTOW_PIXEL_LIST_BYTES(list->capacity)}, {scratch, RTOW_PIXEL_LIST_SCRATCH_BYTES(p.width, p.height)}};
    const Range read[] = {{color, n * 16}, {mask, n}};
    return aliasingOk(written, countOf(written), read, countOf(read)) ? RTOW_SUCCESS : kBad;
}

int validateMeterExposure(const RtowExposureParams* params, const float* inColor, const void* scratch, const RtowExposureState* state)
{
    if (!params || !inColor || !scratch || !state) return kBad;
    const RtowExposureParams& p = *params;
    if (!frameSizeValid(p.width, p.height)) return kBad;
    if (p.lowPermille < 0 || p.lowPermille > p.highPermille || p.highPermille > 1000) return kBad;
    if (!(p.compensation >= -FLT_MAX && p.compensation <= FLT_MAX)) return kBad;      // NaN fails
    if (!(p.minStops >= -32.0f && p.minStops <= p.maxStops && p.maxStops <= 32.0f)) return kBad;
    if (!(p.rate >= 0.0f && p.rate <= 1.0f)) return kBad;
    if (p.flags != 0 || p.reserved != 0) return kBad;
    const size_t n = (size_t)p.width * (size_t)p.height;
    const Range written[] = {{scratch, RTOW_EXPOSURE_SCRATCH_BYTES}, {state, sizeof(RtowExposureState)}};
    const Range read[] = {{inColor, n * 12}};
    return aliasingOk(written, countOf(written), read, countOf(read)) ? RTOW_SUCCESS : kBad;
}

int validateFinalizeToneMapped(const RtowToneMapParams* params, const RtowExposureState* state, const float* inColor, const float* inNormal, const float* inAlbedo,
                               const uint8_t* outColor, const uint8_t* outNormal, const uint8_t* outAlbedo)
{
    if (!params || !inColor || !outColor) return kBad;
    if ((inNormal == nullptr) != (outNormal == nullptr) || (inAlbedo == nullptr) != (outAlbedo == nullptr)) return kBad;
    const RtowToneMapParams& p = *params;
    if (p.pixelCount <= 0) return kBad;
    if (p.curve != RTOW_TONE_CLAMP && p.curve != RTOW_TONE_ACES_FITTED && p.curve != RTOW_TONE_ACES_FILM) return kBad;
    if (!finiteNonNegative(p.exposure)) return kBad;
    if (p.flags != 0 || p.reserved[0] != 0 || p.reserved[1] != 0) return kBad;
    const size_t n = (size_t)p.pixelCount;
    const Range written[] = {{outColor, n * 4}, {outNormal, n * 4}, {outAlbedo, n * 4}};                 // the normal and albedo pairs may be null
    const Range read[] = {{inColor, n * 12}, {inNormal, n * 12}, {inAlbedo, n * 12}, {state, sizeof(RtowExposureState)}};
    return aliasingOk(written, countOf(written), read, countOf(read)) ? RTOW_SUCCESS : kBad;
}

int validateBloom(const RtowBloomParams* params, const RtowExposureState* state, const float* inColor, const void* scratch, const float* outColor)
{
    if (!params || !inColor || !scratch || !outColor) return kBad;
    const RtowBloomParams& p = *params;
    if (!frameSizeValid(p.width, p.height)) return kBad;
    if (p.levels < 1 || p.levels > 8) return kBad;
    if (!finiteNonNegative(p.threshold) || !finiteNonNegative(p.intensity)) return kBad;
    if (!(p.knee >= 0.0f && p.knee <= 1.0f) || !(p.scatter >= 0.0f && p.scatter <= 1.0f)) return kBad;      // NaN fails
    if (!(p.exposure >= 0.0f && p.exposure <= 65536.0f)) return kBad;
    if (!flagsValid(p.flags, RTOW_BLOOM_KARIS_AVERAGE, p.reserved)) return kBad;
    // the composite reads only its own pixel of inColor before it writes it; the pyramid is written while inColor and the state are read
    const size_t n = (size_t)p.width * (size_t)p.height;
    const Range written[] = {{outColor, n * 12}, {scratch, RTOW_BLOOM_SCRATCH_BYTES(p.width, p.height)}};
    const Range read[] = {{state, sizeof(RtowExposureState)}};
    const Range same[] = {{inColor, n * 12}};
    return aliasingOk(written, countOf(written), read, countOf(read), same, countOf(same)) ? RTOW_SUCCESS : kBad;
}

} // namespace rtow
