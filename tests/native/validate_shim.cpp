// Test-only C wrappers around the argument checks of the C ABI (csrc/rtow_validate.h), so that tests/test_validate.py calls them without a device: built together with
// csrc/rtow_validate.cpp by a plain C++ compiler, without contraction.  Addresses arrive as integers and are never dereferenced.
#include "../../raytracing-in-one-weekend_amd/csrc/rtow_validate.h"

using namespace rtow;
#define SHIM extern "C" __attribute__((visibility("default")))
typedef const float* F;
typedef const uint8_t* B;
typedef const void* V;

// ranges: written, then read, then same - base and bytes side by side
SHIM int shim_aliasing_ok(const uint64_t* base, const uint64_t* bytes, int nWritten, int nRead, int nSame)
{
    Range r[64];
    const int n = nWritten + nRead + nSame;
    if (n > 64) return -1;
    for (int i = 0; i < n; ++i) r[i] = {(const void*)(uintptr_t)base[i], (size_t)bytes[i]};
    return aliasingOk(r, nWritten, r + nWritten, nRead, nSame ? r + nWritten + nRead : nullptr, nSame) ? 1 : 0;
}
SHIM int shim_overlaps(uint64_t a, uint64_t aBytes, uint64_t b, uint64_t bBytes) { return overlaps({(V)(uintptr_t)a, (size_t)aBytes}, {(V)(uintptr_t)b, (size_t)bBytes}) ? 1 : 0; }
SHIM void shim_reproject_constants(const RtowView* v, float out[5])
{
    const ReprojectConstants k = reprojectConstants(*v);
    out[0] = k.LF; out[1] = k.LR; out[2] = k.LU; out[3] = k.HR; out[4] = k.VU;
}
SHIM int shim_moments_max_batches() { return kMomentsMaxBatches; }

SHIM int shim_params(const RtowSampleParams* p) { return validateParams(p); }
SHIM int shim_view_size(const RtowTraceViewParams* v) { return viewSizeValid(*v) ? 1 : 0; }
SHIM int shim_guide_arguments(const RtowGuideParams* p, const RtowGuideBuffers* out) { return guideArgumentsValid(p, out) ? 1 : 0; }
SHIM int shim_shade_hits(const RtowShadeHitsParams* p, int32_t count, const RtowRay* rays, const int32_t* entity, const RtowSurfaceBuffers* s) { return validateShadeHits(p, count, rays, entity, s); }
SHIM int shim_reduce_metrics(int32_t n, V diag, int32_t stride, F color, F scw, const RtowMetrics* out) { return validateReduceMetrics(n, diag, stride, color, scw, out); }
SHIM int shim_combine(const RtowCombineParams* p, F c, F n, F a, V oc, V on, V oa) { return validateCombine(p, c, n, a, oc, on, oa); }
SHIM int shim_finalize(int32_t count, F c, F n, F a, B oc, B on, B oa) { return validateFinalize(count, c, n, a, oc, on, oa); }
SHIM int shim_add_accum(int32_t count, const RtowAccumBuffers* dst, const RtowAccumBuffers* src) { return validateAddAccum(count, dst, src); }
SHIM int shim_denoise(const RtowDenoiseParams* p, F c, F n, F a, V scratch, F out) { return validateDenoise(p, c, n, a, scratch, out); }
SHIM int shim_accumulate_moments(int32_t pixels, int32_t count, const float* const* colors, F in, F out) { return validateAccumulateMoments(pixels, count, colors, in, out); }
SHIM int shim_denoise_variance(const RtowDenoiseParams* p, F c, F n, F a, F m, V scratch, F out, F var) { return validateDenoiseVariance(p, c, n, a, m, scratch, out, var); }
SHIM int shim_reproject(const RtowReprojectParams* p, const RtowRay* rays, const RtowHitBuffers* hits, const RtowHitBuffers* prevHits, const RtowAccumBuffers* prev,
                        const RtowAccumBuffers* out, const int32_t* source, float k[5])
{
    ReprojectConstants c{};
    const int rc = validateReproject(p, rays, hits, prevHits, prev, out, nullptr, nullptr, source, &c);
    if (k) { k[0] = c.LF; k[1] = c.LR; k[2] = c.LU; k[3] = c.HR; k[4] = c.VU; }
    return rc;
}
SHIM int shim_reproject_bilinear(const RtowReprojectParams* p, const RtowRay* rays, const RtowHitBuffers* hits, const RtowHitBuffers* prevHits, const RtowAccumBuffers* prev,
                                 const RtowAccumBuffers* out, F prevMoments, int32_t maxBatches, F outMoments, const int32_t* source)
{
    ReprojectConstants c{};
    return validateReprojectBilinear(p, rays, hits, prevHits, prev, out, prevMoments, maxBatches, outMoments, source, &c);
}
SHIM int shim_reproject_moments(int32_t pixels, const int32_t* source, F prev, int32_t maxBatches, F out) { return validateReprojectMoments(pixels, source, prev, maxBatches, out); }
SHIM int shim_estimate_moments(const RtowEstimateMomentsParams* p, F color, const RtowHitBuffers* hits, F in, F out, B filled) { return validateEstimateMoments(p, color, hits, in, out, filled); }
SHIM int shim_noise_mask(const RtowNoiseMaskParams* p, F moments, B mask, F error, const RtowNoiseStats* stats, V scratch) { return validateNoiseMask(p, moments, mask, error, stats, scratch); }
SHIM int shim_rectify_history(const RtowRectifyParams* p, const RtowAccumBuffers* history, F fresh, const RtowHitBuffers* hits, F in, const RtowAccumBuffers* out, F outMoments,
                              F keep, const RtowRectifyStats* stats)
{
    return validateRectifyHistory(p, history, fresh, hits, in, out, outMoments, keep, stats);
}
SHIM int shim_upsample(const RtowUpsampleParams* p, F src, const RtowHitBuffers* srcHits, F srcAlbedo, const RtowHitBuffers* dstHits, F dstAlbedo, F out, B stage)
{
    return validateUpsample(p, src, srcHits, srcAlbedo, dstHits, dstAlbedo, out, stage);
}
SHIM int shim_build_pixel_list(const RtowPixelListParams* p, F color, B mask, V scratch, const RtowPixelList* list) { return validateBuildPixelList(p, color, mask, scratch, list); }
SHIM int shim_meter_exposure(const RtowExposureParams* p, F color, V scratch, const RtowExposureState* state) { return validateMeterExposure(p, color, scratch, state); }
SHIM int shim_finalize_tone_mapped(const RtowToneMapParams* p, const RtowExposureState* state, F c, F n, F a, B oc, B on, B oa) { return validateFinalizeToneMapped(p, state, c, n, a, oc, on, oa); }
