// rtow_validate.h - what the entry points of the C ABI refuse before they take their lock: pure functions of a few structs and addresses.  Host only, no HIP: it
// includes include/rtow.h and standard headers, so a plain C++ compiler builds rtow_validate.cpp and the tests run it without a device (tests/test_validate.py).
// No address given to a validator is ever dereferenced, only the parameter structs and the structs of pointers (RtowHitBuffers, RtowAccumBuffers, RtowPixelList).
#pragma once
#include <cfloat>
#include <cstddef>
#include <cstdint>

#include "../../include/rtow.h"

namespace rtow {

// ---- aliasing: a caller's buffer, and whether two of them share a byte (a null buffer shares none) ----
struct Range { const void* base; size_t bytes; };
inline bool overlaps(const Range& a, const Range& b)
{
    return a.base && b.base && (uintptr_t)a.base < (uintptr_t)b.base + b.bytes && (uintptr_t)b.base < (uintptr_t)a.base + a.bytes;
}

// The one aliasing rule of the post passes:
//   - no written buffer shares a byte with a buffer that is read,
//   - no two written buffers share a byte,
//   - an output may be the matching input only where the pass reads a pixel before it writes it: written[i] may overlap same[k] only when i == k and the bases are equal.
bool aliasingOk(const Range* written, int nWritten, const Range* read, int nRead, const Range* same = nullptr, int nSame = 0);

// ---- the repeated parameter idioms ----
inline bool frameSizeValid(int32_t width, int32_t height) { return width > 0 && height > 0 && (int64_t)width * height <= INT32_MAX; }
inline bool finiteNonNegative(float x) { return x >= 0.0f && x <= FLT_MAX; }      // NaN fails
inline bool normalSharpnessValid(int32_t s) { return s >= 0 && s <= 8; }
inline bool flagsValid(int32_t flags, int32_t mask, int32_t reserved) { return (flags & ~mask) == 0 && reserved == 0; }
inline bool accumBuffersGiven(const RtowAccumBuffers& b) { return b.color && b.normal && b.albedo && b.sampleCountWeight; }
// a query has to be asked for at least one of distance / entityIndex / normal
inline bool anyHitBuffer(const RtowHitBuffers& h) { return h.distance || h.entityIndex || h.normal; }
inline bool allHitBuffers(const RtowHitBuffers& h) { return h.distance && h.entityIndex && h.normal; }
// what the two denoisers check of their parameters
bool denoiseParamsValid(const RtowDenoiseParams& p);

// rtowAccumulateMomentsDevice: colour buffers of one call (their device pointers travel in the kernel arguments)
constexpr int kMomentsMaxBatches = 16;

// rtowReprojectAccumDevice: the constants of previousView the specification has the host compute, in float32 (every unit that includes this header is compiled
// without contraction)
struct ReprojectConstants { float LF, LR, LU, HR, VU; };
inline ReprojectConstants reprojectConstants(const RtowView& v)
{
    const auto dot = [](const RtowFloat3& a, const RtowFloat3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; };
    return ReprojectConstants{dot(v.lowerLeftCorner, v.forward), dot(v.lowerLeftCorner, v.right), dot(v.lowerLeftCorner, v.up), dot(v.horizontal, v.right), dot(v.vertical, v.up)};
}

// ---- one validator per entry point: the entry point's arguments without the context and the stream; RTOW_SUCCESS or the code the entry point returns ----
// the sample entry points: every batch's params (a trace depth beyond 64 is RTOW_ERROR_CAPACITY)
int validateParams(const RtowSampleParams* p);
// the queries: the size of a view (rtowTraceViewDevice, rtowTraceGuideViewDevice), what both guide calls check of their parameters and outputs, rtowShadeHitsDevice
bool viewSizeValid(const RtowTraceViewParams& v);
bool guideArgumentsValid(const RtowGuideParams* params, const RtowGuideBuffers* out);
int validateShadeHits(const RtowShadeHitsParams* params, int32_t count, const RtowRay* rays, const int32_t* entityIndex, const RtowSurfaceBuffers* surface);
// rtowRecordPathsDevice (RTOW_ERROR_UNSUPPORTED: a policy other than the reference stream; the sizes of the outputs are taken in 64 bits)
int validateRecordPaths(const RtowSampleParams* batch, const RtowRecordPathsParams* params, const RtowPixelList* list, const float* inColor,
                        const float* inSampleCountWeight, const RtowPathSummary* summaries, const RtowPathSegment* segments);
// the post passes
int validateReduceMetrics(int32_t pixelCount, const void* diagnostics, int32_t diagnosticsStride, const float* color, const float* sampleCountWeight,
                          const RtowMetrics* outMetrics);      // both forms: pointers, count and stride
int validateCombine(const RtowCombineParams* params, const float* inColor, const float* inNormal, const float* inAlbedo, const void* outColor, const void* outNormal,
                    const void* outAlbedo);                    // rtowCombineDevice and rtowCombineFinalizeDevice
int validateFinalize(int32_t pixelCount, const float* inColor, const float* inNormal, const float* inAlbedo, const uint8_t* outColor, const uint8_t* outNormal,
                     const uint8_t* outAlbedo);
int validateAddAccum(int32_t pixelCount, const RtowAccumBuffers* dst, const RtowAccumBuffers* src);
int validateDenoise(const RtowDenoiseParams* params, const float* inColor, const float* inNormal, const float* inAlbedo, const void* scratch, const float* outColor);
int validateAccumulateMoments(int32_t pixelCount, int32_t count, const float* const* colors, const float* inMoments, const float* outMoments);
int validateDenoiseVariance(const RtowDenoiseParams* params, const float* inColor, const float* inNormal, const float* inAlbedo, const float* moments, const void* scratch,
                            const float* outColor, const float* outVariance);
// rtowReprojectAccumDevice (previousMoments and outMoments null: a null range overlaps nothing) and what rtowReprojectAccumBilinearDevice refuses like it; fills `k`
int validateReproject(const RtowReprojectParams* params, const RtowRay* rays, const RtowHitBuffers* hits, const RtowHitBuffers* previousHits,
                      const RtowAccumBuffers* previous, const RtowAccumBuffers* out, const float* previousMoments, const float* outMoments, const int32_t* outSource,
                      ReprojectConstants* k);
int validateReprojectBilinear(const RtowReprojectParams* params, const RtowRay* rays, const RtowHitBuffers* hits, const RtowHitBuffers* previousHits,
                              const RtowAccumBuffers* previous, const RtowAccumBuffers* out, const float* previousMoments, int32_t maxBatches, const float* outMoments,
                              const int32_t* outSource, ReprojectConstants* k);
int validateReprojectMoments(int32_t pixelCount, const int32_t* source, const float* previousMoments, int32_t maxBatches, const float* outMoments);
int validateEstimateMoments(const RtowEstimateMomentsParams* params, const float* color, const RtowHitBuffers* hits, const float* inMoments, const float* outMoments,
                            const uint8_t* outFilled);
int validateNoiseMask(const RtowNoiseMaskParams* params, const float* moments, const uint8_t* outMask, const float* outError, const RtowNoiseStats* outStats,
                      const void* scratch);
int validateRectifyHistory(const RtowRectifyParams* params, const RtowAccumBuffers* history, const float* fresh, const RtowHitBuffers* hits, const float* inMoments,
                           const RtowAccumBuffers* out, const float* outMoments, const float* outKeep, const RtowRectifyStats* outStats);
int validateUpsample(const RtowUpsampleParams* params, const float* srcColor, const RtowHitBuffers* srcHits, const float* srcAlbedo, const RtowHitBuffers* dstHits,
                     const float* dstAlbedo, const float* outColor, const uint8_t* outStage);
int validateBuildPixelList(const RtowPixelListParams* params, const float* color, const uint8_t* mask, const void* scratch, const RtowPixelList* list);
int validateMeterExposure(const RtowExposureParams* params, const float* inColor, const void* scratch, const RtowExposureState* state);
int validateFinalizeToneMapped(const RtowToneMapParams* params, const RtowExposureState* state, const float* inColor, const float* inNormal, const float* inAlbedo,
                               const uint8_t* outColor, const uint8_t* outNormal, const uint8_t* outAlbedo);
// rtowBloomDevice: outColor may be inColor itself (equal bases), the one overlap the pass allows
int validateBloom(const RtowBloomParams* params, const RtowExposureState* state, const float* inColor, const void* scratch, const float* outColor);

} // namespace rtow
