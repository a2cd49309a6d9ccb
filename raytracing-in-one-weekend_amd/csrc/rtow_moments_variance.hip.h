// rtow_moments_variance.hip.h - from the luminance moments (s1, s2, n) of rtowAccumulateMomentsDevice to the variance of the mean of the batches, once, for the passes
// that read it (rtow_denoise_variance.hip: v0 of rtowDenoiseVarianceDevice; rtow_noise_mask.hip: e(q) of rtowNoiseMaskDevice).  One float32 operation of the
// specification in include/rtow.h after the other (the units are compiled without contraction).
#pragma once
#include "rtow_denoise_taps.hip.h"

namespace rtow {
namespace taps {

// false: no estimate (n is not >= 2, a NaN n included).  true: mean = s1 / n and v = max(0, s2 - s1 * mean) / (n * (n - 1)); the caller decides what a non-finite v means.
__device__ __forceinline__ bool mean_variance(P3 m, float& mean, float& v)
{
    const float s1 = m.x, s2 = m.y, n = m.z;
    if (!(n >= 2.0f)) return false;
    mean = s1 / n;
    float d = s2 - s1 * mean;
    d = d > 0.0f ? d : 0.0f;
    v = d / (n * (n - 1.0f));
    return true;
}

}  // namespace taps
}  // namespace rtow
