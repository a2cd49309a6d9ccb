// rtow_guide_weight.hip.h - the first-hit guide weight g(p, q) of include/rtow.h (rtowUpsampleDevice's specification), shared by the passes that weigh a neighbour by
// whether its first hit is the surface the pixel itself sees (rtow_upsample.hip: rtowUpsampleDevice; rtow_guided_halo.hip.h: the tap loop of rtowEstimateMomentsDevice
// and rtowRectifyHistoryDevice).  The rule exists once, here; every statement is one float32 operation of the specification (the units are compiled without contraction).
#pragma once
#include <hip/hip_runtime.h>

namespace rtow {
namespace guide {

// e, t, (nx, ny, nz): entityIndex, distance and normal of the pixel p.  `q` gives the other pixel's guides on demand - int entity(), float distance(),
// void normal(float&, float&, float&) - so that a caller reading them from global memory loads the distance only after the entity test passed and the normal only
// after the depth test did.
//   e < 0 (sky):  g = e' < 0 ? 1 : 0.
//   otherwise:    g = 0 if e' < 0; g = 0 if matchEntity and e' != e; g = 0 unless fabs(t' - t) <= depthTolerance * t (NaN fails); else d = (nx*nx' + ny*ny') + nz*nz',
//                 d = d > 0 ? d : 0, then d = d * d, normalSharpness times, and g = d.
template <class Q>
__device__ __forceinline__ float weight(int e, float t, float nx, float ny, float nz, int matchEntity, float depthTolerance, int normalSharpness, const Q& q)
{
    const int eq = q.entity();
    if (e < 0) return eq < 0 ? 1.0f : 0.0f;
    if (eq < 0 || (matchEntity && eq != e)) return 0.0f;
    const float tq = q.distance();
    if (!(__builtin_fabsf(tq - t) <= depthTolerance * t)) return 0.0f;          // NaN fails
    float qx, qy, qz;
    q.normal(qx, qy, qz);
    float d = (nx * qx + ny * qy) + nz * qz;
    d = d > 0.0f ? d : 0.0f;
    for (int k = 0; k < normalSharpness; ++k) d = d * d;
    return d;
}

}  // namespace guide
}  // namespace rtow
