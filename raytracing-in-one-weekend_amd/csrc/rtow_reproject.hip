// rtow_reproject.hip - rtowReprojectAccumDevice's kernel: the previous view's accumulated sums, gathered to the pixels of a new view (backward reprojection of a
// static scene by the first hit of each pixel's camera ray, nearest neighbour).  The numeric specification is in include/rtow.h next to RtowReprojectParams
// (and DESIGN.md 5); tests/reproject_reference.py restates it in numpy and the GPU tests compare the two bit for bit.
//
// Launch shape: one lane per output pixel, a wave is an 8 x 8 pixel tile (as rtowTraceViewDevice maps them), so the 64 gathers of a wave from the
// previous frame land in a few rows of it; a workgroup is four tiles, and tiles beyond the grid limit are walked by a grid-stride loop.  No LDS, no barrier.
#include "rtow_reproject_steps.hip.h"

namespace rtow {

namespace {

// the previous pixel that pixel `i` carries, or -1 (steps 1 - 3 of the specification)
__device__ __forceinline__ int source_pixel(const ReprojectArgs& A, size_t i)
{
    float fx, fy, r;
    int e;
    if (!project_point(A, i, fx, fy, e, r)) return -1;
    const int qx = (int)fx, qy = (int)fy;
    if (qx >= A.width || qy >= A.height) return -1;        // only where (float)width > width (sizes beyond 2^24): never outside the frame
    const int q = qy * A.width + qx;
    return tap_matches(A, q, e, r) ? q : -1;
}

__global__ void __launch_bounds__(kReprojectBlock) reproject_kernel(ReprojectArgs A)
{
    const unsigned stride = gridDim.x * (kReprojectBlock / 64);       // at most 4 x kReprojectMaxBlocks: no wrap below
    for (unsigned tile = blockIdx.x * (kReprojectBlock / 64) + (threadIdx.x >> 6); tile < A.tiles; tile += stride) {
        // wave = 8 x 8 pixel tile, lane = (lane & 7, lane >> 3) inside it
        const int cx = (int)(tile % A.tilesX) * 8 + (int)(threadIdx.x & 7u);
        const int cy = (int)(tile / A.tilesX) * 8 + (int)((threadIdx.x >> 3) & 7u);
        if (cx >= A.width || cy >= A.height) continue;
        const size_t i = (size_t)cy * (size_t)A.width + (size_t)cx;
        int q = source_pixel(A, i);
        P4 c{0.0f, 0.0f, 0.0f, 0.0f};
        P3 n{0.0f, 0.0f, 0.0f}, a{0.0f, 0.0f, 0.0f};
        float w = 0.0f;
        if (q >= 0) {
            c = reinterpret_cast<const P4*>(A.prevColor)[q];
            const bool finite = __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z) && __builtin_isfinite(c.w);
            if (finite && c.w >= 1.0f) {
                n = reinterpret_cast<const P3*>(A.prevNormal)[q];
                a = reinterpret_cast<const P3*>(A.prevAlbedo)[q];
                w = A.prevScw[q];
                if (c.w > A.maxHistory) {                  // the sums of color.w samples scaled to maxHistory of them
                    const float k = A.maxHistory / c.w;
                    c = P4{c.x * k, c.y * k, c.z * k, A.maxHistory};
                    n = P3{n.x * k, n.y * k, n.z * k};
                    a = P3{a.x * k, a.y * k, a.z * k};
                    w = w * k;
                }
            } else {
                q = -1;
                c = P4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
        reinterpret_cast<P4*>(A.outColor)[i] = c;
        reinterpret_cast<P3*>(A.outNormal)[i] = n;
        reinterpret_cast<P3*>(A.outAlbedo)[i] = a;
        A.outScw[i] = w;
        if (A.outSource) A.outSource[i] = q;
    }
}

}  // namespace

hipError_t launchReproject(const RtowReprojectParams& p, const ReprojectConstants& k, const RtowRay* rays, const RtowHitBuffers& hits, const RtowHitBuffers& previousHits,
                           const RtowAccumBuffers& previous, const RtowAccumBuffers& out, int32_t* outSource, hipStream_t stream)
{
    const ReprojectArgs A = reprojectArgs(p, k, rays, hits, previousHits, previous, out, outSource);
    hipLaunchKernelGGL(reproject_kernel, dim3(reprojectBlocks(A)), dim3(kReprojectBlock), 0, stream, A);
    return hipGetLastError();
}

}  // namespace rtow
