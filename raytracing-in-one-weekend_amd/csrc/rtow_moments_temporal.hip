// rtow_moments_temporal.hip - the temporal half of the variance-guided denoiser: what keeps the luminance moments of rtowAccumulateMomentsDevice alive across a
// camera move.  rtowReprojectMomentsDevice gathers the previous view's moments through the source map rtowReprojectAccumDevice writes, with a history cap of its own.
// rtowEstimateMomentsDevice is SVGF's spatial fallback (Schied et al., HPG 2017, section 4.2): a pixel with too short a history - a reprojection hole, any pixel of a
// single-batch or chained frame - takes its moments from the 7 x 7 neighbourhood of the current frame, weighted by the first-hit guides, in the moments format
// rtowDenoiseVarianceDevice reads.  The numeric specification is in include/rtow.h next to the two entry points (and DESIGN.md 5);
// tests/temporal_moments_reference.py restates it in numpy and the GPU tests compare the two bit for bit.
//
// Launch shape.  The gather knows only pixelCount: one lane per pixel, 256-lane grid-stride; the scattered 12-byte read is what occupancy hides.  The
// estimate uses the 64 x 4 pixel workgroup tile of the denoise levels (a wave is 64 pixels of one row).  A workgroup first asks whether any of its pixels is to be
// estimated: after a small camera move almost none is, and the tile then copies its moments (nothing at all in place) without touching the colour or the guides.
// Otherwise it stages its whole 70 x 10 halo region into LDS once and the 49 taps run from there: the staging and the tap loop of rtow_guided_halo.hip.h, which
// rtow_rectify_history.hip shares.
#include "rtow_kernels.h"
#include "rtow_guided_halo.hip.h"

namespace rtow {

namespace {

using namespace taps;

constexpr unsigned kMaxBlocks = 1u << 20;       // work beyond this many blocks is walked by a grid-stride loop

// One lane per pixel.  A source outside [0, pixels) is never used as an address.
__global__ void __launch_bounds__(256) reproject_moments_kernel(unsigned pixels, float maxBatches, const int32_t* __restrict__ source,
                                                                const float* __restrict__ previousMoments, float* __restrict__ outMoments)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < pixels; i += (size_t)gridDim.x * 256u) {
        const int32_t q = source[i];
        P3 m{0.0f, 0.0f, 0.0f};
        if (q >= 0 && (unsigned)q < pixels) {
            const P3 v = ld3(previousMoments, (size_t)q);
            if (finite3(v) && v.z >= 1.0f) {
                m = v;
                if (v.z > maxBatches) {                    // the sums of n batches scaled to maxBatches of them: the mean stays
                    const float k = maxBatches / v.z;
                    m = P3{v.x * k, v.y * k, maxBatches};
                }
            }
        }
        reinterpret_cast<P3*>(outMoments)[i] = m;
    }
}

struct EstimateArgs {
    int width, height;
    TileGrid grid;                      // the 64 x 4 pixel tiles
    float minBatches;                   // (float)minBatches
    int minTaps, normalSharpness, matchEntity;
    float depthTolerance;
    const float* color;
    const float* distance;
    const int32_t* entity;
    const float* normal;
    const float* inMoments;
    float* outMoments;
    uint8_t* outFilled;
};

__global__ void __launch_bounds__(256, 8) estimate_moments_kernel(EstimateArgs A)
{
    __shared__ float sL[halo::kHalo], sT[halo::kHalo], sNx[halo::kHalo], sNy[halo::kHalo], sNz[halo::kHalo];
    __shared__ int sE[halo::kHalo];
    const halo::Planes planes{sL, sE, sT, sNx, sNy, sNz};
    const int lx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);
    for (unsigned t = blockIdx.x; t < A.grid.tiles; t += gridDim.x) {          // the same tiles for every lane of the workgroup: the barriers below are uniform
        const int x0 = (int)(t % A.grid.tilesX) * kGroupW, y0 = (int)(t / A.grid.tilesX) * kGroupH;
        const int x = x0 + lx, y = y0 + ly;
        const bool inside = x < A.width && y < A.height;
        const size_t p = (size_t)y * (size_t)A.width + (size_t)x;
        P3 m{0.0f, 0.0f, 0.0f};
        if (inside && A.inMoments) m = ld3(A.inMoments, p);
        const bool wanted = inside && !(m.z >= A.minBatches);             // a NaN n is estimated
        // a barrier as well: every lane is through with the planes of the previous tile before they are staged again
        if (!__syncthreads_or(wanted ? 1 : 0)) {                          // the common tile after a small camera move: no colour, no guide is read
            if (inside) {
                if (A.inMoments != A.outMoments) reinterpret_cast<P3*>(A.outMoments)[p] = m;
                if (A.outFilled) A.outFilled[p] = 0;
            }
            continue;
        }
        halo::stage(planes, x0, y0, A.width, A.height, halo::kMaxRadius, A.color, A.entity, A.distance, A.normal);
        __syncthreads();
        const int centre = halo::centre_of(lx, ly);
        bool filled = false;
        if (wanted && sL[centre] == sL[centre]) {                         // a pixel without a valid L of its own keeps its moments
            const halo::Sums s = halo::neighbourhood(planes, centre, halo::kMaxRadius, A.matchEntity, A.depthTolerance, A.normalSharpness);
            if (s.taps >= A.minTaps) {
                const float a = s.S1 / s.W, b = s.S2 / s.W;
                if (__builtin_isfinite(a) && __builtin_isfinite(b)) {
                    m = P3{a + a, b + b, 2.0f};                           // the neighbourhood's weighted moments as two batches
                    filled = true;
                }
            }
        }
        if (inside) {
            if (filled || A.inMoments != A.outMoments) reinterpret_cast<P3*>(A.outMoments)[p] = m;
            if (A.outFilled) A.outFilled[p] = filled ? 1 : 0;
        }
    }
}

}  // namespace

hipError_t launchReprojectMoments(int pixelCount, const int32_t* source, const float* previousMoments, int maxBatches, float* outMoments, hipStream_t stream)
{
    const size_t blocks = ((size_t)pixelCount + 255u) / 256u;
    hipLaunchKernelGGL(reproject_moments_kernel, dim3(blocks < kMaxBlocks ? (unsigned)blocks : kMaxBlocks), dim3(256), 0, stream, (unsigned)pixelCount, (float)maxBatches,
                       source, previousMoments, outMoments);
    return hipGetLastError();
}

hipError_t launchEstimateMoments(const RtowEstimateMomentsParams& p, const float* color, const RtowHitBuffers& hits, const float* inMoments, float* outMoments,
                                 uint8_t* outFilled, hipStream_t stream)
{
    EstimateArgs A{};
    A.width = p.width;
    A.height = p.height;
    A.grid = tileGrid(p.width, p.height);
    A.minBatches = (float)p.minBatches;
    A.minTaps = p.minTaps;
    A.normalSharpness = p.normalSharpness;
    A.matchEntity = (p.flags & RTOW_ESTIMATE_MOMENTS_MATCH_ENTITY) != 0;
    A.depthTolerance = p.depthTolerance;
    A.color = color;
    A.distance = hits.distance;
    A.entity = hits.entityIndex;
    A.normal = hits.normal;
    A.inMoments = inMoments;
    A.outMoments = outMoments;
    A.outFilled = outFilled;
    hipLaunchKernelGGL(estimate_moments_kernel, dim3(A.grid.tiles < kMaxBlocks ? A.grid.tiles : kMaxBlocks), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace rtow
