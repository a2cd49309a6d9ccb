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
// Otherwise it stages its 70 x 10 halo region into LDS once - L(q) with NaN for "invalid or outside the image", entity, distance and normal, 24 bytes per pixel as six
// planes of 700 words (16800 bytes: 9 workgroups per CU, so LDS does not cap the 8 waves per SIMD) - and the 49 taps run from there.  A wave reads 64 consecutive words of
// a plane per tap: no bank conflict, no padding.  L(q) is computed once per pixel by the operations the specification gives, so staging changes no bit.
#include "rtow_kernels.h"
#include "rtow_denoise_taps.hip.h"
#include "rtow_guide_weight.hip.h"

// A/B build for same-box timing (never shipped: csrc/Makefile, EXTRA=-DRTOW_ESTIMATE_TAPS_FROM_LDS=0): the same tap loop reading every tap from global memory
#ifndef RTOW_ESTIMATE_TAPS_FROM_LDS
#define RTOW_ESTIMATE_TAPS_FROM_LDS 1
#endif

namespace rtow {

namespace {

using namespace taps;

// float4 at a 4-byte aligned address (an accumulator colour buffer, possibly a view that starts 4 bytes into an allocation)
struct __attribute__((packed, aligned(4))) P4 { float x, y, z, w; };

constexpr unsigned kMaxBlocks = 1u << 20;       // work beyond this many blocks is walked by a grid-stride loop
constexpr int kEstimateTileW = 64, kEstimateTileH = 4;          // the workgroup's pixels
constexpr int kRadius = 3;                      // 7 x 7 taps
constexpr int kHaloW = kEstimateTileW + 2 * kRadius, kHaloH = kEstimateTileH + 2 * kRadius, kHalo = kHaloW * kHaloH;      // 70 x 10

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
    unsigned tilesX, tiles;             // 64 x 4 pixel tiles per row / in all
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

// L(q) of the specification, NaN when invalid (a valid L is finite, so NaN is free to mean "no luminance")
__device__ __forceinline__ float luminance_or_nan(const float* color, size_t q)
{
    const P4 c = reinterpret_cast<const P4*>(color)[q];
    if (!(c.w > 0.0f)) return __builtin_nanf("");          // no successful sample (NaN included)
    const float l = lum(c.x / c.w, c.y / c.w, c.z / c.w);
    return __builtin_isfinite(l) ? l : __builtin_nanf("");
}

// the guides of a tap for guide::weight: from the staged planes, or (A/B build) from global memory
struct TileGuides {
    const int* E;
    const float *T, *Nx, *Ny, *Nz;
    int k;
    __device__ __forceinline__ int entity() const { return E[k]; }
    __device__ __forceinline__ float distance() const { return T[k]; }
    __device__ __forceinline__ void normal(float& x, float& y, float& z) const { x = Nx[k]; y = Ny[k]; z = Nz[k]; }
};
struct GlobalGuides {
    const EstimateArgs& A;
    size_t q;
    __device__ __forceinline__ int entity() const { return A.entity[q]; }
    __device__ __forceinline__ float distance() const { return A.distance[q]; }
    __device__ __forceinline__ void normal(float& x, float& y, float& z) const { const P3 n = ld3(A.normal, q); x = n.x; y = n.y; z = n.z; }
};

__global__ void __launch_bounds__(256, 8) estimate_moments_kernel(EstimateArgs A)
{
#if RTOW_ESTIMATE_TAPS_FROM_LDS
    __shared__ float sL[kHalo], sT[kHalo], sNx[kHalo], sNy[kHalo], sNz[kHalo];
    __shared__ int sE[kHalo];
#endif
    const int lx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);
    for (unsigned t = blockIdx.x; t < A.tiles; t += gridDim.x) {          // the same tiles for every lane of the workgroup: the barriers below are uniform
        const int x0 = (int)(t % A.tilesX) * kEstimateTileW, y0 = (int)(t / A.tilesX) * kEstimateTileH;
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
#if RTOW_ESTIMATE_TAPS_FROM_LDS
        for (int k = (int)threadIdx.x; k < kHalo; k += 256) {
            const int qx = x0 - kRadius + k % kHaloW, qy = y0 - kRadius + k / kHaloW;
            float l = __builtin_nanf("");                                 // outside the image: skipped like an invalid L
            if (qx >= 0 && qx < A.width && qy >= 0 && qy < A.height) {
                const size_t q = (size_t)qy * (size_t)A.width + (size_t)qx;
                l = luminance_or_nan(A.color, q);
                sE[k] = A.entity[q];
                sT[k] = A.distance[q];
                const P3 n = ld3(A.normal, q);
                sNx[k] = n.x; sNy[k] = n.y; sNz[k] = n.z;
            }
            sL[k] = l;
        }
        __syncthreads();
        const int centre = (ly + kRadius) * kHaloW + lx + kRadius;
#endif
        bool filled = false;
        if (wanted) {
#if RTOW_ESTIMATE_TAPS_FROM_LDS
            const float lp = sL[centre];
#else
            const float lp = luminance_or_nan(A.color, p);
#endif
            if (lp == lp) {
                const int e = A.entity[p];
                const float tp = A.distance[p];
                const P3 np = ld3(A.normal, p);
                float W = 0.0f, S1 = 0.0f, S2 = 0.0f;
                int taps = 0;
#pragma unroll 1
                for (int j = -kRadius; j <= kRadius; ++j) {
#pragma unroll 1
                    for (int i = -kRadius; i <= kRadius; ++i) {
#if RTOW_ESTIMATE_TAPS_FROM_LDS
                        const int k = centre + j * kHaloW + i;
                        const float l = sL[k];
                        if (l != l) continue;                             // outside the image, or L(q) invalid
                        const float w = (i == 0 && j == 0) ? 1.0f         // the centre consults no guide
                                                           : guide::weight(e, tp, np.x, np.y, np.z, A.matchEntity, A.depthTolerance, A.normalSharpness,
                                                                           TileGuides{sE, sT, sNx, sNy, sNz, k});
#else
                        if (j < -y || j > A.height - 1 - y || i < -x || i > A.width - 1 - x) continue;
                        const size_t q = (size_t)(y + j) * (size_t)A.width + (size_t)(x + i);
                        const float l = (i == 0 && j == 0) ? lp : luminance_or_nan(A.color, q);
                        if (l != l) continue;
                        const float w = (i == 0 && j == 0) ? 1.0f
                                                           : guide::weight(e, tp, np.x, np.y, np.z, A.matchEntity, A.depthTolerance, A.normalSharpness,
                                                                           GlobalGuides{A, q});
#endif
                        if (!(w > 0.0f)) continue;                        // NaN included
                        W = W + w;
                        S1 = S1 + w * l;
                        S2 = S2 + w * (l * l);
                        ++taps;
                    }
                }
                if (taps >= A.minTaps) {
                    const float a = S1 / W, b = S2 / W;
                    if (__builtin_isfinite(a) && __builtin_isfinite(b)) {
                        m = P3{a + a, b + b, 2.0f};                       // the neighbourhood's weighted moments as two batches
                        filled = true;
                    }
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
    A.tilesX = ((unsigned)p.width + kEstimateTileW - 1) / kEstimateTileW;
    A.tiles = (unsigned)((uint64_t)A.tilesX * (((uint64_t)p.height + kEstimateTileH - 1) / kEstimateTileH));      // (w / 64 + 1) (h / 4 + 1) < 2^30 for w h < 2^31
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
    hipLaunchKernelGGL(estimate_moments_kernel, dim3(A.tiles < kMaxBlocks ? A.tiles : kMaxBlocks), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace rtow
