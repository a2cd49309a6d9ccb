// rtow_upsample.hip - rtowUpsampleDevice's kernels: a frame rendered at srcW x srcH (the host's resolutionScaling) brought to the displayed dstW x dstH - the point and
// bilinear reads of the reference's raster blit (UNITY/Raytracer.cs:1123), and a joint bilateral upsampling (Kopf et al., SIGGRAPH 2007) guided by the first hits of
// rtowTraceViewDevice at both sizes, optionally on the colour with the albedo divided out.  The numeric specification is in include/rtow.h next to RtowUpsampleParams
// (and DESIGN.md 5); tests/upsample_reference.py restates it in numpy and the GPU tests compare the two bit for bit.
//
// Launch shape: one lane per dst pixel, a wave is an 8 x 8 dst tile (as rtowTraceViewDevice maps them), so the taps of a wave land in a few src rows; a
// workgroup is four tiles, and tiles beyond the grid limit are walked by a grid-stride loop.  No LDS, no barrier.  The mode and the demodulation are template
// parameters: the POINT and BILINEAR kernels carry no guide loads, and only the DEMODULATE kernels the albedo loads and divisions.
#include "rtow_kernels.h"

#include "rtow_guide_weight.hip.h"
#include "rtow_vecmath.hip.h"

namespace rtow {

namespace {

__device__ __forceinline__ P3 ld3(const float* p, size_t index) { return reinterpret_cast<const P3*>(p)[index]; }

constexpr int kUpsampleBlock = 256;                      // four 8 x 8 tiles
constexpr unsigned kUpsampleMaxBlocks = 4096;            // two rounds of the 2048 workgroups an MI355X holds at 8 waves per SIMD; tile groups beyond this (dst frames from
                                                         // about 1024 x 1024) are walked by the grid-stride loop
constexpr float kDemodMin = 0.0009765625f;               // 2^-10

struct UpsampleArgs {
    int srcW, srcH, dstW, dstH;
    unsigned tilesX, tiles;             // 8 x 8 dst pixel tiles per row / in all
    int normalSharpness, matchEntity;
    float depthTolerance;
    const float* srcColor;
    const float* srcDistance;
    const int32_t* srcEntity;
    const float* srcNormal;
    const float* srcAlbedo;
    const float* dstDistance;
    const int32_t* dstEntity;
    const float* dstNormal;
    const float* dstAlbedo;
    float* outColor;
    uint8_t* outStage;
};

__device__ __forceinline__ bool finite3(P3 c) { return __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One axis of the position, in integers.  N = (2 X + 1) src - dst lies in (-dst, 2 src dst) and 2 src dst <= 2^29 for sizes up to 16384, so int32 holds it and the one
// unsigned division is exact; N < 0 is the only case with a negative quotient, and its floor is -1.  base = floor(N / (2 dst)), rem = N - base * 2 dst in [0, 2 dst);
// the point pixel floor((N + dst) / (2 dst)) is base + (rem >= dst): no second division.
__device__ __forceinline__ void axis_position(int X, int src, int dst, int& base, int& rem)
{
    const int N = (2 * X + 1) * src - dst;
    const unsigned two = 2u * (unsigned)dst;
    base = N < 0 ? -1 : (int)((unsigned)N / two);
    rem = N - base * (int)two;
}

// the src pixel q's guides, loaded as the guide weight asks for them
struct SrcGuides {
    const UpsampleArgs& A;
    size_t q;
    __device__ __forceinline__ int entity() const { return A.srcEntity[q]; }
    __device__ __forceinline__ float distance() const { return A.srcDistance[q]; }
    __device__ __forceinline__ void normal(float& x, float& y, float& z) const { const P3 n = ld3(A.srcNormal, q); x = n.x; y = n.y; z = n.z; }
};

// the guide weight g(p, q) of the specification (rtow_guide_weight.hip.h); e, t, n are the dst pixel's
__device__ __forceinline__ float guide_weight(const UpsampleArgs& A, int e, float t, P3 n, size_t q)
{
    return guide::weight(e, t, n.x, n.y, n.z, A.matchEntity, A.depthTolerance, A.normalSharpness, SrcGuides{A, q});
}

struct Sum { float x, y, z, w; };

// one tap: the src pixel (qx, qy) clamped into the image, with the weight `base` (stage A: bx * by) times the guide weight, or the guide weight alone (stage B)
template <int MODE, bool DEMOD, bool STAGE_B>
__device__ __forceinline__ void tap(const UpsampleArgs& A, Sum& s, int qx, int qy, float base, int e, float t, P3 n)
{
    const size_t q = (size_t)clampi(qy, A.srcH - 1) * (size_t)A.srcW + (size_t)clampi(qx, A.srcW - 1);
    float w = base;
    if (MODE == RTOW_UPSAMPLE_GUIDED) {
        const float g = guide_weight(A, e, t, n, q);
        w = STAGE_B ? g : base * g;
    }
    if (!(w > 0.0f)) return;                                  // NaN included
    P3 c = ld3(A.srcColor, q);
    if (DEMOD) {
        const P3 a = ld3(A.srcAlbedo, q);
        c = P3{a.x >= kDemodMin ? c.x / a.x : c.x, a.y >= kDemodMin ? c.y / a.y : c.y, a.z >= kDemodMin ? c.z / a.z : c.z};
    }
    if (!finite3(c)) return;
    s.x = s.x + w * c.x; s.y = s.y + w * c.y; s.z = s.z + w * c.z;
    s.w = s.w + w;
}

template <int MODE, bool DEMOD>
__global__ void __launch_bounds__(kUpsampleBlock) upsample_kernel(UpsampleArgs A)
{
    const unsigned stride = gridDim.x * (kUpsampleBlock / 64);       // at most 4 x kUpsampleMaxBlocks: no wrap below (tiles <= 2^22)
    for (unsigned tile = blockIdx.x * (kUpsampleBlock / 64) + (threadIdx.x >> 6); tile < A.tiles; tile += stride) {
        // wave = 8 x 8 dst pixel tile, lane = (lane & 7, lane >> 3) inside it
        const int cx = (int)(tile % A.tilesX) * 8 + (int)(threadIdx.x & 7u);
        const int cy = (int)(tile / A.tilesX) * 8 + (int)((threadIdx.x >> 3) & 7u);
        if (cx >= A.dstW || cy >= A.dstH) continue;
        const size_t p = (size_t)cy * (size_t)A.dstW + (size_t)cx;
        int x0, rx, y0, ry;
        axis_position(cx, A.srcW, A.dstW, x0, rx);
        axis_position(cy, A.srcH, A.dstH, y0, ry);
        const size_t point = (size_t)(y0 + (ry >= A.dstH ? 1 : 0)) * (size_t)A.srcW + (size_t)(x0 + (rx >= A.dstW ? 1 : 0));
        int stage = 2;
        P3 r{0.0f, 0.0f, 0.0f};
        if (MODE != RTOW_UPSAMPLE_POINT) {
            const float fx = (float)rx / (float)(2 * A.dstW), fy = (float)ry / (float)(2 * A.dstH);
            const float bx0 = 1.0f - fx, by0 = 1.0f - fy;
            int e = 0;
            float t = 0.0f;
            P3 n{0.0f, 0.0f, 0.0f};
            if (MODE == RTOW_UPSAMPLE_GUIDED) {
                e = A.dstEntity[p];
                t = A.dstDistance[p];
                n = ld3(A.dstNormal, p);
            }
            Sum s{0.0f, 0.0f, 0.0f, 0.0f};
            tap<MODE, DEMOD, false>(A, s, x0, y0, bx0 * by0, e, t, n);
            tap<MODE, DEMOD, false>(A, s, x0 + 1, y0, fx * by0, e, t, n);
            tap<MODE, DEMOD, false>(A, s, x0, y0 + 1, bx0 * fy, e, t, n);
            tap<MODE, DEMOD, false>(A, s, x0 + 1, y0 + 1, fx * fy, e, t, n);
            if (s.w > 0.0f) stage = 0;
            else if (MODE == RTOW_UPSAMPLE_GUIDED) {
                // the twelve outer taps of the 4 x 4 block; a loop, so that the rare stage costs the common one no registers
#pragma unroll 1
                for (int j = -1; j <= 2; ++j) {
#pragma unroll 1
                    for (int i = -1; i <= 2; ++i) {
                        if ((i == 0 || i == 1) && (j == 0 || j == 1)) continue;
                        tap<MODE, DEMOD, true>(A, s, x0 + i, y0 + j, 1.0f, e, t, n);
                    }
                }
                if (s.w > 0.0f) stage = 1;
            }
            if (stage != 2) {
                r = P3{s.x / s.w, s.y / s.w, s.z / s.w};
                if (DEMOD) {
                    const P3 a = ld3(A.dstAlbedo, p);
                    r = P3{a.x >= kDemodMin ? r.x * a.x : r.x, a.y >= kDemodMin ? r.y * a.y : r.y, a.z >= kDemodMin ? r.z * a.z : r.z};
                }
            }
        }
        if (stage == 2) r = ld3(A.srcColor, point);           // bit for bit: loads and stores of three dwords, no arithmetic
        reinterpret_cast<P3*>(A.outColor)[p] = r;
        if (A.outStage) A.outStage[p] = (uint8_t)stage;
    }
}

}  // namespace

hipError_t launchUpsample(const RtowUpsampleParams& p, const float* srcColor, const RtowHitBuffers& srcHits, const float* srcAlbedo, const RtowHitBuffers& dstHits,
                          const float* dstAlbedo, float* outColor, uint8_t* outStage, hipStream_t stream)
{
    UpsampleArgs A{};
    A.srcW = p.srcWidth; A.srcH = p.srcHeight; A.dstW = p.dstWidth; A.dstH = p.dstHeight;
    A.tilesX = ((unsigned)p.dstWidth + 7u) / 8u;
    A.tiles = A.tilesX * (((unsigned)p.dstHeight + 7u) / 8u);          // at most 2048 x 2048
    A.normalSharpness = p.normalSharpness;
    A.matchEntity = (p.flags & RTOW_UPSAMPLE_MATCH_ENTITY) != 0;
    A.depthTolerance = p.depthTolerance;
    A.srcColor = srcColor;
    const bool guided = p.mode == RTOW_UPSAMPLE_GUIDED, demod = (p.flags & RTOW_UPSAMPLE_DEMODULATE_ALBEDO) != 0;
    if (guided) {
        A.srcDistance = srcHits.distance; A.srcEntity = srcHits.entityIndex; A.srcNormal = srcHits.normal;
        A.dstDistance = dstHits.distance; A.dstEntity = dstHits.entityIndex; A.dstNormal = dstHits.normal;
    }
    if (demod) { A.srcAlbedo = srcAlbedo; A.dstAlbedo = dstAlbedo; }
    A.outColor = outColor;
    A.outStage = outStage;
    const unsigned groups = (A.tiles + kUpsampleBlock / 64 - 1) / (kUpsampleBlock / 64);
    const dim3 grid(groups < kUpsampleMaxBlocks ? groups : kUpsampleMaxBlocks), block(kUpsampleBlock);
    if (p.mode == RTOW_UPSAMPLE_POINT) hipLaunchKernelGGL((upsample_kernel<RTOW_UPSAMPLE_POINT, false>), grid, block, 0, stream, A);
    else if (p.mode == RTOW_UPSAMPLE_BILINEAR && !demod) hipLaunchKernelGGL((upsample_kernel<RTOW_UPSAMPLE_BILINEAR, false>), grid, block, 0, stream, A);
    else if (p.mode == RTOW_UPSAMPLE_BILINEAR) hipLaunchKernelGGL((upsample_kernel<RTOW_UPSAMPLE_BILINEAR, true>), grid, block, 0, stream, A);
    else if (!demod) hipLaunchKernelGGL((upsample_kernel<RTOW_UPSAMPLE_GUIDED, false>), grid, block, 0, stream, A);
    else hipLaunchKernelGGL((upsample_kernel<RTOW_UPSAMPLE_GUIDED, true>), grid, block, 0, stream, A);
    return hipGetLastError();
}

}  // namespace rtow
