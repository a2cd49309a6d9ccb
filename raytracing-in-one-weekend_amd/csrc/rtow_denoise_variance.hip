// rtow_denoise_variance.hip - the variance-guided denoise passes.  rtowAccumulateMomentsDevice: per-pixel luminance moments (sum, sum of squares, count) over
// the per-batch colours of a batch group.  rtowDenoiseVarianceDevice: the a-trous filter of rtow_denoise.hip with the colour term of SVGF's spatial part
// (Schied et al., HPG 2017, sections 4.2 - 4.4): the colour weight is scaled by the 3 x 3 filtered variance of the pixel, and the variance is carried through the
// levels with the squared weights.  The numeric specification is in include/rtow.h next to the two entry points (and DESIGN.md 5);
// tests/denoise_variance_reference.py restates it in numpy and the GPU tests compare the two bit for bit.
#include "rtow_kernels.h"
#include "rtow_denoise_taps.hip.h"
#include "rtow_moments_variance.hip.h"

namespace rtow {

namespace {

using namespace taps;

constexpr unsigned kMaxBlocks = 1u << 20;       // work beyond this many blocks is walked by a grid-stride loop
constexpr float kVarianceUnknown = -1.0f;       // a pixel without a variance estimate (fewer than 2 batches, a non-finite estimate)
constexpr float kInvCEpsilon = 9.5367431640625e-07f;      // 2^-20

struct MomentsArgs {
    const float* colors[kMomentsMaxBatches];    // device float4[pixelCount] each: the pointers travel in the kernel arguments
    int count;
    unsigned pixels;
};

// One lane per pixel: a pixel's batches in order, so in place (inMoments == outMoments) is safe - a lane reads its own element before it writes it.
__global__ void __launch_bounds__(256) accumulate_moments_kernel(MomentsArgs A, const float* inMoments, float* outMoments)
{
    for (size_t p = (size_t)blockIdx.x * 256u + threadIdx.x; p < A.pixels; p += (size_t)gridDim.x * 256u) {
        P3 m = inMoments ? ld3(inMoments, p) : P3{0.0f, 0.0f, 0.0f};      // (s1, s2, n)
        for (int k = 0; k < A.count; ++k) {
            const float l = luminance_or_nan(A.colors[k], p);
            if (l != l) continue;                                          // no successful sample in this batch, or a luminance that is not finite
            m.x = m.x + l;
            m.y = m.y + l * l;
            m.z = m.z + 1.0f;
        }
        reinterpret_cast<P3*>(outMoments)[p] = m;
    }
}

// v0: the variance of the mean of the batches' luminances, in the scale the levels filter in (demodulated with the flag)
__global__ void __launch_bounds__(256) initial_variance_kernel(unsigned pixels, int demodulate, const float* __restrict__ moments, const float* __restrict__ albedo,
                                                               float* __restrict__ variance)
{
    for (size_t p = (size_t)blockIdx.x * 256u + threadIdx.x; p < pixels; p += (size_t)gridDim.x * 256u) {
        const P3 m = ld3(moments, p);
        float v = kVarianceUnknown, mean, e;
        if (mean_variance(m, mean, e)) {
            if (__builtin_isfinite(e)) {
                v = e;
                if (demodulate) {
                    const P3 a = ld3(albedo, p);
                    const float la = lum(a.x, a.y, a.z);
                    if (la >= kDemodMin) v = v / (la * la);
                }
            }
        }
        variance[p] = v;
    }
}

struct VarianceLevel {
    int width, height;
    int step;                   // 1 << k
    int normalSharpness;
    float sigma2;               // colorSigma * colorSigma, used when useColor
    float invA;                 // 1 / (albedoSigma * albedoSigma), used when useAlbedo
    int useColor, useAlbedo;    // sigma != 0
    int demodIn, remodOut;      // level 0 / last level with RTOW_DENOISE_DEMODULATE_ALBEDO
    TileGrid grid;              // the 64 x 4 pixel tiles
};

// One level: rtow_denoise.hip's kernel (same tiling, same tap loop and skip rules, from rtow_denoise_taps.hip.h) with the variance state added - per pixel the own variance,
// the reciprocal of the colour term's denominator, the own luminance and the variance sum, per tap one more 4-byte load.  The 3 x 3 variance filter runs before the
// tap loop, so its nine values are dead when the loop starts; the kernel stays within the 64 VGPRs of 8 waves per SIMD (tests/test_denoise_variance_isa.py).
__global__ void __launch_bounds__(256, 8) denoise_variance_level_kernel(VarianceLevel L, const float* __restrict__ inColor, const float* __restrict__ normal,
                                                                        const float* __restrict__ albedo, const float* __restrict__ inVariance,
                                                                        float* __restrict__ outColor, float* __restrict__ outVariance)
{
    for (unsigned t = blockIdx.x; t < L.grid.tiles; t += gridDim.x) {
        const int x = (int)(t % L.grid.tilesX) * kGroupW + (int)(threadIdx.x & 63u);      // a wave is the 64 pixels of one tile row
        const int y = (int)(t / L.grid.tilesX) * kGroupH + (int)(threadIdx.x >> 6);
        if (x >= L.width || y >= L.height) continue;
        const size_t p = (size_t)y * (size_t)L.width + (size_t)x;
        const bool needAlbedo = L.demodIn || L.useAlbedo;
        const P3 ap = (needAlbedo || L.remodOut) ? ld3(albedo, p) : P3{0.0f, 0.0f, 0.0f};
        P3 cp = ld3(inColor, p);
        if (L.demodIn) cp = demod(cp, ap);
        const float vp = inVariance[p];
        const bool known = vp >= 0.0f;                                    // -1 (and NaN): no estimate
        P3 r = cp;
        float vout = known ? vp : kVarianceUnknown;                       // a pixel that passes through keeps its variance
        if (finite3(cp)) {
            const bool useColor = L.useColor && known;
            float invC = 0.0f;
            if (useColor) {                                               // g_p: the 3 x 3 filtered variance at unit spacing over the known in-image neighbours
                float num = 0.0f, den = 0.0f;
#pragma unroll 1
                for (int j = -1; j <= 1; ++j) {
                    if (j < -y || j > L.height - 1 - y) continue;
#pragma unroll 1
                    for (int i = -1; i <= 1; ++i) {
                        if (i < -x || i > L.width - 1 - x) continue;
                        const float vq = inVariance[(size_t)(y + j) * (size_t)L.width + (size_t)(x + i)];
                        if (!(vq >= 0.0f)) continue;
                        const float g = (i == 0 ? 0.5f : 0.25f) * (j == 0 ? 0.5f : 0.25f);
                        num = num + g * vq;
                        den = den + g;
                    }
                }
                invC = 1.0f / (L.sigma2 * (num / den) + kInvCEpsilon);
            }
            const float lp = lum(cp.x, cp.y, cp.z);
            const P3 np = ld3(normal, p);
            const bool npZero = zero3(np);
            float ax = 0.0f, ay = 0.0f, az = 0.0f, ws = 0.0f, vacc = 0.0f;
#pragma unroll 1
            for (int j = -2; j <= 2; ++j) {
                const int dy = j * L.step;
                if (dy < -y || dy > L.height - 1 - y) continue;           // outside the image: skipped (no overflow near INT32_MAX)
                const int qy = y + dy;
                const float hj = b3(j);
#pragma unroll 1
                for (int i = -2; i <= 2; ++i) {
                    const int dx = i * L.step;
                    if (dx < -x || dx > L.width - 1 - x) continue;
                    const int qx = x + dx;
                    const float hij = b3(i) * hj;
                    if (i == 0 && j == 0) {                              // the centre: 9/64, no guide consulted
                        ax = ax + hij * cp.x; ay = ay + hij * cp.y; az = az + hij * cp.z;
                        ws = ws + hij;
                        if (known) vacc = vacc + (hij * hij) * vp;
                        continue;
                    }
                    const size_t q = (size_t)qy * (size_t)L.width + (size_t)qx;
                    P3 cq = ld3(inColor, q);
                    const P3 aq = needAlbedo ? ld3(albedo, q) : P3{0.0f, 0.0f, 0.0f};
                    if (L.demodIn) cq = demod(cq, aq);
                    if (!finite3(cq)) continue;
                    float wc = 1.0f;
                    if (useColor) {
                        const float dl = lp - lum(cq.x, cq.y, cq.z);
                        wc = 1.0f / (1.0f + (dl * dl) * invC);
                    }
                    const float wn = normalWeight(np, npZero, ld3(normal, q), L.normalSharpness);
                    const float wa = L.useAlbedo ? 1.0f / (1.0f + dist2(ap, aq) * L.invA) : 1.0f;
                    const float w = ((hij * wc) * wn) * wa;
                    if (!(w > 0.0f)) continue;
                    ax = ax + w * cq.x; ay = ay + w * cq.y; az = az + w * cq.z;
                    ws = ws + w;
                    if (known) {
                        const float vq = inVariance[q];
                        if (vq >= 0.0f) vacc = vacc + (w * w) * vq;      // a tap without an estimate adds to the colour only
                    }
                }
            }
            r = P3{ax / ws, ay / ws, az / ws};
            if (known) {
                vout = vacc / (ws * ws);
                if (!(vout >= 0.0f)) vout = kVarianceUnknown;             // 0 * inf: no NaN is ever stored
            }
        }
        if (L.remodOut) r = remod(r, ap);
        reinterpret_cast<P3*>(outColor)[p] = r;
        outVariance[p] = vout;
    }
}

unsigned blocksFor(size_t pixels)
{
    const size_t blocks = (pixels + 255u) / 256u;
    return blocks < kMaxBlocks ? (unsigned)blocks : kMaxBlocks;
}

}  // namespace

hipError_t launchAccumulateMoments(int pixelCount, int count, const float* const* colors, const float* inMoments, float* outMoments, hipStream_t stream)
{
    MomentsArgs A;
    for (int k = 0; k < kMomentsMaxBatches; ++k) A.colors[k] = k < count ? colors[k] : nullptr;
    A.count = count;
    A.pixels = (unsigned)pixelCount;
    hipLaunchKernelGGL(accumulate_moments_kernel, dim3(blocksFor((size_t)pixelCount)), dim3(256), 0, stream, A, inMoments, outMoments);
    return hipGetLastError();
}

hipError_t launchDenoiseVariance(const RtowDenoiseParams& p, const float* inColor, const float* inNormal, const float* inAlbedo, const float* moments, float* scratch,
                                 float* outColor, float* outVariance, hipStream_t stream)
{
    const size_t pixels = (size_t)p.width * (size_t)p.height;
    // the scratch: the colour ping-pong plane (float3), then two variance planes (float)
    float* const colorPlane = scratch;
    float* const varPlane[2] = {scratch + pixels * 3, scratch + pixels * 4};
    const bool demod = (p.flags & RTOW_DENOISE_DEMODULATE_ALBEDO) != 0;
    hipLaunchKernelGGL(initial_variance_kernel, dim3(blocksFor(pixels)), dim3(256), 0, stream, (unsigned)pixels, demod ? 1 : 0, moments, inAlbedo, varPlane[0]);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    VarianceLevel L;
    L.width = p.width;
    L.height = p.height;
    L.normalSharpness = p.normalSharpness;
    L.useColor = p.colorSigma != 0.0f;
    L.useAlbedo = p.albedoSigma != 0.0f;
    L.sigma2 = p.colorSigma * p.colorSigma;
    L.invA = L.useAlbedo ? 1.0f / (p.albedoSigma * p.albedoSigma) : 0.0f;
    L.grid = tileGrid(p.width, p.height);
    const unsigned blocks = L.grid.tiles < kMaxBlocks ? L.grid.tiles : kMaxBlocks;
    const float* src = inColor;
    for (int k = 0; k < p.iterations; ++k) {
        const bool last = k == p.iterations - 1;
        float* dst = ((p.iterations - 1 - k) & 1) ? colorPlane : outColor;      // the last level lands in outColor
        float* vdst = (last && outVariance) ? outVariance : varPlane[(k + 1) & 1];
        L.step = 1 << k;
        L.demodIn = demod && k == 0;
        L.remodOut = demod && last;
        hipLaunchKernelGGL(denoise_variance_level_kernel, dim3(blocks), dim3(256), 0, stream, L, src, inNormal, inAlbedo, (const float*)varPlane[k & 1], dst, vdst);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        src = dst;
    }
    return hipSuccess;
}

}  // namespace rtow
