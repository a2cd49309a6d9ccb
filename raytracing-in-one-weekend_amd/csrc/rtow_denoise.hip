// rtow_denoise.hip - rtowDenoiseDevice's kernel: one level of the edge-avoiding a-trous wavelet filter (Dammertz et al., HPG 2010), guided by the
// normal and albedo that CombineJob writes.  The numeric specification is in include/rtow.h next to RtowDenoiseParams (and DESIGN.md 5);
// tests/denoise_reference.py restates it in numpy and the GPU tests compare the two bit for bit.
#include "rtow_kernels.h"
#include "rtow_denoise_taps.hip.h"

namespace rtow {

namespace {

using namespace taps;      // P3 / ld3, demod / remod, b3, the guide weights: shared with rtow_denoise_variance.hip

struct DenoiseLevel {
    int width, height;
    int step;                   // 1 << k
    int normalSharpness;
    float invC;                 // (float)(1 << 2k) / (colorSigma * colorSigma), used when useColor
    float invA;                 // 1 / (albedoSigma * albedoSigma), used when useAlbedo
    int useColor, useAlbedo;    // sigma != 0
    int demodIn, remodOut;      // level 0 / last level with RTOW_DENOISE_DEMODULATE_ALBEDO
    TileGrid grid;              // the 64 x 4 pixel tiles
};

// One lane per output pixel; a workgroup is a 64 x 4 tile, so every tap load of a wave reads one contiguous row segment (768 bytes of float3).
// The guides are read from the inputs at every level.  The 25 taps stay a loop: unrolled, the compiler hoists the loads of several taps and the
// kernel leaves the 64-VGPR budget of 8 waves per SIMD (tests/test_denoise_isa.py).
__global__ void __launch_bounds__(256, 8) denoise_level_kernel(DenoiseLevel L, const float* __restrict__ inColor, const float* __restrict__ normal,
                                                               const float* __restrict__ albedo, float* __restrict__ outColor)
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
        P3 r = cp;
        if (finite3(cp)) {
            const P3 np = ld3(normal, p);
            const bool npZero = zero3(np);
            float ax = 0.0f, ay = 0.0f, az = 0.0f, ws = 0.0f;
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
                        continue;
                    }
                    const size_t q = (size_t)qy * (size_t)L.width + (size_t)qx;
                    P3 cq = ld3(inColor, q);
                    const P3 aq = needAlbedo ? ld3(albedo, q) : P3{0.0f, 0.0f, 0.0f};
                    if (L.demodIn) cq = demod(cq, aq);
                    if (!finite3(cq)) continue;
                    const float wc = L.useColor ? 1.0f / (1.0f + dist2(cp, cq) * L.invC) : 1.0f;
                    const float wn = normalWeight(np, npZero, ld3(normal, q), L.normalSharpness);
                    const float wa = L.useAlbedo ? 1.0f / (1.0f + dist2(ap, aq) * L.invA) : 1.0f;
                    const float w = ((hij * wc) * wn) * wa;
                    if (!(w > 0.0f)) continue;
                    ax = ax + w * cq.x; ay = ay + w * cq.y; az = az + w * cq.z;
                    ws = ws + w;
                }
            }
            r = P3{ax / ws, ay / ws, az / ws};
        }
        if (L.remodOut) r = remod(r, ap);
        reinterpret_cast<P3*>(outColor)[p] = r;
    }
}

constexpr unsigned kDenoiseMaxBlocks = 1u << 20;     // tiles beyond this (frames of more than 2^28 pixels) are walked by a grid-stride loop

}  // namespace

hipError_t launchDenoise(const RtowDenoiseParams& p, const float* inColor, const float* inNormal, const float* inAlbedo, float* scratch, float* outColor,
                         hipStream_t stream)
{
    DenoiseLevel L;
    L.width = p.width;
    L.height = p.height;
    L.normalSharpness = p.normalSharpness;
    L.useColor = p.colorSigma != 0.0f;
    L.useAlbedo = p.albedoSigma != 0.0f;
    L.invA = L.useAlbedo ? 1.0f / (p.albedoSigma * p.albedoSigma) : 0.0f;
    L.grid = tileGrid(p.width, p.height);
    const unsigned blocks = L.grid.tiles < kDenoiseMaxBlocks ? L.grid.tiles : kDenoiseMaxBlocks;
    const bool demod = (p.flags & RTOW_DENOISE_DEMODULATE_ALBEDO) != 0;
    const float sigma2 = p.colorSigma * p.colorSigma;
    const float* src = inColor;
    for (int k = 0; k < p.iterations; ++k) {
        float* dst = ((p.iterations - 1 - k) & 1) ? scratch : outColor;      // the last level lands in outColor
        L.step = 1 << k;
        L.invC = L.useColor ? (float)(1 << (2 * k)) / sigma2 : 0.0f;
        L.demodIn = demod && k == 0;
        L.remodOut = demod && k == p.iterations - 1;
        hipLaunchKernelGGL(denoise_level_kernel, dim3(blocks), dim3(256), 0, stream, L, src, inNormal, inAlbedo, dst);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        src = dst;
    }
    return hipSuccess;
}

}  // namespace rtow
