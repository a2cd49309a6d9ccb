// rtow_bloom.hip - rtowBloomDevice: HDR bloom on the scene-referred colour in front of the meter and the tone-mapped finalize - a bright pass, a pyramid of mips, the
// pyramid summed upwards, the sum added to the frame.  The numeric specification is in include/rtow.h next to the entry point (and DESIGN.md 5);
// tests/bloom_reference.py restates it in numpy and the GPU tests compare the two bit for bit.
//
// Launch shape: 2 * levels plain launches in stream order, no global atomics, no clear - every texel a launch reads was stored by a launch before it.
//   bloom_prefilter_kernel<KARIS>: a 64 x 4 tile of mip 1 per workgroup of 256 lanes.  The tile's 130 x 10 source pixels (each coordinate clamped into the image, so the
//     tap loop has no edge case) are read from the unaligned float3 stream, bright-passed ONCE and staged in LDS as planes of 1300 words: r, g, b of the bright-passed
//     colour and, with the Karis flag, the weight wk - 4 x 1300 x 4 = 20800 bytes with the flag, 3 x 1300 x 4 = 15600 bytes without (7 and 10 workgroups per CU by
//     LDS; tests/test_bloom_isa.py holds both figures).  A row of a plane keeps its 65 even columns in front of its 65 odd ones, so tap i of the 64 lanes of a wave
//     reads 64 consecutive words: no bank conflict, no padding.  The flag is a template parameter: without it wsum is exactly 1 and the kernel carries no division per
//     texel and no wk plane.
//   bloom_downsample_kernel: mip k from mip k - 1, a lane per texel, sixteen 16-byte loads.
//   bloom_upsample_kernel: U_k = mip_k + scatter * Up(U_k+1), a lane per texel, stored over mip_k (it reads no other texel of mip_k).
//   bloom_composite_kernel: the streaming shape of tonemap_finalize_kernel (rtow_tonemap.hip) - the next pixel's loads are issued before this pixel is stored.  It reads
//     only its own pixel of inColor, which is why outColor may be inColor.
// The mips are 16-byte texels (r, g, b, 0) at a 4-byte boundary: one global_load_dwordx4 per tap.
#include "rtow_kernels.h"

namespace rtow {

namespace {

constexpr int kMipTileW = 64, kMipTileH = 4;                                      // texels of mip 1 per workgroup: a lane each, a wave per row
constexpr int kSrcW = 2 * kMipTileW + 2, kSrcH = 2 * kMipTileH + 2;               // 130 x 10 source pixels: (0, 0) is the pixel (2 x0 - 1, 2 y0 - 1)
constexpr int kSrc = kSrcW * kSrcH, kHalfW = kSrcW / 2;
constexpr int kMaxLevels = 8;
static_assert(kSrc == 1300 && kMipTileW * kMipTileH == 256, "1300 words a plane: the LDS figures of tests/test_bloom_isa.py");
static_assert(sizeof(RtowBloomParams) == 40, "include/rtow.h states this size");

struct __attribute__((packed, aligned(4))) F3 { float x, y, z; };
struct __attribute__((packed, aligned(4))) F4 { float x, y, z, w; };       // 16 bytes at a 4-byte boundary: one global_load_dwordx4

__device__ __forceinline__ float sel_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float sel_max(float a, float b) { return a > b ? a : b; }
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float bright_operand(float c)
{
    const float q = c > 0.0f ? c : 0.0f;                                    // NaN and negatives to 0
    return q < 65536.0f ? q : 65536.0f;
}
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

struct BrightArgs { float threshold, knee, exposure; };

template <bool KARIS>
__global__ void __launch_bounds__(256) bloom_prefilter_kernel(int width, int height, int w1, int h1, unsigned tilesX, BrightArgs A,
                                                              const RtowExposureState* __restrict__ state, const float* inColor, F4* mip1)
{
    __shared__ float sB[KARIS ? 4 : 3][kSrc];
    float s = A.exposure;
    if (state) s = A.exposure * (state->valid ? state->exposure : 1.0f);    // what the previous frame's meter left, read here and not by the host
    const float k = A.threshold * A.knee;
    const int x0 = (int)(blockIdx.x % tilesX) * kMipTileW, y0 = (int)(blockIdx.x / tilesX) * kMipTileH;
    const F3* in3 = reinterpret_cast<const F3*>(inColor);
#pragma unroll 1
    for (int t = (int)threadIdx.x; t < kSrc; t += kMipTileW * kMipTileH) {
        const int cx = t % kSrcW, cy = t / kSrcW;
        long long px = 2ll * x0 - 1 + cx, py = 2ll * y0 - 1 + cy;           // 64 bits: 2 x0 + 129 may pass INT32_MAX before the clamp
        px = px < 0 ? 0 : px > width - 1 ? width - 1 : px;
        py = py < 0 ? 0 : py > height - 1 ? height - 1 : py;
        const F3 c = in3[(size_t)py * (size_t)width + (size_t)px];
        const float qr = bright_operand(c.x), qg = bright_operand(c.y), qb = bright_operand(c.z);
        const float le = lum(qr, qg, qb) * s, d = le - A.threshold;
        float m = d;
        if (k > 0.0f) {
            const float r = sel_min(sel_max(d + k, 0.0f), 2.0f * k);
            m = sel_max((r * r) / (4.0f * k), d);
        }
        m = m > 0.0f ? m : 0.0f;
        const float g = (le > 0.0f && le < __builtin_inff()) ? m / le : 0.0f;
        const float br = qr * g, bg = qg * g, bb = qb * g;
        const int word = cy * kSrcW + (cx & 1) * kHalfW + (cx >> 1);        // even columns in front of the odd ones
        sB[0][word] = br; sB[1][word] = bg; sB[2][word] = bb;
        if (KARIS) sB[KARIS ? 3 : 0][word] = 1.0f / (1.0f + lum(br, bg, bb) * s);
    }
    __syncthreads();
    const int lx = (int)threadIdx.x & (kMipTileW - 1), ly = (int)threadIdx.x / kMipTileW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w1 || y >= h1) return;
    constexpr float h[4] = {0.125f, 0.375f, 0.375f, 0.125f};
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int word = (2 * ly + j) * kSrcW + (i & 1) * kHalfW + lx + (i >> 1);
            float w = h[j] * h[i];
            if (KARIS) { w = w * sB[KARIS ? 3 : 0][word]; wsum = wsum + w; }
            ar = ar + w * sB[0][word]; ag = ag + w * sB[1][word]; ab = ab + w * sB[2][word];
        }
    }
    F4 out{ar, ag, ab, 0.0f};                                               // without the flag wsum is exactly 1
    if (KARIS) {
        const bool any = wsum > 0.0f;                                       // NaN fails
        out.x = any ? ar / wsum : 0.0f; out.y = any ? ag / wsum : 0.0f; out.z = any ? ab / wsum : 0.0f;
    }
    mip1[(size_t)y * (size_t)w1 + (size_t)x] = out;
}

__global__ void __launch_bounds__(256) bloom_downsample_kernel(int sw, int sh, int dw, int dh, const F4* __restrict__ src, F4* __restrict__ dst)
{
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (size_t)dw * (size_t)dh) return;
    const int x = (int)(idx % (size_t)dw), y = (int)(idx / (size_t)dw);
    constexpr float h[4] = {0.125f, 0.375f, 0.375f, 0.125f};
    float ar = 0.0f, ag = 0.0f, ab = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const size_t row = (size_t)clampi(2 * y - 1 + j, sh - 1) * (size_t)sw;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const F4 t = src[row + (size_t)clampi(2 * x - 1 + i, sw - 1)];
            const float w = h[j] * h[i];
            ar = ar + w * t.x; ag = ag + w * t.y; ab = ab + w * t.z;
        }
    }
    dst[idx] = F4{ar, ag, ab, 0.0f};
}

// Up(U)(x, y) of the specification: the 2x tent over the coarse mip `U` of cw x ch texels
struct Rgb { float r, g, b; };
__device__ __forceinline__ Rgb tent(const F4* __restrict__ U, int cw, int ch, int x, int y)
{
    const bool ox = (x & 1) != 0, oy = (y & 1) != 0;
    const int bx = ox ? x / 2 : x / 2 - 1, by = oy ? y / 2 : y / 2 - 1;
    const int xs[2] = {clampi(bx, cw - 1), clampi(bx + 1, cw - 1)}, ys[2] = {clampi(by, ch - 1), clampi(by + 1, ch - 1)};
    const float ux[2] = {ox ? 0.75f : 0.25f, ox ? 0.25f : 0.75f}, uy[2] = {oy ? 0.75f : 0.25f, oy ? 0.25f : 0.75f};
    F4 t[4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) t[2 * j + i] = U[(size_t)ys[j] * (size_t)cw + (size_t)xs[i]];
    Rgb a{0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float w = uy[j] * ux[i];
            a.r = a.r + w * t[2 * j + i].x; a.g = a.g + w * t[2 * j + i].y; a.b = a.b + w * t[2 * j + i].z;
        }
    }
    return a;
}

__global__ void __launch_bounds__(256) bloom_upsample_kernel(int cw, int ch, int fw, int fh, float scatter, const F4* __restrict__ coarse, F4* __restrict__ fine)
{
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (size_t)fw * (size_t)fh) return;
    const int x = (int)(idx % (size_t)fw), y = (int)(idx / (size_t)fw);
    const Rgb up = tent(coarse, cw, ch, x, y);
    const F4 m = fine[idx];
    fine[idx] = F4{m.x + scatter * up.r, m.y + scatter * up.g, m.z + scatter * up.b, 0.0f};
}

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// inColor and outColor may be one buffer: no __restrict__ on either
__global__ void __launch_bounds__(256, 8) bloom_composite_kernel(int n, int width, int cw, int ch, float intensity, const F4* __restrict__ U1, const float* inColor,
                                                                 float* outColor)
{
    const F3* in3 = reinterpret_cast<const F3*>(inColor);
    F3* out3 = reinterpret_cast<F3*>(outColor);
    // software pipelined like tonemap_finalize_kernel: the next pixel's loads are issued before this pixel is stored
    const int stride = (int)(gridDim.x * blockDim.x);
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    F3 c{0.0f, 0.0f, 0.0f};
    Rgb up{0.0f, 0.0f, 0.0f};
    if (i < n) {
        c = in3[(size_t)i];
        up = tent(U1, cw, ch, i % width, i / width);
    }
    while (i < n) {
        const int j = n - i > stride ? i + stride : n;                      // no step past INT32_MAX
        F3 c2{0.0f, 0.0f, 0.0f};
        Rgb up2{0.0f, 0.0f, 0.0f};
        if (j < n) {
            c2 = in3[(size_t)j];
            up2 = tent(U1, cw, ch, j % width, j / width);
        }
        F3 o = c;                                                           // a non-finite channel: the pixel is copied through
        if (finite_bits(c.x) && finite_bits(c.y) && finite_bits(c.z)) { o.x = c.x + intensity * up.r; o.y = c.y + intensity * up.g; o.z = c.z + intensity * up.b; }
        out3[(size_t)i] = o;
        c = c2; up = up2;
        i = j;
    }
}

}  // namespace

hipError_t launchBloom(const RtowBloomParams& p, const RtowExposureState* state, const float* inColor, void* scratch, float* outColor, hipStream_t stream)
{
    if (p.levels < 1 || p.levels > kMaxLevels) return hipErrorInvalidValue;
    // mip k: w[k] x h[k] texels at texel `at[k]` of the scratch; level 0 is the frame
    int w[kMaxLevels + 1], h[kMaxLevels + 1];
    size_t at[kMaxLevels + 1], end = 0;
    w[0] = p.width; h[0] = p.height; at[0] = 0;
    for (int k = 1; k <= p.levels; ++k) {
        w[k] = w[k - 1] / 2 + (w[k - 1] & 1); h[k] = h[k - 1] / 2 + (h[k - 1] & 1);
        at[k] = end;
        end += (size_t)w[k] * (size_t)h[k];
    }
    if (end * sizeof(F4) > RTOW_BLOOM_SCRATCH_BYTES(p.width, p.height)) return hipErrorInvalidValue;      // cannot happen: the macro bounds eight levels of every size
    F4* const mips = static_cast<F4*>(scratch);
    const auto blocksOf = [](int tw, int th) { return (unsigned)(((size_t)tw * (size_t)th + 255u) / 256u); };

    const unsigned tilesX = (unsigned)((w[1] + kMipTileW - 1) / kMipTileW), tilesY = (unsigned)((h[1] + kMipTileH - 1) / kMipTileH);
    const BrightArgs A{p.threshold, p.knee, p.exposure};
    if (p.flags & RTOW_BLOOM_KARIS_AVERAGE)
        hipLaunchKernelGGL(bloom_prefilter_kernel<true>, dim3(tilesX * tilesY), dim3(256), 0, stream, p.width, p.height, w[1], h[1], tilesX, A, state, inColor, mips + at[1]);
    else
        hipLaunchKernelGGL(bloom_prefilter_kernel<false>, dim3(tilesX * tilesY), dim3(256), 0, stream, p.width, p.height, w[1], h[1], tilesX, A, state, inColor, mips + at[1]);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (int k = 2; k <= p.levels; ++k) {
        hipLaunchKernelGGL(bloom_downsample_kernel, dim3(blocksOf(w[k], h[k])), dim3(256), 0, stream, w[k - 1], h[k - 1], w[k], h[k], mips + at[k - 1], mips + at[k]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    for (int k = p.levels - 1; k >= 1; --k) {
        hipLaunchKernelGGL(bloom_upsample_kernel, dim3(blocksOf(w[k], h[k])), dim3(256), 0, stream, w[k + 1], h[k + 1], w[k], h[k], p.scatter, mips + at[k + 1], mips + at[k]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // the grid of the streaming post passes (rtow_tonemap.hip): one workgroup per 256 pixels, dispatched in order
    constexpr int kMaxBlocks = 1048576;
    const int n = p.width * p.height;
    const int blocks = n < 256 * kMaxBlocks ? (n + 255) / 256 : kMaxBlocks;
    hipLaunchKernelGGL(bloom_composite_kernel, dim3(blocks > 0 ? blocks : 1), dim3(256), 0, stream, n, p.width, w[1], h[1], p.intensity, mips + at[1], inColor, outColor);
    return hipGetLastError();
}

}  // namespace rtow
