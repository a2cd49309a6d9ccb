// rtow_surface.hip.h - what a surface or the sky looks like where a ray ends: Cubemap.Sample and Texture.SampleColor / SampleScalar over the launch's CubemapRefs / TexRefs
// (rtow_kernels.h), RoughnessToAlpha, and cold_args, the way a kernel reads launch constants on use instead of holding them in registers.
// Included by rtow_sample_kernel.hip.h (HIT and SKY stages), rtow_shade.hip and rtow_kernels.hip (the materials' derived constants).
#pragma once
#include "rtow_detmath.hip.h"
#include "rtow_kernels.h"
#include "rtow_vecmath.hip.h"

namespace rtow {

namespace {

// Launch constants read where they are used.  A kernel argument that is only needed in a rare or short stage lives in scalar registers (or, spilled, in VGPR lanes and
// scratch) through every stage if nothing is done; read through a laundered pointer to the kernarg segment it is s_load-ed on use instead.  `hot` is the kernel's by-value
// argument struct, which has to be the kernel's ONLY argument: the segment then begins with it.
template <typename Args>
__device__ __forceinline__ const Args& cold_args(const Args& hot)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const Args* cold = (const Args*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(cold));
    (void)hot;
    return *cold;
#else
    return hot;                                                    // host pass of the HIP compiler: never executed
#endif
}

// Microfacet.TrowbridgeReitz.RoughnessToAlpha (RT/Microfacet.cs:9-12): per material where its roughness is a constant (prepare_materials_kernel, rtow_kernels.hip), per hit where
// a texture gives it (HIT)
__device__ __forceinline__ float roughness_to_alpha(float roughness)
{
    roughness = um_max(roughness, 1e-3f);
    const float x = det_log(roughness);
    return 1.62142f + 0.819955f * x + 0.1734f * x * x + 0.0171201f * x * x * x + 0.000640711f * x * x * x * x;
}

// ------------------------------------------------------------------------------------------------------------
// Cubemap.Sample (RT/Texture.cs:171-210): the face is the first axis whose |component| is the largest (x before y before z), the
// texel min((int2)((uv + 1) * halfFaceSize), faceSizeMinusOne) of that face, point sampled; RGBA half or byte channels.
// (The sample kernel hands in cold_args(A).cubemap: nine constants most launches, with their gradient sky, never read.)
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ V3 cubemap_sample(const CubemapRefs& A, V3 d)
{
    if (!A.data) return v3(0, 0, 0);
    const float ax = __builtin_fabsf(d.x), ay = __builtin_fabsf(d.y), az = __builtin_fabsf(d.z);
    const float m = um_max(um_max(um_max(ax, ay), az), 0.0f);                  // cmax(float4(abs(vector), 0))
    int lane;
    if (m == ax) lane = 0; else if (m == ay) lane = 1; else if (m == az) lane = 2; else return v3(0, 0, 0);   // NaN direction
    const float major = lane == 0 ? d.x : lane == 1 ? d.y : d.z;
    const float amajor = lane == 0 ? ax : lane == 1 ? ay : az;
    const bool positive = major >= 0;
    float u, v;
    if (lane == 0) { u = positive ? -d.z : d.z; v = -d.y; }
    else if (lane == 1) { u = d.x; v = positive ? d.z : -d.z; }
    else { u = positive ? d.x : -d.x; v = -d.y; }
    u = u / amajor;
    v = v / amajor;
    int cx = (int)((u + 1) * (float)A.halfW), cy = (int)((v + 1) * (float)A.halfH);
    cx = cx < A.w1 ? cx : A.w1;
    cy = cy < A.h1 ? cy : A.h1;
    const uint8_t* px = A.data + (size_t)(lane * 2 + (positive ? 0 : 1)) * (size_t)A.faceStride + cx * A.pixelStride + cy * A.rowStride;
    if (A.channelType == RTOW_CUBEMAP_UNSIGNED_BYTE) return v3((float)px[0] / 255.0f, (float)px[1] / 255.0f, (float)px[2] / 255.0f);
    const unsigned short* hp = reinterpret_cast<const unsigned short*>(px);
    return v3(half_bits_to_float(hp[0]), half_bits_to_float(hp[1]), half_bits_to_float(hp[2]));
}

// hitSkyColor (JOBS/SampleBatchJob.cs:349-370) of direction rd, the SKY stage's expressions for the query units (rtow_shade.hip, rtow_record_paths.hip; the sample
// kernel keeps its own): the gradient between the two sky colours or the cubemap's texel; any other sky type is black
__device__ __forceinline__ V3 sky_color(const RtowEnvironment& ENV, const CubemapRefs& cubemap, V3 rd)
{
    if (ENV.skyType == RTOW_SKY_GRADIENT) {
        const float s = 0.5f * (rd.y + 1);
        const V3 b = v3(ENV.skyBottomColor), tp = v3(ENV.skyTopColor);
        return v3(b.x + s * (tp.x - b.x), b.y + s * (tp.y - b.y), b.z + s * (tp.z - b.z));
    }
    if (ENV.skyType == RTOW_SKY_CUBEMAP) return cubemap_sample(cubemap, rd);
    return v3(0, 0, 0);
}

// ------------------------------------------------------------------------------------------------------------
// Texture.SampleColor / SampleScalar (RT/Texture.cs:51-138) for the per-hit evaluation of textured materials.  Image: the texel
// (int2)(uv * ImageSize) - clamped into the image, where the reference would read out of bounds - as bytes / 255 * MainColor.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ const uint8_t* texture_pixel(const TexRefs& A, const GpuTexture& t, float2 uv)
{
    const GpuImage im = reinterpret_cast<const GpuImage*>(A.blob + A.layout.imageOffset)[t.image];
    int x = (int)(uv.x * (float)im.width), y = (int)(uv.y * (float)im.height);
    x = x < 0 ? 0 : x > im.width - 1 ? im.width - 1 : x;
    y = y < 0 ? 0 : y > im.height - 1 ? im.height - 1 : y;
    return A.blob + A.layout.pixelOffset + im.offset + ((size_t)y * (size_t)im.width + (size_t)x) * (size_t)im.pixelStride;
}
__device__ __forceinline__ V3 texture_color(const TexRefs& A, const GpuTexture& t, float2 uv)
{
    if (t.type == RTOW_TEXTURE_CONSTANT) return v3(t.mainColor[0], t.mainColor[1], t.mainColor[2]);
    if (t.type == RTOW_TEXTURE_CONSTANT_SCALAR) return v3(t.parameter, t.parameter, t.parameter);
    if (t.type == RTOW_TEXTURE_IMAGE && t.image >= 0) {
        const uint8_t* px = texture_pixel(A, t, uv);
        return v3((float)px[0] / 255.0f * t.mainColor[0], (float)px[1] / 255.0f * t.mainColor[1], (float)px[2] / 255.0f * t.mainColor[2]);
    }
    return v3(0, 0, 0);
}
__device__ __forceinline__ float texture_scalar(const TexRefs& A, const GpuTexture& t, float2 uv)
{
    const float main = t.channel == 0 ? t.mainColor[0] : t.channel == 1 ? t.mainColor[1] : t.mainColor[2];
    if (t.type == RTOW_TEXTURE_CONSTANT) return main;
    if (t.type == RTOW_TEXTURE_CONSTANT_SCALAR) return t.parameter;
    if (t.type == RTOW_TEXTURE_IMAGE && t.image >= 0) return (float)texture_pixel(A, t, uv)[t.channel] / 255.0f * main;
    return 0.0f;
}

} // namespace

} // namespace rtow
