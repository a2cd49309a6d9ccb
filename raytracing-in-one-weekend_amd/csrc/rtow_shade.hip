// rtow_shade.hip - rtowShadeHitsDevice: the material of every first hit, on the device.
//
// The trace calls (rtow_trace.hip) answer WHERE a ray meets the scene: distance, entity, normal.  This pass answers WHAT it meets there: the surface's albedo and emission at
// the hit's texture coordinates, metallic and glossiness, the material's index and kind - the raw values of the first surface, nothing traced through glass or mirrors - and
// the sky colour where the ray meets nothing.  Together with rtowTraceViewDevice's normals that is a noise-free G-buffer: guides for rtowDenoiseDevice, a material id under
// the cursor, a material to match on in rtowReprojectAccumDevice's host.  include/rtow.h holds the numeric specification.
//
// Every value is computed by the sample kernel's own helpers (rtow_hit_tests.hip.h: general_hit's texCoord as the HIT stage of the textured kernels asks for it;
// rtow_surface.hip.h: texture_color / texture_scalar, cubemap_sample; sky_color, the SKY stage's expressions), so the pass cannot drift from what a sample batch shades with.
// The albedo comes through rtow_albedo.hip.h, which rtow_guides.hip tints the surfaces it follows with: one evaluation for both.
//
// Launch shape: a plain grid of 256-lane workgroups, one lane per element, no LDS, no barrier; a lane without an element leaves at once.  The scene comes
// from HBM / L2 (general_hit<false>): one primitive record, one material record and at most four texels per element.
//
// Memory safety: `rays` and `entityIndex` are the caller's.  An entity index outside [0, entityCount) is a miss; so is an entity whose primitive number (primOfEntity, or the
// index itself) is not one of the scene's, and a material index beyond the scene's materials.  An Image texture whose image number is not one of the blob's samples as a null
// image.  Texels are clamped into their image by texture_pixel, after (int) conversions that saturate on this hardware (NaN: 0), as in cubemap_sample, whose face coordinates
// (u, v) lie in [-1, 1] or are NaN for every direction.  A ray's floats are only ever operands, never addresses.
#include "rtow_albedo.hip.h"

namespace rtow {

namespace {

constexpr int kShadeBlock = 256;

struct ShadeArgs {
    const uint8_t* sceneBlob;
    SceneLayout layout;
    TexRefs tex;
    CubemapRefs cubemap;
    RtowEnvironment environment;
    const int32_t* primOfEntity;    // the host's entity index -> primitive, -1 = none; null: the same number
    const RtowRay* rays;
    const int32_t* entityIndex;
    RtowSurfaceBuffers out;
    int32_t count;
    int32_t entityCount;
    uint32_t imageCount;            // GpuImage records in the texture blob
};

template <int BASE>
__global__ void __launch_bounds__(kShadeBlock) shade_kernel(ShadeArgs A)
{
    const long long i = (long long)blockIdx.x * kShadeBlock + threadIdx.x;
    if (i >= (long long)A.count) return;
    const size_t index = (size_t)i;
    const SceneLayout& L = A.layout;
    const Ray8 r = reinterpret_cast<const Ray8*>(A.rays)[index];
    const V3 ro = v3(r.ox, r.oy, r.oz), rd = v3(r.dx, r.dy, r.dz);
    const SceneRefs sc = global_scene(A.sceneBlob);

    // entity -> primitive -> material, each checked before it is an address
    const int32_t e = A.entityIndex[index];
    int prim = -1;
    if (e >= 0 && e < A.entityCount) prim = A.primOfEntity ? A.primOfEntity[e] : e;
    if (prim < 0 || (uint32_t)prim >= L.sphereCount) prim = -1;
    unsigned mi = 0, matIdx = 0;
    if (prim >= 0) {
        mi = *reinterpret_cast<const unsigned*>(section<false>(sc, L.matIndexOffset) + (uint32_t)prim * 4u);
        matIdx = mi & 0xffffu;
        if (matIdx >= L.materialCount) prim = -1;
    }

    V3 albedo = v3(0, 0, 0), emission = v3(0, 0, 0);
    float2 uv = make_float2(0, 0), mg = make_float2(0, 0);
    int32_t materialIndex = -1;
    uint32_t materialInfo = 0xffffffffu;
    if (prim >= 0) {
        uv = hit_tex_coord<BASE>(sc, L, prim, mi, ro, rd);
        const uint8_t* mp = section<false>(sc, L.materialOffset) + matIdx * 64u;      // (not prim_material: the number is checked before it is part of an address)
        const float4 m0 = *reinterpret_cast<const float4*>(mp);       // albedo.xyz emission.x
        const float4 m1 = *reinterpret_cast<const float4*>(mp + 16);  // emission.yz type metallic
        const float4 m2 = *reinterpret_cast<const float4*>(mp + 32);  // glossiness parameter flags roughness
        albedo = v3(m0.x, m0.y, m0.z);
        emission = v3(m0.w, m1.x, m1.y);
        mg = make_float2(m1.w, m2.x);
        const unsigned flags = __float_as_uint(m2.z);
        if (textures_evaluated<BASE>(A.tex, flags)) {
            const GpuTexMaterial& tm = tex_material(A.tex, matIdx);
            albedo = textured_albedo(A.tex, A.imageCount, matIdx, uv);
            emission = color_checked(A.tex, tm.emission, uv, A.imageCount);
            mg = make_float2(scalar_checked(A.tex, tm.metallic, uv, A.imageCount), scalar_checked(A.tex, tm.glossiness, uv, A.imageCount));
        }
        materialIndex = (int32_t)matIdx;
        materialInfo = (__float_as_uint(m1.z) & 0xffu) | ((flags & MAT_FLAG_PERFECT_SPECULAR) ? 0x100u : 0u);
    } else {
        albedo = sky_color(A.environment, A.cubemap, rd);      // sampleAlbedo = hitSkyColor: the SKY stage's expressions on the direction as stored
    }

    if (A.out.albedo) { float* o = A.out.albedo + index * 3u; o[0] = albedo.x; o[1] = albedo.y; o[2] = albedo.z; }
    if (A.out.emission) { float* o = A.out.emission + index * 3u; o[0] = emission.x; o[1] = emission.y; o[2] = emission.z; }
    if (A.out.texCoord) { float* o = A.out.texCoord + index * 2u; o[0] = uv.x; o[1] = uv.y; }
    if (A.out.metallicGlossiness) { float* o = A.out.metallicGlossiness + index * 2u; o[0] = mg.x; o[1] = mg.y; }
    if (A.out.materialIndex) A.out.materialIndex[index] = materialIndex;
    if (A.out.materialInfo) A.out.materialInfo[index] = materialInfo;
}

}  // namespace

hipError_t launchShadeHits(const QueryScene& scene, const RtowEnvironment& environment, int32_t count, const RtowRay* rays, const int32_t* entityIndex,
                           const RtowSurfaceBuffers& surface, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    ShadeArgs A{};
    A.sceneBlob = scene.binding.blob;
    A.layout = scene.binding.layout;
    A.tex = scene.tex;
    A.cubemap = cubemapRefs(scene.cubemap, scene.cubemapData);
    A.environment = environment;
    A.primOfEntity = scene.primOfEntity;
    A.rays = rays;
    A.entityIndex = entityIndex;
    A.out = surface;
    A.count = count;
    A.entityCount = scene.entityCount;
    A.imageCount = image_count(scene.tex.layout);
    const dim3 grid((unsigned)(((long long)count + kShadeBlock - 1) / kShadeBlock)), block(kShadeBlock);
    if (scene.binding.layout.sceneKind == SCENE_KIND_SPHERES) hipLaunchKernelGGL((shade_kernel<SCENE_KIND_SPHERES>), grid, block, 0, stream, A);
    else if (scene.binding.layout.sceneKind == SCENE_KIND_SPHERES_MOTION) hipLaunchKernelGGL((shade_kernel<SCENE_KIND_SPHERES_MOTION>), grid, block, 0, stream, A);
    else hipLaunchKernelGGL((shade_kernel<SCENE_KIND_GENERAL>), grid, block, 0, stream, A);
    return hipGetLastError();
}

}  // namespace rtow
