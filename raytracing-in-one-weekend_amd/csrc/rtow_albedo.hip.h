// rtow_albedo.hip.h - Albedo.SampleColor(rec.TexCoords) of a named primitive for a given ray: the one evaluation behind rtowShadeHitsDevice's albedo (rtow_shade.hip) and the
// tint of a surface that rtowTraceGuide*Device follows (rtow_guides.hip).  The material's folded constant, or - for a material with an Image texture - the texel at the
// triangle's UV, found by the triangle's own test once more (tMin 0) as the HIT stage of the textured sample kernels does for the winner.
// Also the checked forms of texture_color / texture_scalar the shade pass evaluates the other three textures with, and prim_material (rtow_guides.hip, rtow_record_paths.hip).
#pragma once
#include "rtow_hit_tests.hip.h"
#include "rtow_surface.hip.h"

namespace rtow {

namespace {

// texture_color / texture_scalar index the image table with t.image: an image number that is not the blob's samples as the null image does (0).  The record is read where
// it lies in the blob: a private copy of it would be a per-lane array (texture_scalar selects a channel of mainColor)
__device__ __forceinline__ bool no_such_image(const GpuTexture& t, uint32_t imageCount)
{
    return t.type == RTOW_TEXTURE_IMAGE && t.image >= 0 && (uint32_t)t.image >= imageCount;
}
__device__ __forceinline__ V3 color_checked(const TexRefs& tex, const GpuTexture& t, float2 uv, uint32_t imageCount)
{
    return no_such_image(t, imageCount) ? v3(0, 0, 0) : texture_color(tex, t, uv);
}
__device__ __forceinline__ float scalar_checked(const TexRefs& tex, const GpuTexture& t, float2 uv, uint32_t imageCount)
{
    return no_such_image(t, imageCount) ? 0.0f : texture_scalar(tex, t, uv);
}

// GpuImage records in a texture blob (0: no blob)
inline uint32_t image_count(const TexLayout& T) { return T.totalBytes ? (T.pixelOffset - T.imageOffset) / (uint32_t)sizeof(GpuImage) : 0u; }

// The material of a primitive the walk found, as the HIT stage finds it: the primitive's matIndex word (rtow_scene.h), the material's number and the address of its
// 64-byte record.  (rtow_shade.hip, whose primitive is the caller's, checks the number before it forms the address; with this helper its kernels compile to other code.)
struct PrimMaterial { unsigned word, index; const uint8_t* record; };
__device__ __forceinline__ PrimMaterial prim_material(const SceneRefs& sc, const SceneLayout& L, int prim)
{
    PrimMaterial m;
    m.word = *reinterpret_cast<const unsigned*>(section<false>(sc, L.matIndexOffset) + (uint32_t)prim * 4u);
    m.index = m.word & 0xffffu;
    m.record = section<false>(sc, L.materialOffset) + m.index * 64u;
    return m;
}

// HitRecord.TexCoords of primitive `prim` (mi: its matIndex word) for the ray: the named triangle's own test once more (tMin 0), as HIT does for the winner; every other
// entity type, and a ray that does not meet the triangle, leaves (0, 0)
template <int BASE>
__device__ __forceinline__ float2 hit_tex_coord(const SceneRefs& sc, const SceneLayout& L, int prim, unsigned mi, V3 ro, V3 rd)
{
    float2 uv = make_float2(0, 0);
    if (BASE >= SCENE_KIND_GENERAL && (mi >> kPrimTypeShift) == RTOW_ENTITY_TRIANGLE) {
        float t2; V3 nLocal; float4 rq;
        (void)general_hit<false>(sc, L, prim, RTOW_ENTITY_TRIANGLE, ro, rd, 0.0f, 0.0f, t2, nLocal, rq, &uv);
    }
    return uv;
}

// whether material records with MAT_FLAG_TEXTURED in `flags` have their textures evaluated per hit (Material.Scatter / Emit at rec.TexCoords, RT/Material.cs:71,77-78,123,176-179)
template <int BASE>
__device__ __forceinline__ bool textures_evaluated(const TexRefs& tex, unsigned flags)
{
    return BASE >= SCENE_KIND_GENERAL && (flags & MAT_FLAG_TEXTURED) && tex.blob && tex.layout.totalBytes != 0u;
}
__device__ __forceinline__ const GpuTexMaterial& tex_material(const TexRefs& tex, unsigned matIdx)
{
    return reinterpret_cast<const GpuTexMaterial*>(tex.blob + tex.layout.materialOffset)[matIdx];
}

// Albedo.SampleColor(uv) of a material whose textures are evaluated per hit ...
__device__ __forceinline__ V3 textured_albedo(const TexRefs& tex, uint32_t imageCount, unsigned matIdx, float2 uv)
{
    return color_checked(tex, tex_material(tex, matIdx).albedo, uv, imageCount);
}
// ... and of any material matIdx: `folded` (the record's first three floats) unless its textures are evaluated per hit
template <int BASE>
__device__ __forceinline__ V3 material_albedo(const TexRefs& tex, uint32_t imageCount, unsigned matIdx, V3 folded, unsigned flags, float2 uv)
{
    return textures_evaluated<BASE>(tex, flags) ? textured_albedo(tex, imageCount, matIdx, uv) : folded;
}

} // namespace

} // namespace rtow
