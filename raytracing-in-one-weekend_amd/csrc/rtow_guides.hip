// rtow_guides.hip - rtowTraceGuideRaysDevice / rtowTraceGuideViewDevice: the first surface that is NOT perfectly specular, seen through mirrors and glass.
//
// The trace calls (rtow_trace.hip) stop at the first surface.  On a mirror or a glass ball that is the wrong place for a guide: the sample path itself takes its albedo and
// normal AOVs from the first hit whose material is not Material.IsPerfectSpecular (JOBS/SampleBatchJob.cs:316-328).  This unit walks that chain without random numbers:
// segment after segment of rtow_trace.hip's walk, with the sample kernel's own HIT-stage expressions between two segments - the hit point, Material.Scatter at roughness 0
// with the coin taken out (mirror: reflect; glass: refract, reflect on total internal reflection), the offset of the next origin - until a surface that is not perfectly
// specular, the sky, or maxBounces.  It reports the END of the chain in the form the trace calls use (distance, entity, normal of the last segment, and that segment's
// ray), so that rtowShadeHitsDevice, rtowDenoiseDevice and rtowUpsampleDevice work on it unchanged.  include/rtow.h holds the numeric specification.
//
// Launch shape: rtow_trace.hip's - 256-lane workgroups, one lane per ray (view form: a wave per 8 x 8 pixel tile), no barrier, no scratch, tree, primitives
// and materials from HBM / L2 (load_node<false>, general_hit<false>), the [entry][lane] LDS stack of rtow_trace_lanes.hip.h (26 x 256 x 4 B), emptied before every segment.
// A lane whose chain has ended waits for the last lane of its wave: no regrouping - a wave of a view tile mostly follows one object.  The loop runs at most
// maxBounces + 1 <= RTOW_GUIDE_MAX_BOUNCES + 1 walks per lane (the API refuses a larger maxBounces).
//
// Memory safety: a ray's floats are only ever operands, never addresses.  Primitive and material numbers come from the walk and the scene image, as in the sample kernel;
// texels are clamped and image numbers checked by rtow_albedo.hip.h as for rtowShadeHitsDevice.
#include "rtow_albedo.hip.h"
#include "rtow_trace_lanes.hip.h"

namespace rtow {

namespace {

struct GuideArgs {
    SceneBinding scene;             // device image of the scene, entity map, layout (rtow_kernels.h)
    TexRefs tex;
    uint32_t imageCount;            // GpuImage records in the texture blob
    int32_t maxBounces;
    RtowHitBuffers hits;            // RtowGuideBuffers, member by member
    RtowRay* outRays;
    float* throughput;
    float* pathDistance;
    int32_t* bounces;
    uint8_t* end;
    // ray form
    const RtowRay* rays;
    long long count;
    // view form (set_view)
    RtowView view;
    float time, sizeX, sizeY;
    int width, height;
    unsigned tilesX;
    unsigned long long tiles;
};

enum : unsigned { GUIDE_END_SKY = 0, GUIDE_END_SURFACE = 1, GUIDE_END_CUT = 2 };

template <int BASE, bool VIEW>
__global__ void __launch_bounds__(kTraceBlock) guide_kernel(GuideArgs A)
{
    __shared__ int stackRows[kTraceStackEntries * kTraceBlock];
    size_t index;
    V3 ro, rd;
    float time;
    if (VIEW) {
        const unsigned long long tile = view_tile();
        if (tile >= A.tiles) return;
        int cx, cy;
        view_pixel(A, tile, cx, cy);
        if (cx >= A.width || cy >= A.height) return;
        view_ray(A, cx, cy, index, ro, rd, time);
    } else {
        const long long i = (long long)blockIdx.x * kTraceBlock + threadIdx.x;
        if (i >= A.count) return;
        index = (size_t)i;
        const Ray8 r = reinterpret_cast<const Ray8*>(A.rays)[index];      // read before anything is written: A.rays may be A.outRays
        ro = v3(r.ox, r.oy, r.oz);      // (not load_ray: with it the compiler orders two moves of this kernel differently)
        time = r.time;
        rd = v3(r.dx, r.dy, r.dz);
    }
    const SceneLayout& L = A.scene.layout;
    const SceneRefs sc = global_scene(A.scene.blob);
    LdsStack stack;
    stack.col = stackRows + threadIdx.x;

    V3 T = v3(1, 1, 1), N = v3(0, 0, 0);
    float D = 0.0f, t;
    int prim, b = 0;
    unsigned end;
    for (;;) {
        // ---- 1. nearest hit: one ray of rtowTraceRaysDevice ----
        float rtime;
        stack.sp = 0;
        (void)walk<BASE, WALK_OPEN>(A.scene.blob, L, ro, rd, time, 0.0f, 0.0f, stack, t, prim, rtime);      // (the launcher refuses a tree deeper than the stack: push cannot fail)
        N = v3(0, 0, 0);
        if (prim < 0) { end = GUIDE_END_SKY; break; }

        // ---- 2. hit record (HIT of the sample kernel) ----
        D = D + t;
        const PrimMaterial pm = prim_material(sc, L, prim);
        const uint8_t* mp = pm.record;
        const float4 m2 = *reinterpret_cast<const float4*>(mp + 32);  // glossiness parameter flags roughness
        const unsigned flags = __float_as_uint(m2.z);
        const bool specular = (flags & MAT_FLAG_PERFECT_SPECULAR) != 0;
        const bool follow = specular && b != A.maxBounces;
        if (follow || A.hits.normal) N = hit_normal<BASE>(sc, L, prim, ro, rd, rtime, 0.0f, t);     // the last segment's normal is derived only for a caller who asks for it
        if (!follow) { end = specular ? GUIDE_END_CUT : GUIDE_END_SURFACE; break; }
        const V3 P = v3(ro.x + t * rd.x, ro.y + t * rd.y, ro.z + t * rd.z);           // ray.GetPoint(distance)

        // ---- 3. Material.Scatter at roughness 0, without its random numbers (RT/Material.cs:75-161) ----
        const float4 m0 = *reinterpret_cast<const float4*>(mp);       // albedo.xyz emission.x
        const float4 m1 = *reinterpret_cast<const float4*>(mp + 16);  // emission.yz type metallic
        float2 uv = make_float2(0, 0);
        if (textures_evaluated<BASE>(A.tex, flags)) uv = hit_tex_coord<BASE>(sc, L, prim, pm.word, ro, rd);
        V3 tint = material_albedo<BASE>(A.tex, A.imageCount, pm.index, v3(m0.x, m0.y, m0.z), flags, uv);
        V3 sdir;
        if (__float_as_int(m1.z) == RTOW_MATERIAL_STANDARD) {
            sdir = reflect(rd, N);                                     // the metal branch; the untinted glossy branch (reflectionChance) is left out
        } else {
            // Dielectric, followed along its mean direction (roughN = normalize(N + 0)); Schlick's reflection is left out
            const float ior = m2.y, invIor = *reinterpret_cast<const float*>(mp + 60);
            const V3 rn = normalize(N);
            const float dn = dot(rd, rn);
            V3 on;
            float nn;
            if (dn > 0) { on = neg(rn); nn = ior; }
            else { on = rn; nn = invIor; }
            // Refract (:198-210)
            const float dt = dot(rd, on);
            const float disc = 1 - nn * nn * (1 - dt * dt);
            if (disc > 0) {
                const float sq = RTOW_SQRT(disc);
                sdir = v3(nn * (rd.x - on.x * dt) - on.x * sq,
                          nn * (rd.y - on.y * dt) - on.y * sq,
                          nn * (rd.z - on.z * dt) - on.z * sq);
            } else {
                sdir = reflect(rd, rn);                                // total internal reflection (a NaN discriminant too)
                tint = v3(1, 1, 1);
            }
        }
        T = v3(T.x * tint.x, T.y * tint.y, T.z * tint.z);

        // ---- 4. ray = scattered.OffsetTowards(dot(dir, N) >= 0 ? N : -N)  (JOBS/SampleBatchJob.cs:335-336, RT/Ray.cs:18) ----
        const V3 offN = dot(sdir, N) >= 0 ? N : neg(N);
        ro = v3(P.x + 0.001f * offN.x, P.y + 0.001f * offN.y, P.z + 0.001f * offN.z);
        rd = sdir;
        b++;
    }

    store_hit_place(A, index, t, prim);
    if (A.hits.normal) store_hit_normal(A, index, N);
    if (A.outRays) reinterpret_cast<Ray8*>(A.outRays)[index] = Ray8{ro.x, ro.y, ro.z, time, rd.x, rd.y, rd.z, 0.0f};
    if (A.throughput) { float* o = A.throughput + index * 3u; o[0] = T.x; o[1] = T.y; o[2] = T.z; }
    if (A.pathDistance) A.pathDistance[index] = D;
    if (A.bounces) A.bounces[index] = b;
    if (A.end) A.end[index] = (uint8_t)end;
}

template <bool VIEW>
hipError_t launch(const GuideArgs& A, unsigned long long blocks, hipStream_t stream)
{
    return launch_query(A.scene.layout, blocks, [&](auto base, dim3 grid, dim3 block) { hipLaunchKernelGGL((guide_kernel<decltype(base)::value, VIEW>), grid, block, 0, stream, A); });
}

GuideArgs guide_args(const QueryScene& scene, int32_t maxBounces, const RtowGuideBuffers& out)
{
    GuideArgs A{};
    A.scene = scene.binding;
    A.tex = scene.tex;
    A.imageCount = image_count(scene.tex.layout);
    A.maxBounces = maxBounces;
    A.hits = out.hits;
    A.outRays = out.rays;
    A.throughput = out.throughput;
    A.pathDistance = out.pathDistance;
    A.bounces = out.bounces;
    A.end = out.end;
    return A;
}

}  // namespace

hipError_t launchTraceGuideRays(const QueryScene& scene, int32_t maxBounces, int64_t count, const RtowRay* rays, const RtowGuideBuffers& out, hipStream_t stream)
{
    GuideArgs A = guide_args(scene, maxBounces, out);
    A.rays = rays;
    A.count = count;
    return launch<false>(A, ((unsigned long long)count + kTraceBlock - 1) / kTraceBlock, stream);
}

hipError_t launchTraceGuideView(const QueryScene& scene, int32_t maxBounces, const RtowTraceViewParams& p, const RtowGuideBuffers& out, hipStream_t stream)
{
    GuideArgs A = guide_args(scene, maxBounces, out);
    return launch<true>(A, set_view(A, p), stream);
}

}  // namespace rtow
