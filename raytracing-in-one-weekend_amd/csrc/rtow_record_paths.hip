// rtow_record_paths.hip - rtowRecordPathsDevice: one sample of a pixel replayed segment by segment (the reference's PATH_DEBUGGING, JOBS/SampleBatchJob.cs:53-55,96-101,
// 140-142,304-307,344-347), and a second, straight-line implementation of the sample path to hold the megakernel (rtow_sample_kernel.hip.h) to, pixel by pixel.
//
// One lane per list entry, one bounce after the other: the pixel's generator as begin_pixel sets it up, the sample count from the pixel's accumulated weight (:118-126),
// then samples 0 .. N - 1 on that one random stream - the camera ray (REGEN), the nearest hit (one ray of rtowTraceRaysDevice: rtow_walk.hip.h), Material.Scatter and
// Material.Emit (HIT) and the sky with the fold tail -> head (SKY), each in the megakernel's expressions on the megakernel's helpers, every draw in its order (the Lambert
// class's unused rough-normal draw and the raw ray-time draw included).  One sample is reported: the one the caller names, or the one that ranks first by luminance (a
// first pass over all N that keeps the best key and the generator as it stood at that sample's start, then that sample once more).  include/rtow.h holds the specification.
//
// The emission / attenuation stacks (:103-104,311,330) are not private arrays: a lane keeps them in its own segment slots (the attenuation and emission fields, written as
// the path goes and read back tail -> head), or - for a caller without `segments` - in its rows of a scratch block the context owns (24 bytes per depth).
//
// Launch shape: rtow_trace.hip's - 256-lane workgroups, no barrier, no scratch, tree, primitives and materials from HBM / L2, the [entry][lane] LDS stack of
// rtow_trace_lanes.hip.h, emptied before every segment.  Lanes of a wave follow their own paths and sample counts; a lane that is done waits for the last one.
// No ProbabilisticVolume branch (it needs every hit of a ray): the entry point refuses such a scene.
//
// Memory safety: a list entry is compared with the frame's pixel count before it is an address (flags bit 2 otherwise); the count read from words[0] is clamped to the
// capacity the launch was sized with.  Primitive and material numbers come from the walk and the scene image, as in the sample kernel; texels are clamped and image numbers
// checked by rtow_albedo.hip.h as for rtowShadeHitsDevice.  A ray's floats are only ever operands, never addresses.
#include "rtow_sample_kernel.hip.h"

#include "rtow_albedo.hip.h"
#include "rtow_trace_lanes.hip.h"

namespace rtow {

namespace {

struct RecordArgs {
    SampleKernelArgs S;             // what buildArgs (rtow_api.hip) fills for a batch of these params: view, environment, seed, counts, extrema, noise textures, scene, textures, cubemap
    const int32_t* entityOfPrim;    // primitive -> the host's entity index, or null (the same number)
    uint32_t imageCount;            // GpuImage records in the texture blob
    const uint32_t* words;          // the caller's list, read in place
    uint32_t capacity;
    int32_t select, sampleIndex;
    RtowPathSummary* summaries;
    RtowPathSegment* segments;      // may be null
    float* stackRows;               // segments == null: capacity x traceDepth x (attenuation.xyz emission.xyz)
};

// a lane's emission / attenuation stack: inside its segment slots, or its rows of the scratch block
struct PathStack {
    float* base;
    unsigned stride, emission;      // floats between two depths; from a depth's attenuation to its emission
    __device__ __forceinline__ void set(int depth, V3 a, V3 e) const
    {
        float* p = base + (size_t)depth * stride;
        p[0] = a.x; p[1] = a.y; p[2] = a.z;
        p[emission] = e.x; p[emission + 1] = e.y; p[emission + 2] = e.z;
    }
    __device__ __forceinline__ V3 attenuation(int depth) const { const float* p = base + (size_t)depth * stride; return v3(p[0], p[1], p[2]); }
    __device__ __forceinline__ V3 emitted(int depth) const { const float* p = base + (size_t)depth * stride + emission; return v3(p[0], p[1], p[2]); }
};

__device__ __forceinline__ RtowFloat3 f3(V3 a) { RtowFloat3 r; r.x = a.x; r.y = a.y; r.z = a.z; return r; }
__device__ __forceinline__ float path_luminance(V3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

struct SampleResult {
    V3 color, normal, albedo;
    float randomEvents, time;
    int rays;
    bool ok;
};

// Sample (JOBS/SampleBatchJob.cs:166-401) of pixel (cx, cy) on `rng`; seg: the pixel's segment slots to fill (null: a sample that is only run)
template <int BASE, int NOISE>
__device__ __forceinline__ SampleResult run_sample(const RecordArgs& A, const NoiseSite& at, Rng<NOISE>& rng, int cx, int cy, LdsStack& stack, const PathStack& hist,
                                                   RtowPathSegment* seg)
{
    const SampleKernelArgs& S = A.S;
    const SceneLayout& L = S.layout;
    const SceneRefs sc = global_scene(S.sceneBlob);
    const int traceDepth = S.traceDepth;

    // ---- camera ray (:134-135, RT/View.cs:38-48): REGEN of the sample kernel ----
    // (the view's, the sky's, the textures' and the cubemap's launch constants are read on use - cold_args - instead of living in scalar registers through the walk)
    const SampleKernelArgs& VS = cold_args(A).S;
    const RtowView& VW = VS.view;
    const V3 viewRight = v3(VW.right), viewUp = v3(VW.up);
    const V3 viewLLC = v3(VW.lowerLeftCorner), viewH = v3(VW.horizontal), viewV = v3(VW.vertical);
    const float lensRadius = VW.lensRadius;
    float jx = 0.5f, jy = 0.5f;
    if (VS.subPixelJitter) rng.next2(at, jx, jy);
    const float u = ((float)cx + jx) / VS.sizeX;
    const float v = ((float)cy + jy) / VS.sizeY;
    float rdx = 0, rdy = 0;
    if (lensRadius != 0) {
        float dx, dy;
        rng.in_unit_disk(at, dx, dy);
        rdx = lensRadius * dx;
        rdy = lensRadius * dy;
    }
    const V3 offset = v3(viewRight.x * rdx + viewUp.x * rdy, viewRight.y * rdx + viewUp.y * rdy, viewRight.z * rdx + viewUp.z * rdy);
    V3 ro = add(v3(VW.origin), offset);
    V3 rd = normalize(v3(viewLLC.x - offset.x + u * viewH.x + v * viewV.x,
                         viewLLC.y - offset.y + u * viewH.y + v * viewV.y,
                         viewLLC.z - offset.z + u * viewH.z + v * viewV.z));
    const float time = rng.next(at);      // Ray.Time as drawn; the walk derives what sphere_at expects from it, segment by segment (scattered rays inherit the time)

    SampleResult R;
    R.color = v3(0, 0, 0); R.normal = v3(0, 0, 0); R.albedo = v3(0, 0, 0);
    R.randomEvents = 0; R.time = time; R.rays = 0; R.ok = false;
    bool firstNonSpecular = false;
    int depth = 0;
    for (;;) {
        // ---- nearest hit: one ray of rtowTraceRaysDevice ----
        float t, rtime;
        int prim;
        stack.sp = 0;
        (void)walk<BASE, WALK_OPEN>(S.sceneBlob, L, ro, rd, time, 0.0f, 0.0f, stack, t, prim, rtime);      // (the launcher refuses a tree deeper than the stack: push cannot fail)
        R.rays++;                                                                                          // :203

        if (prim < 0) {
            // ---- sky (:341-374), then fold tail -> head (:384-396): SKY of the sample kernel ----
            const SampleKernelArgs& ES = cold_args(A).S;
            const V3 sky = sky_color(ES.environment, ES.cubemap, rd);
            if (!firstNonSpecular) { R.albedo = sky; R.normal = neg(rd); }
            if (seg) {
                RtowPathSegment s;
                s.from = f3(ro); s.distance = __builtin_inff();
                s.direction = f3(rd); s.entityIndex = -1;
                s.to = f3(v3(rd.x * 99999.0f, rd.y * 99999.0f, rd.z * 99999.0f)); s.info = 0xffffu | ((uint32_t)RTOW_PATH_SKY << 16);
                s.normal = f3(v3(0, 0, 0)); s.randomEvents = 0.0f;
                s.attenuation = f3(v3(1, 1, 1)); s.pad0 = 0.0f;
                s.emission = f3(sky); s.pad1 = 0.0f;
                seg[depth] = s;
            }
            V3 col = sky; // 0 * 1 + sky
            for (int i = depth - 1; i >= 0; i--) {
                const V3 att = hist.attenuation(i), em = hist.emitted(i);
                col = v3(col.x * att.x + em.x, col.y * att.y + em.y, col.z * att.z + em.z);
            }
            R.color = col;
            R.ok = true;
            break;
        }

        // ---- surface hit: Entity.Hit record + Material.Scatter: HIT of the sample kernel ----
        const PrimMaterial pm = prim_material(sc, L, prim);
        const unsigned matIdx = pm.index, cls = (pm.word >> 16) & 3u;
        const V3 P = v3(ro.x + t * rd.x, ro.y + t * rd.y, ro.z + t * rd.z);           // ray.GetPoint(distance)
        const V3 N = hit_normal<BASE>(sc, L, prim, ro, rd, rtime, 0.0f, t);
        const uint8_t* mp = pm.record;
        const float4 m0 = *reinterpret_cast<const float4*>(mp);       // albedo.xyz emission.x
        const float4 m1 = *reinterpret_cast<const float4*>(mp + 16);  // emission.yz type metallic
        float4 m2 = *reinterpret_cast<const float4*>(mp + 32);        // glossiness parameter flags roughness
        float4 m3 = *reinterpret_cast<const float4*>(mp + 48);        // alpha ior r0 1/ior
        V3 reflectance = v3(m0.x, m0.y, m0.z);
        V3 emission = v3(m0.w, m1.x, m1.y);
        float metallic = m1.w;
        const RecordArgs& TA = cold_args(A);
        const TexRefs& tex = TA.S.tex;
        if (textures_evaluated<BASE>(tex, __float_as_uint(m2.z))) {
            // Material.Scatter / Emit evaluate the four textures at rec.TexCoords, and everything derived from metallic / glossiness follows per hit
            const float2 hitUv = hit_tex_coord<BASE>(sc, L, prim, pm.word, ro, rd);
            const GpuTexMaterial& tm = tex_material(tex, matIdx);
            reflectance = color_checked(tex, tm.albedo, hitUv, TA.imageCount);
            emission = color_checked(tex, tm.emission, hitUv, TA.imageCount);
            const float glossiness = scalar_checked(tex, tm.glossiness, hitUv, TA.imageCount);
            float roughness, ior, invIor = 0.0f, alpha = 0.0f;
            if (__float_as_int(m1.z) == RTOW_MATERIAL_STANDARD) {
                metallic = scalar_checked(tex, tm.metallic, hitUv, TA.imageCount);
                roughness = det_sq(1 - glossiness);
                ior = 1.5f + metallic * (1.1f - 1.5f);
                alpha = roughness_to_alpha(roughness);
            } else {
                roughness = 1 - glossiness;
                ior = m2.y;
                invIor = RTOW_RCP(ior);
            }
            float r0 = (1 - ior) / (1 + ior);
            r0 *= r0;
            m2 = make_float4(glossiness, m2.y, m2.z, roughness);
            m3 = make_float4(alpha, ior, r0, invIor);
        }
        bool perfectSpecular = false;
        unsigned event;
        V3 sdir;
        float randomEvents = 0.0f;
        if (cls == MAT_CLASS_LAMBERT) {
            // Standard with glossiness == 0 and metallic == 0: the rough normal costs one cosine-hemisphere draw whose result is never used
            rng.skip_cosine_hemisphere(at);
            sdir = rng.cosine_hemisphere(at, N);
            randomEvents += 1.0f;
            event = RTOW_PATH_LAMBERT;
        } else if (cls == MAT_CLASS_GENERAL) {                                        // RT/Material.cs:75-119
            const float glossiness = m2.x;
            const float roughness = m2.w;
            perfectSpecular = (__float_as_uint(m2.z) & MAT_FLAG_PERFECT_SPECULAR) != 0;
            V3 roughN = N;
            if (roughness > 0) {
                const V3 h = rng.cosine_hemisphere(at, N);
                roughN = normalize(v3(N.x + roughness * (h.x - N.x), N.y + roughness * (h.y - N.y), N.z + roughness * (h.z - N.z)));
            }
            const float incidentCosine = -dot(rd, roughN);
            const float fresnel = m3.z + (1 - m3.z) * det_pow5(1 - incidentCosine);
            const float g1 = smith_g1(rd, N, m3.x);
            const float reflectionChance = um_saturate(fresnel * glossiness * g1);

            if (reflectionChance > 0 && rng.next(at) < reflectionChance) {
                sdir = reflect(rd, roughN);
                reflectance = v3(1, 1, 1);
                event = RTOW_PATH_GLOSSY;
            } else if (metallic > 0 && rng.next(at) < metallic) {
                sdir = reflect(rd, roughN);
                event = RTOW_PATH_METAL;
            } else {
                sdir = rng.cosine_hemisphere(at, N);
                event = RTOW_PATH_LAMBERT;
            }
            if (reflectionChance > 0 && reflectionChance < 1) randomEvents++;
            if (metallic > 0 && metallic < 1) randomEvents++;
            randomEvents += roughness * (reflectionChance + (1 - reflectionChance) * metallic);
            randomEvents += (1 - reflectionChance) * (1 - metallic);
        } else {                                                                      // Dielectric, RT/Material.cs:121-161 (a volume class cannot come here: the entry point refuses the scene)
            perfectSpecular = true;
            const float ior = m2.y;
            const float roughness = m2.w;
            const V3 rdir = rng.direction(at);
            const V3 roughN = normalize(v3(N.x + roughness * rdir.x, N.y + roughness * rdir.y, N.z + roughness * rdir.z));

            float niOverNt, cosine;
            V3 outwardN;
            const float dDotN = dot(rd, roughN);
            if (dDotN > 0) { outwardN = neg(roughN); niOverNt = ior; cosine = ior * dDotN; }
            else { outwardN = roughN; niOverNt = m3.w; cosine = -dDotN; }

            // Refract (:198-210)
            const float dt = dot(rd, outwardN);
            const float disc = 1 - niOverNt * niOverNt * (1 - dt * dt);
            bool refractOk = false;
            if (disc > 0) {
                const float sq = RTOW_SQRT(disc);
                const V3 refracted = v3(niOverNt * (rd.x - outwardN.x * dt) - outwardN.x * sq,
                                        niOverNt * (rd.y - outwardN.y * dt) - outwardN.y * sq,
                                        niOverNt * (rd.z - outwardN.z * dt) - outwardN.z * sq);
                const float schlickV = m3.z + (1 - m3.z) * det_pow5(1 - cosine);
                if (rng.next(at) > schlickV) { sdir = refracted; refractOk = true; }
            }
            event = RTOW_PATH_REFRACT;
            if (!refractOk) {
                sdir = reflect(rd, roughN);
                reflectance = v3(1, 1, 1);
                event = RTOW_PATH_REFLECT;
            }
            randomEvents++;
            randomEvents += roughness;
        }

        hist.set(depth, reflectance, emission);                                       // :311,330
        if (seg) {
            RtowPathSegment s;
            s.from = f3(ro); s.distance = t;
            s.direction = f3(rd); const int32_t* const entityOfPrim = cold_args(A).entityOfPrim;
            s.entityIndex = entityOfPrim ? entityOfPrim[prim] : prim;
            s.to = f3(P); s.info = matIdx | ((uint32_t)event << 16) | (perfectSpecular ? 1u << 19 : 0u);
            s.normal = f3(N); s.randomEvents = randomEvents;
            s.attenuation = f3(reflectance); s.pad0 = 0.0f;
            s.emission = f3(emission); s.pad1 = 0.0f;
            seg[depth] = s;
        }
        if (depth == 0) R.normal = N;                                                 // :313-314
        if (!firstNonSpecular && !perfectSpecular) {                                  // :316-328
            R.albedo = add(emission, reflectance);
            R.normal = N;
            firstNonSpecular = true;
        }
        R.randomEvents += randomEvents * inv_pow2(depth);                             // :332

        // ray = scattered.OffsetTowards(dot(dir, N) >= 0 ? N : -N)  (:335-336, RT/Ray.cs:18)
        const V3 offN = dot(sdir, N) >= 0 ? N : neg(N);
        ro = v3(P.x + 0.001f * offN.x, P.y + 0.001f * offN.y, P.z + 0.001f * offN.z);
        rd = sdir;
        depth++;
        if (depth == traceDepth) break;                                               // :379-381: the sample fails, its colour stays 0
    }
    return R;
}

template <int BASE, int NOISE>
__global__ void __launch_bounds__(kTraceBlock) record_paths_kernel(RecordArgs A)
{
    __shared__ int stackRows[kTraceStackEntries * kTraceBlock];
    const SampleKernelArgs& S = A.S;
    const size_t index = (size_t)blockIdx.x * kTraceBlock + threadIdx.x;
    const uint32_t listed = A.words[0];
    if (index >= (size_t)(listed < A.capacity ? listed : A.capacity)) return;
    const uint32_t pixel = A.words[4u + index];
    const int traceDepth = S.traceDepth;
    RtowPathSegment* const seg = A.segments ? A.segments + index * (size_t)traceDepth : nullptr;

    RtowPathSummary out;
    out.pixel = (int32_t)pixel; out.sampleIndex = A.sampleIndex; out.sampleCount = 0; out.segmentCount = 0;
    out.flags = 0u; out.time = 0.0f; out.luminance = 0.0f; out.randomEvents = 0.0f;
    out.color = f3(v3(0, 0, 0)); out.normal = f3(v3(0, 0, 0)); out.albedo = f3(v3(0, 0, 0));

    int written = 0;      // segments of this slot that hold a record
    if (pixel >= (uint32_t)S.width * (uint32_t)S.height) {
        out.flags = 4u;   // not a pixel of the frame: never an address
    } else {
        const int cy = (int)(pixel / (uint32_t)S.width), cx = (int)(pixel - (uint32_t)cy * (uint32_t)S.width);
        const NoiseSite at{&S, (unsigned)cx, (unsigned)cy};
        LdsStack stack;
        stack.col = stackRows + threadIdx.x;
        PathStack hist;
        if (seg) { hist.base = &seg->attenuation.x; hist.stride = (unsigned)(sizeof(RtowPathSegment) / sizeof(float)); hist.emission = 4u; }
        else { hist.base = A.stackRows + index * (size_t)traceDepth * 6u; hist.stride = 6u; hist.emission = 3u; }

        // :91 and :118-126: the pixel's generator and its sample count, as the sample kernel's pixel boundary has them
        Rng<NOISE> rng;
        rng.begin_pixel(at, pixel, S.seed);
        const float scwIn = S.inScw[pixel];
        const int countIn = (int)S.inColor[4 * (size_t)pixel + 3];
        const float w = scwIn / (float)countIn;
        unsigned nsamp;
        if (w == 0) {
            nsamp = S.sampleCountMin;
        } else {
            const float nw = um_saturate((w - S.extremaX) / (S.extremaY - S.extremaX));
            const float lo = (float)S.sampleCountMin, hi = (float)S.sampleCountMax;
            nsamp = (unsigned)__builtin_rintf(lo + nw * (hi - lo));
        }
        out.sampleCount = (int32_t)nsamp;

        const bool brightest = A.select == RTOW_PATH_SELECT_BRIGHTEST;
        if (brightest ? nsamp == 0u : (unsigned)A.sampleIndex >= nsamp) {
            out.flags = 2u;      // no such sample
        } else {
            // INDEX: samples 0 .. k* - 1 only move the generator.  BRIGHTEST: all of them are run and ranked, then the generator goes back to where the winner started
            Rng<NOISE> bestStart = rng;
            unsigned k = 0u, bestK = 0u;
            float bestLum = 0.0f;
            bool bestNan = false, replay = false;
            SampleResult R;
            for (;;) {
                const bool record = brightest ? replay : k == (unsigned)A.sampleIndex;
                const Rng<NOISE> start = rng;
                R = run_sample<BASE, NOISE>(A, at, rng, cx, cy, stack, hist, record ? seg : nullptr);
                if (record) break;
                if (brightest) {
                    const bool isNan = R.color.x != R.color.x || R.color.y != R.color.y || R.color.z != R.color.z;
                    const float lum = path_luminance(R.color);      // a failed sample's colour is 0
                    const bool better = k == 0u || (isNan && !bestNan) || (!isNan && !bestNan && lum > bestLum);
                    if (better) { bestK = k; bestLum = lum; bestNan = isNan; bestStart = start; }
                }
                k++;
                if (brightest && k == nsamp) { rng = bestStart; k = bestK; replay = true; }
            }
            out.sampleIndex = (int32_t)k;
            out.segmentCount = R.rays;
            out.flags = R.ok ? 1u : 0u;
            out.time = R.time;
            out.luminance = path_luminance(R.color);
            out.randomEvents = R.randomEvents;
            out.color = f3(R.color); out.normal = f3(R.normal); out.albedo = f3(R.albedo);
            written = R.rays;
        }
    }
    if (seg) {
        // DebugPaths[i] = default (:98-100) for the depths the sample did not reach - and for the attenuation / emission fields an unrecorded sample left there
        RtowPathSegment zero;
        zero.from = f3(v3(0, 0, 0)); zero.distance = 0.0f;
        zero.direction = f3(v3(0, 0, 0)); zero.entityIndex = 0;
        zero.to = f3(v3(0, 0, 0)); zero.info = 0u;
        zero.normal = f3(v3(0, 0, 0)); zero.randomEvents = 0.0f;
        zero.attenuation = f3(v3(0, 0, 0)); zero.pad0 = 0.0f;
        zero.emission = f3(v3(0, 0, 0)); zero.pad1 = 0.0f;
        for (int d = written; d < traceDepth; d++) seg[d] = zero;
    }
    A.summaries[index] = out;
}

template <int NOISE>
hipError_t launch(const RecordArgs& A, unsigned long long blocks, hipStream_t stream)
{
    return launch_query(A.S.layout, blocks, [&](auto base, dim3 grid, dim3 block) { hipLaunchKernelGGL((record_paths_kernel<decltype(base)::value, NOISE>), grid, block, 0, stream, A); });
}

}  // namespace

hipError_t launchRecordPaths(const SampleKernelArgs& batch, const QueryScene& scene, const RtowRecordPathsParams& params, const uint32_t* words, uint32_t capacity,
                             RtowPathSummary* summaries, RtowPathSegment* segments, float* stackRows, hipStream_t stream)
{
    if (capacity == 0u) return hipSuccess;
    if (!segments && !stackRows) return hipErrorInvalidValue;
    RecordArgs A{};
    A.S = batch;
    A.S.tex = scene.tex;      // (a batch's own launch is handed the blob whatever the scene; the queries' is null without an Image texture)
    A.entityOfPrim = scene.binding.entityOfPrim;
    A.imageCount = image_count(scene.tex.layout);
    A.words = words;
    A.capacity = capacity;
    A.select = params.select;
    A.sampleIndex = params.sampleIndex;
    A.summaries = summaries;
    A.segments = segments;
    A.stackRows = stackRows;
    const unsigned long long blocks = ((unsigned long long)capacity + kTraceBlock - 1) / kTraceBlock;
    if (batch.noiseColor == RTOW_NOISE_BLUE) return launch<RTOW_NOISE_BLUE>(A, blocks, stream);
    if (batch.noiseColor == RTOW_NOISE_SPATIOTEMPORAL_BLUE) return launch<RTOW_NOISE_SPATIOTEMPORAL_BLUE>(A, blocks, stream);
    return launch<RTOW_NOISE_WHITE>(A, blocks, stream);
}

}  // namespace rtow
