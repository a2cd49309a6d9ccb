// Test-only C wrapper around the product's host-side interval probe (csrc/rtow_probe.hip: probeIntervalHost, what rtowProbeNearestHitInterval runs; both modes) and its
// (0, +inf) predecessor probeNearestHitHost, over the product's own scene compiler, so that the CPU suite can hold the interval walk to the brute-force reference
// (tests/trace_interval_reference.py) without a GPU.
// The derived inverse transforms of rotated / translated entities are computed on the device at upload (csrc/rtow_kernels.hip: prepare_entities_kernel) and copied back
// into the host image; without a device this file derives them with the same expressions on the same helpers (rotate of csrc/rtow_vecmath.hip.h), so that a general scene
// made of rects, boxes and spheres (coplanar) has a complete host image here too - tests/test_gpu_trace_interval.py holds the device's own image to the same reference.
// Built by tests/test_interval_walk_host.py: this file and rtow_probe.hip with hipcc --offload-host-only (the vector helpers are HIP headers), the rest with g++.
#include <cstring>
#include <string>

#include "../../raytracing-in-one-weekend_amd/csrc/rtow_kernels.h"
#include "../../raytracing-in-one-weekend_amd/csrc/rtow_vecmath.hip.h"

static rtow::CompiledScene g_scene;

// prepare_entities_kernel, one primitive after the other: InverseTransform = inverse(OriginTransform) (RT/Entity.cs:51-52)
static void prepare_entities_host(uint8_t* blob, const rtow::SceneLayout& L)
{
    using namespace rtow;
    for (unsigned i = 0; i < L.sphereCount; i++) {
        const unsigned type = reinterpret_cast<const unsigned*>(blob + L.matIndexOffset)[i] >> kPrimTypeShift;
        if (type == RTOW_ENTITY_TRIANGLE) continue;
        float4* p = reinterpret_cast<float4*>(blob + L.primOffset + (size_t)i * 128u);
        const float4 q = p[0];
        const float r = 1.0f / (q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
        const float4 inv = make_float4(r * q.x * -1.0f, r * q.y * -1.0f, r * q.z * -1.0f, r * q.w * 1.0f);
        p[1] = inv;
        const float4 q2 = p[2];
        const V3 it = rotate(inv, v3(-q2.x, -q2.y, -q2.z));
        float4 q4 = p[4];
        q4.y = it.x; q4.z = it.y; q4.w = it.z;
        p[4] = q4;
    }
}

extern "C" int shim_interval_compile(const RtowSceneDesc* desc)
{
    std::string err;
    const int rc = rtow::compileScene(desc, RTOW_DEFAULT_MAX_BVH_DEPTH, &g_scene, &err);
    if (rc != RTOW_SUCCESS) return -rc;
    if (g_scene.layout.sceneKind >= rtow::SCENE_KIND_GENERAL && g_scene.entityCount > 0) prepare_entities_host(g_scene.blob.data(), g_scene.layout);
    return (int)g_scene.layout.sceneKind;
}

// 1: the scene compiler found one TimeRange on every moving entity and the walk maps the ray time once (csrc/rtow_walk.hip.h); 0: sphere_at clamps per test
extern "C" int shim_interval_common_time_range() { return (int)g_scene.layout.commonTimeRange; }

static const int32_t* entity_map() { return g_scene.entityOfPrim.empty() ? nullptr : g_scene.entityOfPrim.data(); }

extern "C" int shim_interval_probe(const float* origin, const float* direction, float time, float tMin, float tMax, int any, float* distance, int* entity)
{
    return rtow::probeIntervalHost(g_scene.blob.data(), g_scene.layout, entity_map(), origin, direction, time, tMin, tMax, any != 0, distance, entity) ? 1 : 0;
}

extern "C" int shim_nearest_probe(const float* origin, const float* direction, float time, float* distance, int* entity)
{
    return rtow::probeNearestHitHost(g_scene.blob.data(), g_scene.layout, entity_map(), origin, direction, time, distance, entity) ? 1 : 0;
}
