// Test-only C wrapper around the 80-byte LDS node image of the sign-ordered box walk (csrc/rtow_kernels.h: node_image, node_planes_ordered, planLds with its
// nodeImage argument) and the scene compiler, so that the CPU suite can hold the image to its layout without a GPU.  Built by tests/test_node_image.py (host only).
#include <cstring>
#include <string>

#include "../../raytracing-in-one-weekend_amd/csrc/rtow_kernels.h"

extern "C" int shim_compile_scene(const RtowSceneDesc* desc, int maxDepth, uint8_t* blobOut, uint32_t blobCapacity, rtow::SceneLayout* layoutOut)
{
    rtow::CompiledScene cs;
    std::string err;
    const int rc = rtow::compileScene(desc, maxDepth, &cs, &err);
    if (rc != RTOW_SUCCESS) return rc;
    *layoutOut = cs.layout;
    if (cs.blob.size() > blobCapacity) return -1;
    memcpy(blobOut, cs.blob.data(), cs.blob.size());
    return 0;
}

// the image of `count` 64-byte nodes, as the kernel expands it while it stages the scene: 80 bytes per node
extern "C" void shim_node_image(const uint32_t* nodes, uint32_t count, uint32_t* image)
{
    for (uint32_t i = 0; i < count; i++) rtow::node_image(nodes + 16u * i, image + 20u * i);
}

extern "C" int shim_planes_ordered(const uint8_t* nodes, uint32_t count, int twoChildren)
{
    return rtow::node_planes_ordered(reinterpret_cast<const rtow::GpuNode*>(nodes), count, twoChildren != 0) ? 1 : 0;
}

extern "C" int shim_plan_lds(int wide, uint32_t bvhDepth, uint32_t totalBytes, uint32_t nodeCount, uint32_t histRows, uint32_t budgetOverride, int nodeImage, uint32_t* out /* [9] */)
{
    rtow::SceneLayout L{};
    L.bvhDepth = bvhDepth; L.totalBytes = totalBytes; L.nodeCount = nodeCount;
    const rtow::LdsPlan p = rtow::planLds(wide != 0, L, histRows, budgetOverride, nodeImage != 0);
    out[0] = p.stackRows; out[1] = p.histOffset; out[2] = p.histRows; out[3] = p.frontBytes; out[4] = p.sceneBytes; out[5] = p.nodeCount; out[6] = p.allLds ? 1u : 0u; out[7] = p.histSpillRows;
    out[8] = p.nodeImageBytes;
    return 0;
}

extern "C" int shim_constants(uint32_t* out /* [5] */)
{
    out[0] = (uint32_t)rtow::kLdsBytesMax; out[1] = (uint32_t)rtow::kQueueBytes; out[2] = rtow::kNodeImageBytes; out[3] = rtow::kNodeImageFlag; out[4] = (uint32_t)sizeof(rtow::GpuNode);
    return 0;
}

// the slice a launch runs with (schedulerTune[8] confined to 1 .. 65 535) and what the launcher of a variant with the sign-ordered walk hands its kernel
extern "C" int shim_trav_slice(int requested) { return rtow::travSliceOf(requested); }
extern "C" int shim_trav_slice_for_image(int slice, int imageGranted) { return rtow::travSliceForImage(slice, imageGranted != 0); }
