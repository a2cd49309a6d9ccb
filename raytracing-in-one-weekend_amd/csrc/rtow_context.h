// rtow_context.h - the context behind RtowContext and the helpers every translation unit of the C-ABI layer shares (rtow_api.hip, rtow_api_query.hip, rtow_api_post.hip,
// rtow_comm.hip): logging, the error-return macros, what an entry point does once it holds its lock and the resident scene as a query launch gets it (queryScene).  Internal: nothing here is part of include/rtow.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <vector>

#include "../../include/rtow.h"
#include "rtow_bvh.h"
#include "rtow_device_mem.h"
#include "rtow_kernels.h"
#include "rtow_launch_cache.h"

// The tuning default the context's member initialisers need (RTOW_DEFAULT_REGROUP_SIDE is with the knob it belongs to, rtow_launch_cache.h); the other tuning macros, and
// what the nine thresholds mean, are at the top of rtow_api.hip.
#ifndef RTOW_DEFAULT_TUNE
#define RTOW_DEFAULT_TUNE 24, 32, 1, 32, 28, 1, 3, 1, 16
#endif

struct RtowContext_t {
    template <typename T> using DeviceMem = rtow::DeviceMem<T>;   // every d* member the context allocates: it owns its block, knows its size in bytes, frees it when the context is deleted
    int device = 0;
    int cuCount = 0;
    RtowLogCallback logCb = nullptr;
    void* logData = nullptr;
    int logLevel = 0;

    hipStream_t stream = nullptr;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    hipEvent_t evBatchDone = nullptr;   // end of everything the last sample batch enqueued (kernel + chunk-order refresh)
    bool haveBatchDone = false;
    bool haveTiming = false;

    // scene
    bool haveScene = false;
    rtow::CompiledScene scene;
    DeviceMem<uint8_t> dScene;
    DeviceMem<int32_t> dEntityOfPrim;     // device copy of scene.entityOfPrim for rtowTraceRaysDevice / rtowTraceViewDevice (read only while scene.entityOfPrim is not empty)
    DeviceMem<int32_t> dPrimOfEntity;     // its inverse for rtowShadeHitsDevice: entity -> primitive, -1 for an entity without one; sized by the entity count, allocated under the same
                                          // condition, released and allocated at its exact size at every upload
    int32_t primOfEntityCount = 0;        // entries of dPrimOfEntity: what rtowShadeHitsDevice bounds an entity index by, whatever an upload that failed half way left in `scene`
    uint32_t ldsSceneBytes = 0, ldsNodeCount = 0;
    DeviceMem<unsigned short> dHistSpill; // path-history rows that do not fit LDS (LdsPlan.histSpillRows), [row][workgroup x 1024 + lane]
    rtow::LdsPlan ldsPlan{};              // of launches whose variant keeps its whole path history in registers (trace depth <= 16); the others plan per launch (launchSample)

    // work distribution / cancellation
    DeviceMem<unsigned int> dWorkCounter;
    DeviceMem<unsigned int> dChunkDone;   // chained batches: pixels stored per chunk (grows with dXcdState)
    DeviceMem<uint8_t> dXcdState;         // chained batches: XcdState + kMaxXcds lists of one entry per chunk (which XCD owns which chunk)
    DeviceMem<rtow::ChainBatch> dChainBatches;   // chained batches: per-batch seed / diagnostics table of the launch being enqueued
    // chunk cost map -> launch order (longest chunks first), and the ticket map: valid for one ChunkOrderKey (scene upload, frame and slice, groups per pixel, mapped or not)
    struct ChunkOrder {
        DeviceMem<unsigned int> dChunkCost, dChunkOrder;   // these four grow together (prepareChunkOrder)
        DeviceMem<unsigned short> dPixelCost;
        DeviceMem<unsigned int> dTicketMap;   // ticket -> owned pixel (SampleKernelArgs.ticketMap), 64 entries per chunk; re-sorted from every launch's cost map
        rtow::Keyed<rtow::ChunkOrderKey> key; // what the cost map / order on hand were recorded under
    } chunkOrder;
    rtow::PinnedBlock pinned;             // the 256 bytes behind the next three
    volatile uint32_t* hCancel = nullptr; // pinned, device-visible: [0] cancel, [1] hit-list overflow, [2] tie-list overflow; the metrics record of rtowReduceMetricsDevice at byte 64
    volatile RtowMetrics* hMetricsRecord = nullptr;
    RtowMetrics* dMetricsRecord = nullptr;
    // RTOW_RNG_PER_SAMPLE: one 64-byte record per (owned pixel, sample group) unit
    DeviceMem<float> dUnitRecords;
    // RTOW_CONTEXT_REFERENCE_DIAGNOSTICS: the reference's own tree of the current scene (CompiledScene.refTree), HBM only
    DeviceMem<uint8_t> dRefTree;
    // hit lists beyond the 24 entries a lane holds itself (volume scenes, exact-tie kernels): [entry][lane] columns, grow-only
    DeviceMem<uint4> dHitSpill;
    uint32_t hitSpillEntries = 0;         // of the current scene (the block may hold more)
    uint32_t hitListCapacity = 0;         // RtowContextOptions.hitListCapacity (0 = default)
    uint32_t grownListCapacity = 0;       // hitListCapacity == 0 only: what the capacity has grown to after batches that met longer lists (growHitList); kept across scenes
    bool triWatchOff = false;             // this all-triangle scene ties too often for the tie watch (a watched launch marked thousands of pixels, or more than the list holds): exact-tie kernels from now on
    bool overflowGrew = false;            // the last reported overflow enlarged the capacity: the same batch, issued again, has room
    // Image-texture blob of the current scene (CompiledScene.texBlob), HBM only
    DeviceMem<uint8_t> dTexBlob;
    // noise texture sets (rtowUploadBlueNoise / rtowUploadStbNoise): device copies, `textureCount` textures back to back
    DeviceMem<uint8_t> dBlueNoise;
    uint32_t blueRowStride = 0, blueTextureCount = 0;
    DeviceMem<uint8_t> dStbNoise;        // scalar | vector2 | cosineUnitVector3 | unitVector2 | unitVector3 sets, in this order
    uint32_t stbRowStride = 0, stbTextureCount = 0;
    // sky cubemap (rtowUploadSkyCubemap)
    DeviceMem<uint8_t> dCubemap;
    RtowCubemapDesc cubemap{};   // .faces is not kept (host pointer): dCubemap holds the copy, null when none
    uint64_t sceneSerial = 0;             // counts the uploads that succeeded: what both cache keys name the scene by
    // camera-ray candidate lists (primary_candidates_kernel): valid for one CameraListKey (scene upload, view, frame and slice, the float Size the beams divide by, jitter, pruning)
    struct CameraLists {
        DeviceMem<uint2> dLists;
        rtow::Keyed<rtow::CameraListKey> key;
        uint32_t ownedPixels = 0;             // owned pixels the lists were built for
        DeviceMem<unsigned long long> dStats; // rtowGetCameraRayListStats: ten counters, allocated on first use
    } cameraLists;

    // grow-only staging for rtowSampleBatch (host buffers) - like CudaBuffer.EnsureCapacity (OptixApi.cs:240-251)
    DeviceMem<float> dColor, dNormal, dAlbedo, dScw;   // (grow together)
    DeviceMem<uint8_t> dDiag;

    DeviceMem<rtow::MetricsPartial> dPartials;
    DeviceMem<RtowFloat2> dExtremaPartials;   // [kMetricsBlocks] rtowSampleBatchChainAdaptiveDevice: partials of the per-batch weight-extrema reduction
    DeviceMem<unsigned> dExtremaKeys;         // [2 x kMaxChain] ... of a fused launch: every batch's (min, max) folded at store time

    // nearest-hit ties of the rank-rule sphere kernels (SampleKernelArgs.tieBits / tieRedo): the bitmap the fast kernel marks, the list the fix-up launch renders, a copy
    // of the inputs of launches that accumulate in place, and the fix-up launch's own (small) hit-list spill area
    DeviceMem<unsigned> dTieRedo;
    DeviceMem<unsigned> dTieBits;
    DeviceMem<float> dTieInputs;          // colour | normal | albedo | weight of the frame's pixels
    DeviceMem<uint4> dRedoSpill;
    uint32_t redoSpillEntries = 0;        // entries of the current plan (prepareTieWatch; the block may hold more)
    // rtowSamplePixelsDevice: the context's own copy of the caller's list (4 + capacity words, entries beyond the frame dropped) with the filter's scan scratch, and the
    // hit-list spill area of a list launch's workgroups.  Not dTieRedo / dRedoSpill: those belong to watched launches in flight
    DeviceMem<unsigned> dPixelList;       // (a capacity of 0 is a valid list: the four header words - so the block's bytes tell a list that is there from none)
    DeviceMem<unsigned> dPixelListScratch;
    DeviceMem<uint4> dListSpill;
    // rtowRecordPathsDevice without `segments`: the lanes' emission / attenuation stacks (capacity x traceDepth x 24 bytes), allocated on first use
    DeviceMem<float> dPathStack;

    // RtowContextOptions: behaviour switches and development knobs (nothing is read from the environment)
    bool wideCodes = false;               // current scene: more than 65 535 entities or tree nodes (32-bit candidate / stack codes, tree read from HBM)
    uint32_t flags = 0;
    uint32_t ldsSceneBudget = 0;          // 0 = everything that fits
    int tune[9] = {RTOW_DEFAULT_TUNE};
    bool userTune = false;                // RtowContextOptions.schedulerTune was given: no per-scene adjustment
    rtow::SchedulerKnob knob{};           // RtowContextOptions.schedulerTune[7] (see RTOW_DEFAULT_REGROUP_SIDE), decoded by rtowCreateContext
    bool userSliceDefault = false;        // ... with a zero walk slice: the per-scene built-in value
    bool chainFusion = true;              // the same-XCD hand-over litmus passed on this device (rtowCreateContext): chains may run as one launch
    // per-scene measurement of the stage thresholds (measureThresholds): everything but the winner cache is of the current scene, and dropThresholdTuning starts it over
    struct ThresholdTuning {
        enum State { Unmeasured, Pending, Settled };
        State state = Unmeasured;             // Pending: probes are enqueued, their events are read by a later call, never waited for; Settled: measured, taken from the
                                              // winner cache, or not measurable - no further probes for this scene
        int winner = -1;                      // Settled: which candidate's thresholds run (-1: the kernel kind's built-in ones)
        int candidates = 0, builtin = 0;      // Pending: how many candidates the probes time, and which of them the kernel kind runs unmeasured
        std::vector<hipEvent_t> events;
        DeviceMem<uint32_t> dProbeSink;       // where probes report rays beyond the hit-list capacity (not the batch's flag)
        uint64_t sppSinceUpload = 0;          // samples per pixel this scene has been asked for since its upload: a measurement must be worth its probes
        uint64_t signature = 0;               // of the current scene (sceneSignature)
        struct Winner { uint64_t signature; int winner; };
        std::vector<Winner> cache;            // winners by scene signature: a re-upload of a like scene does not measure again
    } tuning;

    // rtowRegisterHostBuffer: pinned + device-mapped ranges of caller memory
    struct HostRange { uint8_t* base; size_t size; uint8_t* device; };
    std::vector<HostRange> hostRanges;

    // rtowComm*: RCCL communicator of this rank (one process per GPU) and the packed-row staging of rtowGatherRowsDevice
    void* comm = nullptr;                 // ncclComm_t
    int commRank = 0, commWorld = 1;
    DeviceMem<float> dGatherSend, dGatherRecv;
    DeviceMem<float> dByteThresholds;     // FinalizeTexturesJob's float -> byte step table (rtow_finalize.hip.h), built when the context is created
    hipEvent_t evGatherDone = nullptr;    // end of the last gather: the staging blocks are per context, gathers may come on different streams
    bool haveGatherDone = false;
    hipEvent_t evMetricsDone = nullptr;   // end of the last metrics reduction (the per-block partials are per context)
    bool haveMetricsDone = false;

    std::mutex mu;
    std::mutex sceneMu;      // guards the HOST image of the scene (scene.blob / layout / entityOfPrim, haveScene) between rtowUploadScene and rtowProbeNearestHit; taken after mu, never the other way round

    ~RtowContext_t()      // rtowDestroyContext has set the device, waited for the stream and destroyed the communicator; the blocks above free themselves after this
    {
        for (hipEvent_t e : {evStart, evStop, evBatchDone, evGatherDone, evMetricsDone}) if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace rtow {

inline void logf(RtowContext ctx, int level, const char* tag, const char* fmt, ...)
{
    if (!ctx || !ctx->logCb || level > ctx->logLevel) return;
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    ctx->logCb(level, tag, buf, ctx->logData);
}

#define HIP_TRY(ctx, expr, result)                                                                    \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            logf(ctx, 2, "hip", "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return (result);                                                                          \
        }                                                                                             \
    } while (0)

#define RTOW_TRY(expr)                                                                                \
    do {                                                                                              \
        const int _rc = (expr);                                                                       \
        if (_rc != RTOW_SUCCESS) return _rc;                                                          \
    } while (0)

// DeviceBlock::ensureAll with the context's log line and error code: blocks that grow together in one call, `grew` as there
inline int growDevice(RtowContext ctx, std::initializer_list<DeviceBlock::Need> needs, bool* grew = nullptr)
{
    HIP_TRY(ctx, DeviceBlock::ensureAll(needs, grew), RTOW_ERROR_MEMORY_ALLOCATION);
    return RTOW_SUCCESS;
}

// What the entry points do once they hold their lock: this thread on the context's device (calls come from a different worker thread each time) and the stream the work
// goes to (null: the context's)
inline int useDevice(RtowContext ctx, void* stream, hipStream_t* s)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    *s = stream ? (hipStream_t)stream : ctx->stream;
    return RTOW_SUCCESS;
}

// primitive -> the host's entity index (all-triangle scenes number their primitives in leaf order), on the device and on the host; null: the same number
inline const int32_t* entityMapDevice(const RtowContext_t* ctx) { return ctx->scene.entityOfPrim.empty() ? nullptr : ctx->dEntityOfPrim.get(); }
inline const int32_t* entityMapHost(const RtowContext_t* ctx) { return ctx->scene.entityOfPrim.empty() ? nullptr : ctx->scene.entityOfPrim.data(); }

// The resident scene for a query launch (QueryScene, rtow_kernels.h); the caller holds ctx->mu.  The two rules every query shares are here: a scene without an Image
// texture has no texture blob, and an entity index is never bounded beyond the inverse map that is on the device
inline QueryScene queryScene(const RtowContext_t* ctx)
{
    const bool mapped = !ctx->scene.entityOfPrim.empty();
    QueryScene q{};
    q.binding.blob = ctx->dScene;
    q.binding.entityOfPrim = entityMapDevice(ctx);
    q.binding.layout = ctx->scene.layout;
    q.tex.blob = ctx->scene.texLayout.totalBytes ? ctx->dTexBlob.get() : nullptr;
    q.tex.layout = ctx->scene.texLayout;
    q.primOfEntity = mapped ? ctx->dPrimOfEntity.get() : nullptr;
    q.entityCount = mapped ? std::min(ctx->scene.entityCount, ctx->primOfEntityCount) : ctx->scene.entityCount;
    q.cubemapData = ctx->dCubemap;
    q.cubemap = ctx->cubemap;
    return q;
}

// device-visible address of caller memory [p, p + bytes) if it lies inside a range given to rtowRegisterHostBuffer, else null
inline uint8_t* mappedHost(RtowContext ctx, const void* p, size_t bytes)
{
    const uint8_t* q = (const uint8_t*)p;
    for (const RtowContext_t::HostRange& r : ctx->hostRanges)
        if (q >= r.base && q + bytes <= r.base + r.size) return r.device + (q - r.base);
    return nullptr;
}

// rtow_comm.hip, for rtowDestroyContext: destroys the communicator (before the context's packed-row staging goes)
void releaseComm(RtowContext ctx);

} // namespace rtow
