// rtow_api.hip - implementation of the C ABI declared in include/rtow.h (librtow_hip.so).
//
// Host-side runtime of the path: context / device selection, scene compilation + upload, grow-only device staging
// for the host-buffer entry point, kernel launch on a HIP stream with HIP-event timing, cooperative cancellation,
// and rtowRecordPathsDevice, the one query the batch planner feeds.  There is no CPU implementation behind any entry point: without a usable HIP device
// rtowCreateContext fails with RTOW_ERROR_NO_DEVICE and nothing else can be called.  The multi-GPU entry points (rtowComm*, rtowGatherRowsDevice,
// rtowHybridPlan, rtowExchangeAccumDevice) are in rtow_comm.hip, the post passes in rtow_api_post.hip, the probes, the trace, shade and guide calls in
// rtow_api_query.hip; the context itself - and queryScene, the resident scene as a query launch gets it - is rtow_context.h, what
// an entry point refuses before it takes its lock is rtow_validate.h, and what the caches a context keeps between launches are valid for is rtow_launch_cache.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rtow.h"
#include "rtow_context.h"

// minimum lane population per stage, in 64ths of the wave's live lanes: REGEN TRAV TEST HIT SKY VOL | candidates that end a walk (hand-over to TEST) | unused | box-walk slice (node visits per trip).
// Sphere kinds: REGEN from 3/8, the walk and HIT from 1/2, SKY from 7/16, TEST at once.  Since a chunk's 64 tickets are an 8 x 8 tile of the image
// (rtow_kernels.h) the lanes of a wave meet the same few materials, and a HIT stage that waits for half of them runs its class bodies a third as
// often with three times the lanes; with 64 x 1 strips any threshold on HIT lost (rounds 1 / 2).  Same box, alternating runs, gpurun_out/r03am-r03ao:
// cover 9 417 against 8 685 Msamples/s (+8.4 %), 10 000 spheres 7 513 against 7 042 (+6.7 %), moving + defocus 6 306 against 5 958 (+5.8 %),
// 4K / 1024 spp / 16 bounces 9 464 against 8 851 (+6.9 %).  The general-entity kinds keep REGEN 1/4, walk 3/4, HIT and SKY at once (kGeneralTune):
// on the 250 k-triangle mesh HIT from 1/2 loses 6 % (1 732 against 1 840), SKY from 1/2 3 %.
#ifndef RTOW_GROUP_SLOT_BLOCK
#define RTOW_GROUP_SLOT_BLOCK 4     // (chunk, batch) slots a wave reserves at a time in a batch group (SampleKernelArgs.slotBlock): groups + fold 9 978 -> 10 160 Msamples/s at 4, 10 118 at 2
#endif
static constexpr unsigned kGroupSlotBlock = RTOW_GROUP_SLOT_BLOCK;
#ifndef RTOW_PIXEL_GATE
#define RTOW_PIXEL_GATE 1     // lanes of a wave that must want a pixel boundary before the boundary block runs (1 = at once; the kernel's A.tune[7]); measured: see HISTORY.md round 6
#endif
#ifndef RTOW_URGENT_RAYS_PER_SAMPLE
// lanes in a hurry (kernel: HURRY): the rate - rays per sample done so far - beyond which a pixel's lane stops waiting for company.  Same box (profiles/r06x_lanes_in_a_hurry.json,
// run_r06ag.sh / run_r06ah.sh): cover scene at depth 32, chains: 14 -> 7 126 Msamples/s, 18 -> 7 302, 24 -> 6 220 (nobody is in a hurry any more); 10 000 spheres at depth 32:
// 14 -> 5 370, 18 -> 4 895, 24 -> 4 180.  (Float bits with the low eight zero: they share tune[7] with the pixel gate.)
#define RTOW_URGENT_RAYS_PER_SAMPLE 18.0f
#define RTOW_URGENT_RAYS_PER_SAMPLE_BEYOND_LDS 14.0f
#endif
#ifndef RTOW_GENERAL_TUNE
#define RTOW_GENERAL_TUNE 16, 48, 1, 1, 1, 1, 3, 1, 16
#endif
// A second general family - REGEN and SKY from 1/8 - is what the 250 k-triangle mesh wants (2 167 against 2 037 Msamples/s) and the Cornell box with
// volumes does not (840 against 920; mixed primitives +0.7 %; gpurun_out/r03bv): a third candidate for the per-scene measurement below.
#ifndef RTOW_GENERAL_TUNE_2
#define RTOW_GENERAL_TUNE_2 8, 48, 1, 1, 8, 1, 3, 1, 16
#endif
// Which of the two families suits a scene is a property of the scene, not of its kernel kind: an image-textured scene of spheres runs 25 % faster
// on the sphere kinds' thresholds (10 160 against 8 100 Msamples/s), a scene of rects, boxes and triangles 9 % slower (3 220 against 3 540), a mesh with
// fog volumes 15 % faster when the volume stage too waits for half of the live lanes (460 against 399; gpurun_out/r03ax).  So the first batch after
// rtowUploadScene MEASURES them: each candidate (three families; six for volume scenes) renders kTuneProbeSamples samples per pixel through the batch's own kernel (a probe:
// nothing is stored), twice, timed with events on the batch's stream; the fastest one stays for the scene.  A probe of a few samples per pixel ranks the
// candidates like the full workload does (cover, textured, mixed, volumes, 10 000 spheres at 2 / 4 / 8 / 64 samples per pixel: same order every
// time, gpurun_out/r03ay).  Thresholds never change a result (tests/test_gpu_fullsize.py: frames under every schedule).  The call that tunes
// waits for its probes (a few milliseconds to ~0.1 s, once per scene); RTOW_CONTEXT_NO_THRESHOLD_TUNING keeps the per-kind values above.
constexpr int kTuneProbeSamples = 4, kTuneProbeRepeats = 3;
constexpr uint64_t kTuneMinSamplesPerPixel = 64;    // ... and the scene must have been asked for this many samples per pixel since its upload before it is worth 40 - 76 of probes
constexpr float kTuneMargin = 0.98f;      // a candidate replaces the kind's built-in family only if its best probe is more than 2 % faster: single probes (1 - 10 ms)
                                          // scatter by a few per cent, and a wrong pick costs more than a missed one (10 000 spheres: family 2 picked once in r03bw, -7 %)
// The families above, by candidate number: candidate c of a measurement is family c % kFamilies, with the volume stage from half of the live lanes for c >= kFamilies
// (the ninth value, the walk slice, is set by rtowUploadScene)
constexpr int kFamilies = 3;
constexpr int kThresholdFamilies[kFamilies][9] = {{RTOW_DEFAULT_TUNE}, {RTOW_GENERAL_TUNE}, {RTOW_GENERAL_TUNE_2}};
static void candidateThresholds(int candidate, int* tune, int count)
{
    for (int k = 0; k < count; k++) tune[k] = kThresholdFamilies[candidate % kFamilies][k];
    if (candidate >= kFamilies) tune[5] = 32;
}

using namespace rtow;


namespace {

int ownedRows(const RtowSampleParams* p)
{
    const int h = (int)p->size.y;
    if (p->sliceOffset >= h) return 0;
    return (h - p->sliceOffset + p->sliceDivider - 1) / p->sliceDivider;
}

// chain (optional): {count, seeds[count], diagnostics[count]} - `count` successive batches of the frame in this one launch (seeds[0] / diags[0] are
// batch 0's; p->seed and diag are ignored then)
// outs (optional): a batch group - batch b stores to outs[b] and every batch reads `in` (rtowSampleBatchGroupDevice); null: a chain, batch b reads what b - 1 stored to `out`
// extrema / extremaKeys (optional, chains only): per batch where it reads SampleCountWeightExtrema (null = p's), and the [2 x count] keys its stores fold the batch's extrema into
struct ChainSpec { int count; const uint32_t* seeds; void* const* diags; const RtowAccumBuffers* outs; const RtowFloat2* const* extrema = nullptr; unsigned* extremaKeys = nullptr; };

// per-scene threshold measurement (launchSample): forget the scene's measurement, in flight or settled (new scene, context going away; a measurement that ends settles after it)
void dropThresholdTuning(RtowContext ctx)
{
    RtowContext_t::ThresholdTuning& t = ctx->tuning;
    for (auto& e : t.events) if (e) (void)hipEventDestroy(e);
    t.events.clear();
    t.state = t.Unmeasured;
    t.winner = -1;
}

// ... and settle it: `winner`'s thresholds (-1: the kernel kind's built-in ones) run until the next upload, nothing is measured again
void settleThresholdTuning(RtowContext ctx, int winner)
{
    dropThresholdTuning(ctx);
    ctx->tuning.state = ctx->tuning.Settled;
    ctx->tuning.winner = winner;
}

// Which scenes get the same thresholds without being measured again: a host that re-uploads on every scene edit (sceneSerial moves) keeps what was
// measured for a scene of the same kernel kind and size.
uint64_t sceneSignature(const CompiledScene& sc, bool wide)
{
    return ((uint64_t)sc.layout.sceneKind << 60) ^ ((uint64_t)(sc.layout.exactTies ? 1 : 0) << 59) ^ ((uint64_t)(wide ? 1 : 0) << 58) ^ ((uint64_t)sc.layout.nodeCount << 29) ^
           (uint64_t)(uint32_t)sc.entityCount ^ ((uint64_t)sc.layout.materialCount << 44);
}

// read the probes' events if they are all complete (wait == false: otherwise leave them for a later call) and switch to the fastest candidate; true = thresholds changed or confirmed
bool finishThresholdTuning(RtowContext ctx, bool wait)
{
    RtowContext_t::ThresholdTuning& tuning = ctx->tuning;
    if (tuning.state != tuning.Pending || tuning.events.empty()) return false;
    const hipError_t q = wait ? hipEventSynchronize(tuning.events.back()) : hipEventQuery(tuning.events.back());
    if (q == hipErrorNotReady) { (void)hipGetLastError(); return false; }
    const int candidates = tuning.candidates, builtin = tuning.builtin;
    bool ok = q == hipSuccess;
    float best = 0.0f, builtinMs = 0.0f;
    int winner = -1;
    for (int c = 0; ok && c < candidates; c++) {
        float t = 0.0f;
        for (int r = 0; r < kTuneProbeRepeats; r++) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, tuning.events[(size_t)(r * candidates + c)], tuning.events[(size_t)(r * candidates + c) + 1]) != hipSuccess) { ms = 1e30f; (void)hipGetLastError(); }
            t = (r == 0 || ms < t) ? ms : t;
        }
        if (c == builtin) builtinMs = t;
        if (winner < 0 || t < best) { best = t; winner = c; }
    }
    if (ok && winner >= 0) {
        if (winner != builtin && !(best < kTuneMargin * builtinMs)) { winner = builtin; best = builtinMs; }
        candidateThresholds(winner, ctx->tune, 8);
        tuning.cache.push_back({tuning.signature, winner});
        logf(ctx, 4, "tune", "stage thresholds measured on this scene: candidate %d of %d (%.3f ms per %d-sample probe)", winner, candidates, best, kTuneProbeSamples);
    } else {
        (void)hipGetLastError();
        winner = -1;
        logf(ctx, 2, "tune", "threshold probes failed; the per-kind values stay");
    }
    settleThresholdTuning(ctx, winner);                         // measured (or not measurable): do not try again for this scene
    return true;
}

// rtowUploadScene has put a new scene into ctx->scene (under both locks, the device idle): the one place where what the context knew of the old scene goes.  The camera-ray
// lists and the chunk order carry the serial in their keys, so moving it is all they need
void sceneReplaced(RtowContext ctx, bool wide)
{
    ctx->triWatchOff = false;
    ctx->hCancel[3] = 0u;
    ctx->sceneSerial++;
    dropThresholdTuning(ctx);
    ctx->tuning.sppSinceUpload = 0;
    ctx->tuning.signature = sceneSignature(ctx->scene, wide);
    if (ctx->userTune || (ctx->flags & RTOW_CONTEXT_NO_THRESHOLD_TUNING)) return;
    for (const RtowContext_t::ThresholdTuning::Winner& e : ctx->tuning.cache)
        if (e.signature == ctx->tuning.signature) {
            // a scene like one this context has measured before (same kernel kind, entity / node / material counts): its thresholds, no new probes
            candidateThresholds(e.winner, ctx->tune, 8);
            settleThresholdTuning(ctx, e.winner);
        }
}

uint64_t listCapacity(const RtowContext_t* ctx, bool volumes);    // (defined with growHitList below)
inline bool triangleKind(uint32_t kind) { return kind == SCENE_KIND_TRIANGLES || kind == SCENE_KIND_TRIANGLES_TEXTURED; }
constexpr unsigned kTieWatchBusy = 4096;   // a watched launch of an all-triangle scene that lists more pixel-batches than this (8 workgroups render them) sends the scene to the exact-tie kernels

// The kernel family launchSampleBatch picks for these arguments (rtow_kernels.hip; the names of the translation units): what the level-4 log says of every launch
const char* sampleKernelName(const SceneLayout& L)
{
    const bool ties = L.exactTies != 0;
    switch (L.sceneKind) {
        case SCENE_KIND_SPHERES: return ties ? "sample_spheres_ties" : "sample_spheres";
        case SCENE_KIND_SPHERES_MOTION: return ties ? "sample_spheres_motion_ties" : "sample_spheres_motion";
        case SCENE_KIND_VOLUMES: return "sample_volumes";
        case SCENE_KIND_TEXTURED: return ties ? "sample_textured_ties" : "sample_textured";
        case SCENE_KIND_VOLUMES_TEXTURED: return "sample_volumes_textured";
        case SCENE_KIND_TRIANGLES_TEXTURED: return ties ? "sample_triangles_textured_ties" : "sample_triangles_textured";
        case SCENE_KIND_TRIANGLES: return ties ? "sample_triangles_ties" : "sample_triangles";
        default: return ties ? "sample_general_ties" : "sample_general";
    }
}

// ---- launchSample, step by step ----

// The kernel's arguments from the batch's params and buffers and the context's scene, noise textures and cubemap (RTOW_ERROR_INVALID_VALUE: the noise set is not uploaded)
int buildArgs(RtowContext ctx, const RtowSampleParams* p, const RtowAccumBuffers* in, const RtowAccumBuffers* out, void* diag, bool useCancelFlag, const ChainSpec* chain,
              const RtowFloat2* extremaIn, SampleKernelArgs& a)
{
    a.inColor = in->color; a.inNormal = in->normal; a.inAlbedo = in->albedo; a.inScw = in->sampleCountWeight;
    a.outColor = out->color; a.outNormal = out->normal; a.outAlbedo = out->albedo; a.outScw = out->sampleCountWeight;
    a.diagnostics = (uint8_t*)diag;
    a.diagnosticsStride = p->diagnosticsStride;
    a.sceneBlob = ctx->dScene;
    a.layout = ctx->scene.layout;
    a.ldsSceneBytes = ctx->ldsSceneBytes;
    a.ldsNodeCount = ctx->ldsNodeCount;
    a.ldsNodeImageBytes = ctx->ldsPlan.nodeImageBytes;
    a.ldsStackRows = ctx->ldsPlan.stackRows; a.ldsHistOffset = 0u; a.ldsFrontBytes = ctx->ldsPlan.frontBytes;      // (launches of the generic variants plan again: planHistory)
    a.workCounter = ctx->dWorkCounter;
    a.cancelFlag = useCancelFlag ? ctx->hCancel : nullptr;
    a.overflowFlag = const_cast<uint32_t*>(ctx->hCancel) + 1;      // [1]: a ray beyond the hit-list capacity (grows: takeOverflow); [2]: more tied pixel-batches than the fix-up list holds (final for sphere scenes; an all-triangle scene moves to its exact-tie kernels); [3]: kTieWatchBusy
    a.width = (int)p->size.x;
    a.height = (int)p->size.y;
    a.totalWork = (uint32_t)ownedRows(p) * (uint32_t)a.width;
    a.tilesPerRow = (RTOW_TICKET_TILES && a.width % (int)kTileW == 0) ? (uint32_t)a.width / kTileW : 0u;
    a.tiledPixels = a.tilesPerRow ? ((uint32_t)ownedRows(p) / kTileH) * kTileH * (uint32_t)a.width : 0u;
    a.sizeX = p->size.x; a.sizeY = p->size.y;
    a.sliceOffset = p->sliceOffset; a.sliceDivider = p->sliceDivider;
    a.seed = chain ? chain->seeds[0] : p->seed;
    a.chainCount = chain ? (uint32_t)chain->count : 1u;
    a.chainIndependent = (chain && chain->outs) ? 1 : 0;
    // slot / chainCount = (slot * groupRecip) >> 32 for every slot of a launch (chunkCount * chainCount <= 2^25).  A count of one has no 32-bit reciprocal, and the value
    // here is not one either (__umulhi(slot, 2^32 - 1) is slot - 1): the kernel reads groupRecip only in batch groups of more than one batch, never when chainCount <= 1
    a.groupRecip = a.chainCount <= 1u ? 0xffffffffu : (uint32_t)((1ull << 32) / a.chainCount + 1ull);
    if (chain) {
        if (diag == nullptr && chain->diags) diag = chain->diags[0];
        a.diagnostics = (uint8_t*)diag;
    }
    a.view = p->view;
    a.environment = p->environment;
    a.sampleCountMin = p->sampleCountRange[0];
    a.sampleCountMax = p->sampleCountRange[1];
    a.traceDepth = p->traceDepth;
    a.subPixelJitter = p->subPixelJitter;
    a.extremaX = p->sampleCountWeightExtrema.x;
    a.extremaY = p->sampleCountWeightExtrema.y;
    a.extremaIn = extremaIn;
    a.refTree = (ctx->flags & RTOW_CONTEXT_REFERENCE_DIAGNOSTICS) ? ctx->dRefTree : nullptr;
    a.hitSpill = ctx->hitSpillEntries ? ctx->dHitSpill : nullptr;
    a.hitSpillEntries = ctx->hitSpillEntries;
    a.hitSpillStride = (uint32_t)ctx->cuCount * (uint32_t)kBlockThreads;
    a.tex.blob = ctx->dTexBlob;
    a.tex.layout = ctx->scene.texLayout;
    a.noiseColor = p->noiseColor;
    if (p->noiseColor == RTOW_NOISE_BLUE) {
        if (!ctx->dBlueNoise || p->noiseTextureIndex < 0 || (uint32_t)p->noiseTextureIndex >= ctx->blueTextureCount) return RTOW_ERROR_INVALID_VALUE;
        a.blueRowStride = ctx->blueRowStride;
        a.blueNoise = ctx->dBlueNoise + (size_t)p->noiseTextureIndex * ctx->blueRowStride * ctx->blueRowStride * 8u;
    } else if (p->noiseColor == RTOW_NOISE_SPATIOTEMPORAL_BLUE) {
        if (!ctx->dStbNoise || p->noiseTextureIndex < 0 || (uint32_t)p->noiseTextureIndex >= ctx->stbTextureCount) return RTOW_ERROR_INVALID_VALUE;
        const size_t texels = (size_t)ctx->stbRowStride * ctx->stbRowStride, all = texels * ctx->stbTextureCount, t = (size_t)p->noiseTextureIndex * texels;
        a.stbRowStride = ctx->stbRowStride;
        a.stbScalar = ctx->dStbNoise + t;                                    // 1 byte per texel
        a.stbVector2 = ctx->dStbNoise + all + t * 3;                         // RGB24
        a.stbCosineUnitVector3 = ctx->dStbNoise + all * 4 + t * 4;           // RGBA32
        a.stbUnitVector2 = ctx->dStbNoise + all * 8 + t * 3;                 // RGB24
        a.stbUnitVector3 = ctx->dStbNoise + all * 11 + t * 3;                // RGB24
    }
    a.cubemap = cubemapRefs(ctx->cubemap, ctx->dCubemap);
    return RTOW_SUCCESS;
}

// The variants for paths deeper than 16 (and the generic ones: 16-byte records, texture-driven noise, the per-sample policies beyond depth 8) keep the path-history codes
// beyond the first eight in LDS rows: this launch's LDS is planned with them, and the scene image takes what is left (a scene that no longer fits whole keeps the top of
// its tree there and reads the rest through L2, like any scene beyond LDS)
int planHistory(RtowContext ctx, const RtowSampleParams* p, SampleKernelArgs& a)
{
    const bool fullDiag = a.diagnostics && a.diagnosticsStride >= 16;
    const bool perSample = p->rngPolicy != RTOW_RNG_REFERENCE;
    int hw = historyWords(a.noiseColor, perSample, ctx->wideCodes, ctx->scene.layout.exactTies != 0, fullDiag, a.traceDepth);
    // (an all-triangle scene under the tie watch launches its rank-rule kernels first and its exact-tie kernels on the marked pixels, with the one plan: the wider of the two)
    if (ctx->scene.layout.exactTies) hw = std::max(hw, historyWords(a.noiseColor, perSample, ctx->wideCodes, false, fullDiag, a.traceDepth));
    if (hw != 32 || a.traceDepth <= kHistoryInRegisters) return RTOW_SUCCESS;
    const LdsPlan plan = planLds(ctx->wideCodes, ctx->scene.layout, (uint32_t)(a.traceDepth - kHistoryInRegisters), ctx->ldsSceneBudget);
    a.ldsStackRows = plan.stackRows; a.ldsHistOffset = plan.histOffset; a.ldsFrontBytes = plan.frontBytes; a.ldsHistRows = plan.histRows;
    a.ldsSceneBytes = plan.sceneBytes; a.ldsNodeCount = plan.nodeCount; a.ldsNodeImageBytes = plan.nodeImageBytes;      // (0: the deep-path variants keep 64-byte nodes)
    if (plan.histSpillRows) {
        // the rows that do not fit LDS (32-bit stack rows of a deep tree next to a deep trace depth; a scene kept whole in LDS): 2 bytes per lane and row in HBM
        const size_t stride = (size_t)ctx->cuCount * (size_t)kBlockThreads, need = (size_t)plan.histSpillRows * stride * sizeof(unsigned short);
        if (need > ctx->dHistSpill.bytes()) HIP_TRY(ctx, hipDeviceSynchronize(), RTOW_ERROR_LAUNCH_FAILURE);      // a batch in flight may still use the smaller area
        RTOW_TRY(growDevice(ctx, {{&ctx->dHistSpill, need}}));
        a.histSpill = ctx->dHistSpill; a.histSpillRows = plan.histSpillRows; a.histSpillStride = (uint32_t)stride;
    }
    return RTOW_SUCCESS;
}

// Scheduler thresholds (lane population a stage needs before it runs) and box-walk slice (RtowContextOptions.schedulerTune overrides); tune[7] = pixel gate | hurry rate
void setSchedulerValues(const RtowContext_t* ctx, const RtowSampleParams* p, SampleKernelArgs& a)
{
    for (int i = 0; i < 8; i++) a.tune[i] = ctx->tune[i] < 1 ? 1 : ctx->tune[i];
    a.travSlice = travSliceOf(ctx->tune[8]);      // 1 .. 65 535: bit 16 belongs to the launcher (kNodeImageFlag)
    // Lanes that wait for company at a pixel boundary (kernel: A.tune[7]; schedulerTune[7] bits 12 .. 15 override).  Measured (profiles/r06d_pixel_boundaries_in_company.json):
    // worth it only where boundaries are frequent - the reference host's 50 samples per batch: groups +2.5 % with 3 - 4 lanes, the per-sample policies' 16-sample units +1.6 % -
    // (the adaptive {1, 50} schedule +0.5 ... 1 %) and a loss of 1 - 3 % where a pixel takes hundreds of samples (the wait costs more than the shared instructions save):
    // so by the samples a unit of work takes at most
    const unsigned unitSamples = p->rngPolicy != RTOW_RNG_REFERENCE ? kSampleGroup : (a.sampleCountMax > a.sampleCountMin ? a.sampleCountMax : a.sampleCountMin);
    const int pixelGate = ctx->knob.pixelGateOverride ? ctx->knob.pixelGateOverride : (unitSamples <= 64u ? 4 : RTOW_PIXEL_GATE);
    // Lanes in a hurry (kernel: HURRY; twins of the static-sphere kind's generic reference-stream variants): a pixel that runs at more than this many rays per sample stops waiting for
    // company.  Batch groups run a pixel's batches side by side and keep every wave busy to the end: no bound, and the variants without the code.  Static spheres only: measured at
    // depth 32, same box (profiles/r06x_lanes_in_a_hurry.json) - cover scene +21 % (adaptive) / +33 % (chains), 10 000 spheres +24 %; in its first form (a bound on the batch's
    // rays) moving spheres with a lens -1.6 %, the 250 882-triangle mesh -8.6 % (a stage run for one lane costs the whole wave a memory round trip there).
    // (hurryTwin: exactly the launches launchByDiagGeo serves from a twin; on top of it this host's policy - not for groups, the reference stream only)
    const bool records16 = a.diagnostics && a.diagnosticsStride >= 16;
    const bool twin = !a.chainIndependent && p->rngPolicy == RTOW_RNG_REFERENCE &&
                      hurryTwin(a.layout.sceneKind, a.layout.exactTies != 0, ctx->wideCodes, a.noiseColor, false, records16, a.refTree != nullptr, a.traceDepth);
    const float urgentRays = !twin ? __builtin_inff() : (a.ldsSceneBytes == a.layout.totalBytes ? RTOW_URGENT_RAYS_PER_SAMPLE : RTOW_URGENT_RAYS_PER_SAMPLE_BEYOND_LDS);
    uint32_t bits;
    memcpy(&bits, &urgentRays, sizeof bits);
    if (!(urgentRays < __builtin_inff())) bits = 0u;                                  // no bound: the variants without the code (they read tune[7] as the pixel gate alone)
    a.tune[7] = (int32_t)((bits & 0xffffff00u) | (uint32_t)(pixelGate & 255));
}

// A slice that owns no row (SliceOffset >= height): Execute returns for every index (JOBS/SampleBatchJob.cs:69-70) - nothing is
// written, nothing is launched (a zero-sized grid is not a valid launch); the events still bracket "this batch"
int recordEmptyBatch(RtowContext ctx, hipStream_t stream)
{
    if (ctx->haveBatchDone) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->evBatchDone, 0), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventRecord(ctx->evStart, stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventRecord(ctx->evStop, stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventRecord(ctx->evBatchDone, stream), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->haveBatchDone = true;
    ctx->haveTiming = true;
    return RTOW_SUCCESS;
}

// Per-sample policies: work units are (owned pixel, group of kSampleGroup samples); each leaves a record that fold_unit_records_kernel adds up
int planUnits(RtowContext ctx, const RtowSampleParams* p, SampleKernelArgs& a)
{
    a.groupsPerPixel = 1;
    a.xoroshiro = p->rngPolicy == RTOW_RNG_PER_SAMPLE_XOROSHIRO ? 1 : 0;
    if (p->rngPolicy == RTOW_RNG_REFERENCE) return RTOW_SUCCESS;
    const uint32_t ownedPixels = a.totalWork;
    uint32_t groups = (a.sampleCountMax > a.sampleCountMin ? a.sampleCountMax : a.sampleCountMin);
    groups = (groups + kSampleGroup - 1) / kSampleGroup;
    if (groups < 1) groups = 1;
    if ((uint64_t)ownedPixels * groups > 0x7fffffffull) return RTOW_ERROR_CAPACITY;
    a.groupsPerPixel = groups;
    a.totalWork = ownedPixels * groups;
    RTOW_TRY(growDevice(ctx, {{&ctx->dUnitRecords, (size_t)a.totalWork * 64u}}));
    a.unitRecords = ctx->dUnitRecords;
    return RTOW_SUCCESS;
}

struct TieWatch {
    bool on = false;         // this launch lists tied pixels for the fix-up launch
    bool triangles = false;  // ... of an all-triangle scene (its exact-tie kernels render them)
    bool inPlace = false;    // an output buffer is also the input buffer (a chain's later batches always read the outputs, but they read what THIS launch stored: only batch 0's inputs count)
};

// ---- nearest-hit ties under the rank rule: sphere kinds of more than 16 entities, reference stream - a pixel that meets two different spheres at
// bit-identical distance at a nearest hit is listed instead of stored, and the exact-tie kernel of the same kind renders the list in a second, tiny launch
// All-triangle scenes whose exact-tie kernels were chosen for their size alone (no triangle twice: SceneLayout.tieWatchOk) are watched too: the rank-rule kernels trace the
// frame, the exact-tie kernels the marked pixels - unless the scene has shown that it ties often (triWatchOff: the flag below, or a list that overflowed)
int prepareTieWatch(RtowContext ctx, const RtowSampleParams* p, const RtowAccumBuffers* in, const RtowAccumBuffers* out, SampleKernelArgs& a, TieWatch& tie)
{
    if (ctx->hCancel[3] != 0u) { ctx->hCancel[3] = 0u; if (triangleKind(ctx->scene.layout.sceneKind)) { ctx->triWatchOff = true; logf(ctx, 3, "rtow", "this scene's nearest hits tie often: exact-tie kernels from now on"); } }
    const bool sphereWatch = ctx->scene.layout.sceneKind <= SCENE_KIND_SPHERES_MOTION && !ctx->scene.layout.exactTies && ctx->scene.entityCount > 16;
    tie.triangles = triangleKind(ctx->scene.layout.sceneKind) && ctx->scene.layout.exactTies && ctx->scene.layout.tieWatchOk && !ctx->triWatchOff &&
                    !(ctx->flags & RTOW_CONTEXT_EXACT_TIES_ALWAYS);
    tie.on = (sphereWatch || tie.triangles) && !(ctx->flags & RTOW_CONTEXT_EXACT_TIES_NEVER) && p->rngPolicy == RTOW_RNG_REFERENCE;
    if (tie.on && tie.triangles) a.layout.exactTies = 0u;               // this launch goes through the rank-rule kernels of the kind; the fix-up launch sets the bit again
    tie.inPlace = in->color == out->color || in->normal == out->normal || in->albedo == out->albedo || in->sampleCountWeight == out->sampleCountWeight;
    if (!tie.on) return RTOW_SUCCESS;
    RTOW_TRY(growDevice(ctx, {{&ctx->dTieRedo, (4u + (size_t)kTieRedoCapacity) * sizeof(unsigned)}}));
    const uint32_t most = (uint32_t)std::min<uint64_t>((uint64_t)ctx->scene.entityCount, listCapacity(ctx, false));
    const uint32_t entries = most > (uint32_t)kLocalHitEntries ? most - (uint32_t)kLocalHitEntries : 0u;
    RTOW_TRY(growDevice(ctx, {{&ctx->dRedoSpill, (size_t)entries * kTieRedoBlocks * kBlockThreads * sizeof(uint4)}}));
    ctx->redoSpillEntries = entries;
    const size_t framePixels = (size_t)a.width * (size_t)a.height;
    const size_t words = (framePixels + 31u) / 32u;
    RTOW_TRY(growDevice(ctx, {{&ctx->dTieBits, words * sizeof(unsigned)}}));
    if (tie.inPlace) RTOW_TRY(growDevice(ctx, {{&ctx->dTieInputs, framePixels * 11u * sizeof(float)}}));
    return RTOW_SUCCESS;
}

// ---- camera-ray candidate lists: one conservative beam walk per pixel, reused by all its samples (and by later batches of the same view) ----
int refreshCameraRays(RtowContext ctx, SampleKernelArgs& a, uint32_t ownedPixels, hipStream_t stream)
{
    if (ctx->flags & RTOW_CONTEXT_NO_CAMERA_RAY_LISTS) return RTOW_SUCCESS;
    const size_t pixels = (size_t)a.width * (size_t)a.height;
    const size_t listBytes = pixels * sizeof(uint4);      // 8 x 16-bit node codes per pixel; 4 x 32-bit with wide codes
    bool grew = false;
    RtowContext_t::CameraLists& lists = ctx->cameraLists;
    const int reserved = growDevice(ctx, {{&lists.dLists, listBytes}}, &grew);
    if (grew) lists.key.drop();
    RTOW_TRY(reserved);
    // Pruned lists (rtow_camera_lists.hip.h) leave out what no camera ray of the pixel can hit or see: the frame is the same, but BoundsHitCount / CandidateCount
    // are not - so a launch that writes the 16-byte records keeps the whole lists, and the lists are rebuilt when a context goes from one record size to the other
    const bool prune = !(ctx->flags & RTOW_CONTEXT_UNPRUNED_CAMERA_RAY_LISTS) && !(a.diagnostics && a.diagnosticsStride >= 16);
    // everything the kernel reads that an upload does not fix (rtow_launch_cache.h) - among it the bits of the float Size: a pixel's beam spans cx / Size.x .. (cx + 1) / Size.x
    // of the view, so the fraction of Size moves every beam
    const CameraListKey key = cameraListKey(ctx->sceneSerial, a, prune);
    if (!lists.key.holds(key)) {
        SampleKernelArgs perPixel = a;                       // the lists are per pixel whatever the work units are
        perPixel.totalWork = ownedPixels;
        HIP_TRY(ctx, launchPrimaryCandidates(perPixel, lists.dLists, prune, stream), RTOW_ERROR_LAUNCH_FAILURE);
        lists.key.set(key);
        lists.ownedPixels = ownedPixels;
    }
    a.pixelCandidates = lists.dLists;
    return RTOW_SUCCESS;
}

struct OrderPlan {
    bool want = false;     // the launch runs its chunks in an order, and leaves the order for the next batch
    bool mapped = false;   // ... and a ticket map (which pixels share a chunk), re-sorted behind the launch too
    bool have = false;     // an order is on hand for this launch (else it runs in natural order and records the first one)
};

// Ticket-map classes (regroup_tickets_kernel) for costs of at least floorCost rays per pixel
void regroupClasses(const RtowContext_t* ctx, unsigned floorCost, unsigned out[3])
{
    const unsigned mode = ctx->knob.regroupMode;
    if (ctx->knob.ticketMapSide == 1u) { out[0] = mode == 0u ? 0u : (2u << mode); out[1] = out[2] = 0u; return; }      // tile order: levels of the tile's cost range (mode 1 / 2 / 3: 4 / 8 / 16), 0 = by the ray count itself
    out[0] = mode == 0u ? 0u : floorCost; out[1] = mode >= 2u ? (floorCost * 11u) / 4u : 0xffffffffu; out[2] = mode >= 2u ? floorCost * 4u : 0xffffffffu;
}

int regroupTickets(RtowContext ctx, const SampleKernelArgs& a, unsigned floorCost, hipStream_t stream)
{
    unsigned cls[3];
    regroupClasses(ctx, floorCost, cls);
    const unsigned tileRows = a.tilesPerRow ? a.tiledPixels / (64u * a.tilesPerRow) : 0u;
    HIP_TRY(ctx, launchRegroupTickets(ctx->chunkOrder.dPixelCost, ctx->chunkOrder.dTicketMap, a.tilesPerRow, tileRows, ctx->knob.ticketMapSide, cls, stream), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

// ---- chunk order: most expensive 64-pixel chunks first, from the ray counts of the previous launch (or of a probe) ----
// ---- and which pixels share a chunk (a wave): the pixels of a super-tile of ticketMapSide x ticketMapSide tiles sorted by the ray counts of the previous launch and dealt out
// 64 at a time (regroup_tickets_kernel), re-sorted behind every launch like the order.  Reference stream only (per-sample units are alike by construction).
int prepareChunkOrder(RtowContext ctx, SampleKernelArgs& a, int blocks, hipStream_t stream, OrderPlan& order)
{
    a.chunkCount = (a.totalWork + 63u) / 64u;
    order.want = a.chunkCount >= (uint32_t)(4 * ctx->cuCount) && !(ctx->flags & RTOW_CONTEXT_NO_CHUNK_ORDER);   // tiny frames: not worth it
    // batch groups: (chunk, batch) slots a wave reserves at a time (schedulerTune[7] bits 8 .. 11 override the default for A/B runs)
    a.slotBlock = ctx->knob.slotBlockOverride ? ctx->knob.slotBlockOverride : kGroupSlotBlock;
    if (!ctx->knob.slotBlockOverride) {
        // Reserving several (chunk, batch) slots per pull pays where a wave has dozens of them to work through (a whole frame's group: 79 slots per wave, +1.8 %); a launch that
        // owns a few slots per wave - the sub-batches of an 8-way row slice: 7.9 - must balance with single slots (profiles/r06j_partitions_c2.json: 10.9 ms per step against the
        // 7.9 of round 5's single slots)
        const uint64_t slotsPerWave = (uint64_t)a.chunkCount * a.chainCount / ((uint64_t)blocks * (uint64_t)(kBlockThreads / 64));
        if (slotsPerWave < 32u) a.slotBlock = 1u;
        else if (slotsPerWave < 64u && a.slotBlock > 2u) a.slotBlock = 2u;
    }
    order.mapped = order.want && ctx->knob.ticketMapSide >= 1u && a.tiledPixels != 0u && !a.unitRecords;
    if (!order.want) return RTOW_SUCCESS;
    RtowContext_t::ChunkOrder& co = ctx->chunkOrder;
    bool grew = false;
    const int reserved = growDevice(ctx, {{&co.dChunkCost, (2 * (size_t)a.chunkCount + kChunkOrderScratchWords) * sizeof(unsigned)}, {&co.dChunkOrder, a.chunkCount * sizeof(unsigned)},
                                          {&co.dPixelCost, (size_t)a.chunkCount * 64 * sizeof(unsigned short)}, {&co.dTicketMap, (size_t)a.chunkCount * 64 * sizeof(unsigned)}}, &grew);
    if (grew) co.key.drop();
    RTOW_TRY(reserved);
    const ChunkOrderKey key = chunkOrderKey(ctx->sceneSerial, a, order.mapped);      // (per-sample units are never mapped)
    a.pixelCost = co.dPixelCost;
    a.ticketMap = order.mapped ? co.dTicketMap : nullptr;
    order.have = true;
    if (!co.key.holds(key)) {
        co.key.drop();                                       // what follows overwrites the map on hand, however far it gets
        if (a.unitRecords) {
            // per-sample units are small and alike: the first batch simply runs in natural order and records the map for the next
            HIP_TRY(ctx, hipMemsetAsync(co.dPixelCost, 0, (size_t)a.chunkCount * 64 * sizeof(unsigned short), stream), RTOW_ERROR_LAUNCH_FAILURE);
            order.have = false;
        } else {
            // no cost map yet for this scene and frame configuration: a 1-sample-per-pixel probe of the same kernel (stores nothing else)
            SampleKernelArgs probe = a;
            probe.probeOnly = 1;
            probe.chunkOrder = nullptr;
            probe.ticketMap = nullptr;                           // the probe runs over the tiles themselves; the map starts from them
            if (order.mapped) HIP_TRY(ctx, launchInitTicketMap(co.dTicketMap, a.tiledPixels, stream), RTOW_ERROR_LAUNCH_FAILURE);
            probe.cancelFlag = nullptr;
            probe.chainCount = 1;                                // one pass over the pixels, whatever the launch it prepares
            HIP_TRY(ctx, hipMemsetAsync(ctx->dWorkCounter, 0, sizeof(unsigned int), stream), RTOW_ERROR_LAUNCH_FAILURE);
            HIP_TRY(ctx, hipMemsetAsync(co.dPixelCost, 0, (size_t)a.chunkCount * 64 * sizeof(unsigned short), stream), RTOW_ERROR_LAUNCH_FAILURE);   // the last chunk's tail
            HIP_TRY(ctx, launchSampleBatch(probe, blocks, stream), RTOW_ERROR_LAUNCH_FAILURE);
            if (order.mapped) RTOW_TRY(regroupTickets(ctx, a, 1u, stream));
            HIP_TRY(ctx, launchBuildChunkOrder(co.dPixelCost, co.dChunkCost, a.chunkCount, co.dChunkOrder, 0, stream), RTOW_ERROR_LAUNCH_FAILURE);
        }
        co.key.set(key);
    }
    a.chunkOrder = order.have ? co.dChunkOrder : nullptr;
    return RTOW_SUCCESS;
}

// ---- stage thresholds: measured once per scene on this batch's own kernel, frame and view (see kTuneProbeSamples) ----
// Never waited for: the probes are enqueued in front of a batch, timed with events, and a LATER call that finds the last event complete reads them
// and switches the thresholds (scheduling only: no result depends on when that happens).  Until then the kernel kind's built-in values run.
void measureThresholds(RtowContext ctx, SampleKernelArgs& a, int blocks, bool haveOrder, hipStream_t stream)
{
    for (int k = 0; k < 7; k++) a.tune[k] = ctx->tune[k] < 1 ? 1 : ctx->tune[k];
    RtowContext_t::ThresholdTuning& tuning = ctx->tuning;
    if (finishThresholdTuning(ctx, /*wait*/ false))          // (probes in flight are this scene's: an upload drops them)
        for (int k = 0; k < 7; k++) a.tune[k] = ctx->tune[k] < 1 ? 1 : ctx->tune[k];
    tuning.sppSinceUpload += (uint64_t)a.chainCount * (a.sampleCountMax > a.sampleCountMin ? a.sampleCountMax : a.sampleCountMin);
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;                   // a stream that is being captured into a graph cannot carry the event pairs: no measurement then
    if (hipStreamIsCapturing(stream, &capturing) != hipSuccess) { (void)hipGetLastError(); capturing = hipStreamCaptureStatusNone; }
    // worth it only where the scene is rendered for longer than the probes take (3 or 6 candidates x 3 repeats x 4 samples per pixel: 40 - 76 samples per
    // pixel): a one-shot render of a few samples per pixel (BASELINE.json configs[0]: 8) must not pay several times its own work first
    const bool worthIt = tuning.sppSinceUpload >= kTuneMinSamplesPerPixel;
    if (ctx->userTune || (ctx->flags & RTOW_CONTEXT_NO_THRESHOLD_TUNING) || tuning.state != tuning.Unmeasured || a.unitRecords || !haveOrder ||
        !worthIt || capturing != hipStreamCaptureStatusNone)
        return;
    const bool volumes = a.layout.sceneKind == SCENE_KIND_VOLUMES || a.layout.sceneKind == SCENE_KIND_VOLUMES_TEXTURED;
    const int candidates = volumes ? 2 * kFamilies : kFamilies;                      // volume kinds: each family also with the volume stage from half of the live lanes
    const int launches = candidates * kTuneProbeRepeats;
    tuning.events.assign((size_t)launches + 1, nullptr);
    bool ok = true;
    for (auto& e : tuning.events) ok = ok && hipEventCreate(&e) == hipSuccess;
    ok = ok && tuning.dProbeSink.ensure(64) == hipSuccess;
    SampleKernelArgs probe = a;
    probe.probeOnly = kTuneProbeSamples;
    probe.pixelCost = nullptr;                           // the cost map stays the cost probe's (or the previous batch's)
    probe.cancelFlag = nullptr;
    probe.overflowFlag = tuning.dProbeSink;               // a probe's ray beyond the hit-list capacity is not the batch's (which may trace fewer samples than a probe)
    probe.chainCount = 1;
    probe.chainIndependent = 0;
    // one untimed probe first: clocks, L2 and the instruction cache are warm before the first timed one
    candidateThresholds(0, probe.tune, 7);
    if (ok) ok = hipMemsetAsync(ctx->dWorkCounter, 0, sizeof(unsigned int), stream) == hipSuccess && launchSampleBatch(probe, blocks, stream) == hipSuccess;
    if (ok) ok = hipEventRecord(tuning.events[0], stream) == hipSuccess;
    for (int l = 0; ok && l < launches; l++) {
        candidateThresholds(l % candidates, probe.tune, 7);
        ok = hipMemsetAsync(ctx->dWorkCounter, 0, sizeof(unsigned int), stream) == hipSuccess && launchSampleBatch(probe, blocks, stream) == hipSuccess &&
             hipEventRecord(tuning.events[(size_t)l + 1], stream) == hipSuccess;
    }
    if (ok) {
        tuning.state = tuning.Pending;
        tuning.candidates = candidates;
        tuning.builtin = a.layout.sceneKind <= SCENE_KIND_SPHERES_MOTION ? 0 : 1;       // what rtowUploadScene set for this kernel kind
    } else {
        (void)hipGetLastError();
        settleThresholdTuning(ctx, -1);                 // not measurable: do not try again for this scene
        logf(ctx, 2, "tune", "threshold probes failed; the per-kind values stay");
    }
}

// Plain or chained launches with paths deeper than 16 segments are bound by their slowest pixels (see "lanes in a hurry" above), not by lane occupancy: a static-sphere scene
// that is whole in LDS runs them with REGEN from a quarter of the live lanes, HIT from 3/8, and the walk's hand-over at 4 candidates (profiles/r06u_deep_plain_launch_thresholds.json:
// +7 ... +10 %; the same values cost batch groups 2.8 %, launches at depth <= 16 1.3 ... 3 %, moving spheres 2 %, and 10 000 spheres - next to the lanes in a hurry - 2 %)
void applyDeepPlainThresholds(const RtowContext_t* ctx, const RtowSampleParams* p, SampleKernelArgs& a)
{
    const int* builtin = kThresholdFamilies[0];
    if (!ctx->userTune && !a.chainIndependent && a.traceDepth > 16 && p->rngPolicy == RTOW_RNG_REFERENCE && a.layout.sceneKind == SCENE_KIND_SPHERES && a.ldsSceneBytes == a.layout.totalBytes &&
        a.tune[0] == builtin[0] && a.tune[3] == builtin[3] && a.tune[6] == builtin[6]) {
        a.tune[0] = 16; a.tune[3] = 24; a.tune[6] = 4;
    }
}

// The per-batch table of a chained launch or a batch group - seed and diagnostics; a group's outputs, a chain's extrema source (a zeroed entry is null for the rest) - in device
// memory, written in stream order (the previous launch's kernel may still be reading its own table: this copy is enqueued behind it).  A chain also zeroes its hand-over state.
int writeBatchTable(RtowContext ctx, const ChainSpec* chain, SampleKernelArgs& a, hipStream_t stream)
{
    if (a.chainCount <= 1u) return RTOW_SUCCESS;
    if (!a.chainIndependent) {
        // per-chunk hand-off counters of the chain: pixels stored so far (all batches); batch b of a chunk waits for b x its pixels
        RTOW_TRY(growDevice(ctx, {{&ctx->dChunkDone, (size_t)a.chunkCount * sizeof(unsigned)}, {&ctx->dXcdState, sizeof(XcdState) + (size_t)kMaxXcds * a.chunkCount * sizeof(unsigned)}}));
        HIP_TRY(ctx, hipMemsetAsync(ctx->dChunkDone, 0, (size_t)a.chunkCount * sizeof(unsigned), stream), RTOW_ERROR_LAUNCH_FAILURE);
        a.chunkDone = ctx->dChunkDone;
        // chunk ownership per XCD: counters zero, list entries "not written yet" (the kernel indexes the lists with THIS launch's chunkCount)
        HIP_TRY(ctx, hipMemsetAsync(ctx->dXcdState, 0, sizeof(XcdState), stream), RTOW_ERROR_LAUNCH_FAILURE);
        HIP_TRY(ctx, hipMemsetAsync(ctx->dXcdState + sizeof(XcdState), 0xff, (size_t)kMaxXcds * a.chunkCount * sizeof(unsigned), stream), RTOW_ERROR_LAUNCH_FAILURE);
        a.xcdState = reinterpret_cast<XcdState*>(ctx->dXcdState.get());
        a.extremaKeys = chain->extremaKeys;
    }
    RTOW_TRY(growDevice(ctx, {{&ctx->dChainBatches, sizeof(ChainBatch) * kMaxChain}}));
    ChainBatch table[kMaxChain] = {};
    for (int b = 0; b < chain->count; b++) {
        table[b].seed = chain->seeds[b];
        table[b].diagnostics = chain->diags ? (uint8_t*)chain->diags[b] : nullptr;
        if (chain->outs) { table[b].outColor = chain->outs[b].color; table[b].outNormal = chain->outs[b].normal; table[b].outAlbedo = chain->outs[b].albedo; table[b].outScw = chain->outs[b].sampleCountWeight; }
        if (chain->extrema) table[b].extrema = chain->extrema[b];
    }
    HIP_TRY(ctx, hipMemcpyAsync(ctx->dChainBatches, table, sizeof(ChainBatch) * (size_t)chain->count, hipMemcpyHostToDevice, stream), RTOW_ERROR_LAUNCH_FAILURE);
    a.chainBatches = ctx->dChainBatches;
    return RTOW_SUCCESS;
}

// The tie watch's state for this launch: an empty list and bitmap, and - the fix-up launch renders a marked pixel again from the launch's inputs, which an in-place
// launch overwrites - a copy of those inputs (44 B per pixel through HBM, ~0.05 ms at 1920 x 1080 against a batch's tens of milliseconds); redoIn: where the fix-up reads them
int prepareTieInputs(RtowContext ctx, const RtowSampleParams* p, SampleKernelArgs& a, const TieWatch& tie, const float* redoIn[4], hipStream_t stream)
{
    const size_t framePixels = (size_t)a.width * (size_t)a.height;
    HIP_TRY(ctx, hipMemsetAsync(ctx->dTieRedo, 0, 4u * sizeof(unsigned), stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipMemsetAsync(ctx->dTieBits, 0, ((framePixels + 31u) / 32u) * sizeof(unsigned), stream), RTOW_ERROR_LAUNCH_FAILURE);
    if (tie.inPlace) {
        static const size_t comps[4] = {4, 3, 3, 1};
        float* at = ctx->dTieInputs;
        const size_t rows = (size_t)ownedRows(p);                // the rows this launch writes (row % SliceDivider == SliceOffset), at their places in the frame
        for (int k = 0; k < 4; k++) {
            const size_t rowBytes = (size_t)a.width * comps[k] * sizeof(float), first = (size_t)a.sliceOffset * rowBytes, pitch = (size_t)a.sliceDivider * rowBytes;
            HIP_TRY(ctx, hipMemcpy2DAsync((uint8_t*)at + first, pitch, (const uint8_t*)redoIn[k] + first, pitch, rowBytes, rows, hipMemcpyDeviceToDevice, stream), RTOW_ERROR_LAUNCH_FAILURE);
            redoIn[k] = at;
            at += framePixels * comps[k];
        }
    }
    a.tieBits = ctx->dTieBits;
    return RTOW_SUCCESS;
}

// the fix-up: marked pixels -> list -> the exact-tie kernel of the same kind over the list (almost always empty: that kernel then leaves before it stages the scene).
// A chain's pixel is listed once and carried through all its batches; a group's once per batch.
int launchTieFixup(RtowContext ctx, const SampleKernelArgs& a, const TieWatch& tie, const float* const redoIn[4], hipStream_t stream)
{
    const size_t framePixels = (size_t)a.width * (size_t)a.height;
    HIP_TRY(ctx, launchCollectTiedPixels(ctx->dTieBits, (unsigned)((framePixels + 31u) / 32u), ctx->dTieRedo, kTieRedoCapacity, a.chainIndependent ? a.chainCount : 1u, a.overflowFlag + 1,
                                         tie.triangles ? kTieWatchBusy : 0xffffffffu, stream),
            RTOW_ERROR_LAUNCH_FAILURE);
    SampleKernelArgs r = a;
    r.layout.exactTies = 1u;
    r.redoMode = 1;
    r.tune[7] &= 255;                      // (the exact-tie kernels have no lanes in a hurry: the pixel gate alone)
    r.tieBits = nullptr;
    r.tieRedo = ctx->dTieRedo;
    r.tieRedoCapacity = kTieRedoCapacity;
    r.inColor = redoIn[0]; r.inNormal = redoIn[1]; r.inAlbedo = redoIn[2]; r.inScw = redoIn[3];
    r.pixelCost = nullptr;
    r.chunkOrder = nullptr;
    r.pixelCandidates = a.pixelCandidates;
    r.hitSpill = ctx->redoSpillEntries ? ctx->dRedoSpill : nullptr;
    r.hitSpillEntries = ctx->redoSpillEntries;
    r.hitSpillStride = (uint32_t)kTieRedoBlocks * (uint32_t)kBlockThreads;
    HIP_TRY(ctx, hipMemsetAsync(ctx->dWorkCounter, 0, sizeof(unsigned int), stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, launchSampleBatch(r, kTieRedoBlocks < ctx->cuCount ? kTieRedoBlocks : ctx->cuCount, stream), RTOW_ERROR_LAUNCH_FAILURE);
    logf(ctx, 4, "launch", "%s: tie fix-up over the pixels the watch listed", sampleKernelName(r.layout));
    return RTOW_SUCCESS;
}

// The batch itself: the launch (timed, with its tie fix-up and the fold of per-sample records), then the order for the next batch from what this one measured
int enqueueLaunch(RtowContext ctx, const RtowSampleParams* p, SampleKernelArgs& a, int blocks, const TieWatch& tie, const OrderPlan& order, hipStream_t stream)
{
    const float* redoIn[4] = {a.inColor, a.inNormal, a.inAlbedo, a.inScw};
    if (tie.on) RTOW_TRY(prepareTieInputs(ctx, p, a, tie, redoIn, stream));
    HIP_TRY(ctx, hipMemsetAsync(ctx->dWorkCounter, 0, sizeof(unsigned int), stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventRecord(ctx->evStart, stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, launchSampleBatch(a, blocks, stream), RTOW_ERROR_LAUNCH_FAILURE);
    logf(ctx, 4, "launch", "%s: %u batch%s%s", sampleKernelName(a.layout), a.chainCount, a.chainCount > 1u ? (a.chainIndependent ? "es, a group" : "es, a chain") : "", tie.on ? ", tie watch" : "");
    if (tie.on) RTOW_TRY(launchTieFixup(ctx, a, tie, redoIn, stream));
    if (a.unitRecords) HIP_TRY(ctx, launchFoldUnitRecords(a, stream), RTOW_ERROR_LAUNCH_FAILURE);   // inside the timed region: part of the batch
    HIP_TRY(ctx, hipEventRecord(ctx->evStop, stream), RTOW_ERROR_LAUNCH_FAILURE);
    // refresh the order for the next batch from what this one measured (same stream, after the timed kernel)
    if (order.mapped) RTOW_TRY(regroupTickets(ctx, a, std::max(1u, a.sampleCountMin), stream));
    // (development: schedulerTune[7] + 64 orders the chunks by their TOTAL ray count instead of by their most expensive pixel)
    if (order.want)
        HIP_TRY(ctx, launchBuildChunkOrder(ctx->chunkOrder.dPixelCost, ctx->chunkOrder.dChunkCost, a.chunkCount, ctx->chunkOrder.dChunkOrder, ctx->knob.orderByTotal ? 0 : 1, stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventRecord(ctx->evBatchDone, stream), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->haveBatchDone = true;
    ctx->haveTiming = true;
    return RTOW_SUCCESS;
}

// rtowSamplePixelsDevice: the caller's list (device memory of 4 + capacity words) a launch renders instead of the frame
struct ListSpec { const unsigned* words; uint32_t capacity; };

// A list launch (rtow.h: rtowSamplePixelsDevice): the exact-tie kernel of the scene's kind in redoMode - as launchTieFixup sets it up, the only launch there is - over
// the context's own copy of the caller's list.  The copy (launchFilterPixelList) clamps the count, drops entries beyond the frame - the kernel turns an entry into an
// address without a look - and frees the caller's list in stream order.  No tie bitmap (these kernels resolve their ties themselves), no cost map, chunk order or ticket
// map read or left behind, no threshold probes and no samples counted towards them, no lanes in a hurry; camera-ray lists as for a batch of that view.
int enqueueListLaunch(RtowContext ctx, SampleKernelArgs& a, const ChainSpec* chain, const ListSpec& list, hipStream_t stream)
{
    const uint32_t ownedPixels = a.totalWork;                                        // the whole frame (slice 0 / 1)
    a.wideCodes = ctx->wideCodes ? 1 : 0;
    a.blockThreads = kBlockThreads;
    // persistent workgroups as for a frame, but no more than the list can occupy
    const int blocks = (int)std::max<uint64_t>(1u, std::min<uint64_t>((uint64_t)ctx->cuCount, ((uint64_t)list.capacity + (uint32_t)kBlockThreads - 1u) / (uint32_t)kBlockThreads));
    if (!ctx->scene.layout.exactTies) {
        // a scene that runs on the rank-rule kernels has no hit-list spill of its own: the area of these workgroups, sized the way sizeHitSpill sizes an exact-tie scene's
        const uint32_t most = (uint32_t)std::min<uint64_t>((uint64_t)ctx->scene.entityCount, listCapacity(ctx, false));
        const uint32_t entries = most > (uint32_t)kLocalHitEntries ? most - (uint32_t)kLocalHitEntries : 0u;
        const uint64_t slots = (uint64_t)entries * (uint64_t)blocks;
        RTOW_TRY(growDevice(ctx, {{&ctx->dListSpill, (size_t)slots * kBlockThreads * sizeof(uint4)}}));
        a.hitSpill = entries ? ctx->dListSpill : nullptr;
        a.hitSpillEntries = entries;
        a.hitSpillStride = (uint32_t)blocks * (uint32_t)kBlockThreads;
    }   // (else buildArgs gave the scene's own area: one slice per CU, and blocks <= cuCount)
    // grow-only, allocated on first use (freeing waits for a launch that still reads the smaller list); a list of capacity 0 has its four header words and a scratch word
    RTOW_TRY(growDevice(ctx, {{&ctx->dPixelList, RTOW_PIXEL_LIST_BYTES(list.capacity)}, {&ctx->dPixelListScratch, (((size_t)list.capacity + 63u) / 64u + 1u) * sizeof(unsigned)}}));
    // the context's list, ticket counter, batch table and candidate lists are the previous batch's until it has finished (launchSample)
    if (ctx->haveBatchDone) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->evBatchDone, 0), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, launchFilterPixelList(list.words, list.capacity, ownedPixels, ctx->dPixelListScratch, ctx->dPixelList, stream), RTOW_ERROR_LAUNCH_FAILURE);
    RTOW_TRY(refreshCameraRays(ctx, a, ownedPixels, stream));
    a.chunkCount = (a.totalWork + 63u) / 64u;            // (what writeBatchTable sizes a chain's hand-over state by; a list launch hands over in registers and reads none of it)
    RTOW_TRY(writeBatchTable(ctx, chain, a, stream));
    a.redoMode = 1;
    a.tune[7] &= 255;                                    // the pixel gate alone
    a.tieBits = nullptr;
    a.tieRedo = ctx->dPixelList;
    a.tieRedoCapacity = list.capacity;
    a.pixelCost = nullptr; a.chunkOrder = nullptr; a.ticketMap = nullptr;
    HIP_TRY(ctx, hipMemsetAsync(ctx->dWorkCounter, 0, sizeof(unsigned int), stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventRecord(ctx->evStart, stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, launchSampleBatch(a, blocks, stream), RTOW_ERROR_LAUNCH_FAILURE);
    logf(ctx, 4, "launch", "%s: %u batch%s over a pixel list of up to %u, %d workgroups", sampleKernelName(a.layout), a.chainCount, a.chainCount > 1u ? "es" : "", list.capacity, blocks);
    HIP_TRY(ctx, hipEventRecord(ctx->evStop, stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventRecord(ctx->evBatchDone, stream), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->haveBatchDone = true;
    ctx->haveTiming = true;
    return RTOW_SUCCESS;
}

// One launch of one batch, a chain or a group (chain), enqueued on `stream` behind everything the context's previous batch enqueued.
// extremaIn (optional): device memory the kernel reads the SampleCountWeightExtrema from instead of p's (rtowSampleBatchChainAdaptiveDevice)
// list (optional): the launch renders the pixels of this list instead of the frame (rtowSamplePixelsDevice; the caller has checked that the scene's kind can)
int launchSample(RtowContext ctx, const RtowSampleParams* p, const RtowAccumBuffers* in, const RtowAccumBuffers* out, void* diag,
                 hipStream_t stream, bool useCancelFlag, const ChainSpec* chain = nullptr, const RtowFloat2* extremaIn = nullptr, const ListSpec* list = nullptr)
{
    SampleKernelArgs a{};
    RTOW_TRY(buildArgs(ctx, p, in, out, diag, useCancelFlag, chain, extremaIn, a));
    if (list) a.layout.exactTies = 1u;                   // (before the plan: these kernels have no "lanes in a hurry" twin)
    RTOW_TRY(planHistory(ctx, p, a));
    setSchedulerValues(ctx, p, a);                       // (the hurry rate reads a.layout.exactTies before the triangle tie watch clears it)
    const uint32_t ownedPixels = a.totalWork;
    if (ownedPixels == 0) return recordEmptyBatch(ctx, stream);
    RTOW_TRY(planUnits(ctx, p, a));
    if (list) return enqueueListLaunch(ctx, a, chain, *list, stream);
    TieWatch tie;
    RTOW_TRY(prepareTieWatch(ctx, p, in, out, a, tie));

    // ---- launch geometry: one persistent 1024-lane workgroup per CU (four waves per SIMD).  Smaller workgroups for launches that own about one pixel
    // per resident lane were built, measured and removed: results never depended on it.
    a.wideCodes = ctx->wideCodes ? 1 : 0;
    a.blockThreads = kBlockThreads;
    int blocks = (int)((a.totalWork + (uint32_t)a.blockThreads - 1) / (uint32_t)a.blockThreads);
    if (blocks > ctx->cuCount) blocks = ctx->cuCount; // persistent: one workgroup per CU
    if (blocks < 1) blocks = 1;

    // Batches of one context share its ticket counter, cost map, chunk order and candidate lists, and each one consumes what the
    // previous one produced: whatever stream this batch was given, it starts after everything the previous batch enqueued.
    if (ctx->haveBatchDone) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->evBatchDone, 0), RTOW_ERROR_LAUNCH_FAILURE);
    RTOW_TRY(refreshCameraRays(ctx, a, ownedPixels, stream));
    OrderPlan order;
    RTOW_TRY(prepareChunkOrder(ctx, a, blocks, stream, order));
    if (order.want) measureThresholds(ctx, a, blocks, order.have, stream);
    applyDeepPlainThresholds(ctx, p, a);                 // (after a finished measurement may have replaced a.tune[0 .. 6])
    RTOW_TRY(writeBatchTable(ctx, chain, a, stream));
    return enqueueLaunch(ctx, p, a, blocks, tie, order, stream);
}

// Most surfaces one ray may meet where whole hit lists are kept: the caller's bound if it gave one, else a default that GROWS (growHitList) - the
// reference's list grows on the heap without bound (UTIL/HybridCollections.cs:22-36,65-71).
uint64_t listCapacity(const RtowContext_t* ctx, bool volumes)
{
    if (ctx->hitListCapacity) return ctx->hitListCapacity;
    return std::max<uint64_t>(volumes ? kDefaultHitListCapacity : kDefaultTieListCapacity, ctx->grownListCapacity);
}

// The spill area behind the lanes' own 24 entries, for a scene of this kind and size.  An entity yields at most two hits per ray (a volume hull's entry and exit,
// JOBS/SampleBatchJob.cs:457-469), one in scenes without volumes, so that bound - capped by listCapacity - is all a scene can need.
int sizeHitSpill(RtowContext ctx, uint32_t sceneKind, bool exactTies, int entityCount)
{
    const bool volumes = sceneKind == SCENE_KIND_VOLUMES || sceneKind == SCENE_KIND_VOLUMES_TEXTURED;
    uint64_t most = (volumes || exactTies) ? (uint64_t)entityCount * (volumes ? 2u : 1u) : 0u;
    const uint64_t cap = listCapacity(ctx, volumes);
    if (most > cap) most = cap;
    const uint32_t entries = most > (uint64_t)kLocalHitEntries ? (uint32_t)(most - kLocalHitEntries) : 0u;
    bool grew = false;
    const int reserved = growDevice(ctx, {{&ctx->dHitSpill, (size_t)entries * (size_t)ctx->cuCount * kBlockThreads * sizeof(uint4)}}, &grew);
    if (grew) ctx->hitSpillEntries = 0;
    RTOW_TRY(reserved);
    ctx->hitSpillEntries = entries;
    return RTOW_SUCCESS;
}

// A batch met a ray with more surfaces than the lists hold.  Unless the caller fixed the capacity, double it - up to what the scene can produce at all and to a
// quarter of the device's free memory - so that the batch, issued again, has room.  Called with every batch of the context finished (all callers have just waited).
bool growHitList(RtowContext ctx)
{
    if (ctx->hitListCapacity || !ctx->haveScene) return false;
    const uint32_t kind = ctx->scene.layout.sceneKind;
    const bool volumes = kind == SCENE_KIND_VOLUMES || kind == SCENE_KIND_VOLUMES_TEXTURED;
    const uint64_t bound = (uint64_t)ctx->scene.entityCount * (volumes ? 2u : 1u);
    const uint64_t now = listCapacity(ctx, volumes);
    if (now >= bound) return false;                                                      // the lists already hold everything the scene has
    const uint64_t next = std::min<uint64_t>(bound, now * 2u);
    if (volumes || ctx->scene.layout.exactTies) {
        size_t freeBytes = 0, totalBytes = 0;
        if (hipMemGetInfo(&freeBytes, &totalBytes) != hipSuccess) { (void)hipGetLastError(); return false; }
        const uint64_t held = ctx->dHitSpill.bytes();
        const uint64_t need = (next - kLocalHitEntries) * (uint64_t)ctx->cuCount * kBlockThreads * sizeof(uint4);
        if (need > held && need > (freeBytes + held) / 4u) return false;
    }
    const uint32_t before = ctx->grownListCapacity;
    ctx->grownListCapacity = (uint32_t)next;
    if (sizeHitSpill(ctx, kind, ctx->scene.layout.exactTies != 0, ctx->scene.entityCount) != RTOW_SUCCESS) {
        (void)hipGetLastError();
        ctx->grownListCapacity = before;
        (void)sizeHitSpill(ctx, kind, ctx->scene.layout.exactTies != 0, ctx->scene.entityCount);
        return false;
    }
    return true;                                                                          // (the fix-up launch's own, small area follows at the next launch: launchSample)
}

// A ray met more surfaces than the context's hit-list capacity (volume scenes and exact-tie kernels keep every hit of a ray): the batch's result is not the
// reference's.  With RtowContextOptions.hitListCapacity == 0 the capacity has doubled by the time this returns (growHitList): the host-buffer calls then run the
// batch again themselves, a device-resident caller issues it again (from inputs the batch did not overwrite).
// The flag is sticky: it is set by the kernel and cleared only here, so it covers every batch enqueued since the last report
// (rtowSampleBatch, a cancellable rtowSampleBatchDevice, rtowGetBatchStatus, rtowSynchronize).
int takeOverflow(RtowContext ctx)
{
    if (ctx->hCancel[2] != 0u) {
        // not a hit list: a launch marked more pixel-batches for the tie fix-up pass than its list holds (kTieRedoCapacity = 2^20; a scene of coinciding spheres that
        // did not go to the exact-tie kernels: e.g. one of the two "moving" by a zero offset).  Growing the hit lists would not help, and for a sphere scene running
        // the batch again would overflow again: the error is final there (tests/test_gpu_tie_overflow.py)
        ctx->hCancel[2] = 0u;
        ctx->hCancel[1] = 0u;
        if (ctx->haveScene && triangleKind(ctx->scene.layout.sceneKind) && !ctx->triWatchOff) {
            // an all-triangle scene that ties over whole regions (coplanar layers): its exact-tie kernels need no list - the batch, issued again, runs on them
            ctx->triWatchOff = true;
            ctx->hCancel[3] = 0u;
            ctx->overflowGrew = true;
            logf(ctx, 3, "rtow", "more than %u pixel-batches of one launch met nearest-hit ties: results of this batch are invalid; the scene runs on the exact-tie kernels from now on", kTieRedoCapacity);
            return RTOW_ERROR_CAPACITY;
        }
        ctx->overflowGrew = false;
        logf(ctx, 2, "rtow", "more than %u pixel-batches of one launch met nearest-hit ties: results of this batch are invalid (use RTOW_CONTEXT_EXACT_TIES_ALWAYS for this scene)", kTieRedoCapacity);
        return RTOW_ERROR_CAPACITY;
    }
    if (ctx->hCancel[1] == 0u) return RTOW_SUCCESS;
    ctx->hCancel[1] = 0u;
    const bool volumes = ctx->scene.layout.sceneKind == SCENE_KIND_VOLUMES || ctx->scene.layout.sceneKind == SCENE_KIND_VOLUMES_TEXTURED;
    const uint32_t was = (uint32_t)listCapacity(ctx, volumes);
    ctx->overflowGrew = growHitList(ctx);
    if (ctx->overflowGrew) logf(ctx, 3, "rtow", "a ray met more than %u surfaces: results of this batch are invalid; the hit-list capacity is now %u", was, (uint32_t)listCapacity(ctx, volumes));
    else logf(ctx, 2, "rtow", "a ray met more surfaces than the hit-list capacity of this scene (%u; RtowContextOptions.hitListCapacity): results of this batch are invalid", was);
    return RTOW_ERROR_CAPACITY;
}

// Block until the stop event completes while mirroring the caller's cancellation byte into the device-visible flag.
int waitWithCancel(RtowContext ctx, const volatile uint8_t* cancel)
{
    bool cancelled = false;
    for (;;) {
        const hipError_t q = hipEventQuery(ctx->evStop);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady) {
            logf(ctx, 2, "hip", "sample kernel failed: %s", hipGetErrorString(q));
            ctx->hCancel[1] = 0u;
            ctx->hCancel[2] = 0u;
            return RTOW_ERROR_LAUNCH_FAILURE;
        }
        if (cancel && *cancel && !cancelled) {
            *ctx->hCancel = 1u;
            cancelled = true;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    if (cancel && *cancel) cancelled = true;
    if (cancelled) {
        ctx->hCancel[1] = 0u;          // the cancelled batch's outputs are discarded; its overflow must not be blamed on the next batch
        ctx->hCancel[2] = 0u;
        return RTOW_ERROR_CANCELLED;
    }
    return takeOverflow(ctx);
}

// The host-buffer calls' grow-only staging: the frame's four accumulators, and one diagnostics frame per batch - devDiag[b], null for a batch without a buffer
int prepareStaging(RtowContext ctx, int count, const RtowSampleParams* p, void* const* diagnostics, std::vector<void*>& devDiag)
{
    const size_t pixels = (size_t)(int)p->size.x * (size_t)(int)p->size.y, diagBytes = pixels * (size_t)p->diagnosticsStride;
    RTOW_TRY(growDevice(ctx, {{&ctx->dColor, pixels * 16}, {&ctx->dNormal, pixels * 12}, {&ctx->dAlbedo, pixels * 12}, {&ctx->dScw, pixels * 4}}));
    RTOW_TRY(growDevice(ctx, {{&ctx->dDiag, diagnostics ? diagBytes * (size_t)count : 0}}));
    devDiag.assign((size_t)count, nullptr);
    if (diagnostics) for (int b = 0; b < count; b++) devDiag[(size_t)b] = diagnostics[b] ? ctx->dDiag + (size_t)b * diagBytes : nullptr;
    return RTOW_SUCCESS;
}

// Whether the `count` batches of one call may share launches: they differ in nothing but Seed (the reference's successive batches of a frame: UNITY/Raytracer.cs:656-661) -
// and SampleCountWeightExtrema where `extremaFree` (the adaptive call: each batch reads its own from device memory) - under the reference RNG policy (per-sample units
// fold through records), in a frame of fewer than 2^27 padded owned pixels.  Batches of a chain hand accumulators over inside the launch (handOver): only where this
// device passed the same-XCD litmus (ctx->chainFusion); the batches of a group hand nothing over.
bool canFuse(const RtowContext_t* ctx, int count, const RtowSampleParams* params, void* const* diagnostics, bool handOver, bool extremaFree)
{
    if (params[0].rngPolicy != RTOW_RNG_REFERENCE || (handOver && !ctx->chainFusion)) return false;
    for (int b = 1; b < count; b++) {
        RtowSampleParams q = params[b];
        q.seed = params[0].seed;
        if (extremaFree) q.sampleCountWeightExtrema = params[0].sampleCountWeightExtrema;
        if (memcmp(&q, &params[0], sizeof(q)) != 0) return false;
    }
    if ((uint64_t)ownedRows(&params[0]) * (uint64_t)(int)params[0].size.x + 63u >= (1ull << 27)) return false;     // (padded to chunks of 64: 2^27 is a multiple of 64)
    // (the tie fix-up list names FRAME pixels beside the batch number, batch << 27 | pixel: a sliced launch of a frame of 2^27 pixels or more runs batch by batch)
    if ((uint64_t)(int)params[0].size.x * (uint64_t)(int)params[0].size.y >= (1ull << 27)) return false;
    // one launch is one kernel variant, and the variant follows the record format (launchByDiag: 16-byte FULL_DIAGNOSTICS records need the
    // counters compiled in): a call in which only SOME batches carry a diagnostics buffer runs batch by batch, each with its own variant
    if (diagnostics) {
        int withDiag = 0;
        for (int b = 0; b < count; b++) withDiag += diagnostics[b] != nullptr ? 1 : 0;
        if (withDiag != 0 && withDiag != count) return false;
    }
    return true;
}

// `count` batches enqueued on `s`: one launch per kMaxChain of them when `fuse`, else one per batch.  A chain: batch 0 reads `in`, every later one what its
// predecessor stored to `out` (what the chain is defined to equal).  A group: every batch reads `in` and stores to out[b].  With `cancel` every launch is waited for.
// list (optional): every launch renders the pixels of this list instead of the frame (rtowSamplePixelsDevice).
// The caller holds ctx->mu and has validated params / buffers.
int enqueueBatches(RtowContext ctx, int count, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* out, void* const* diagnostics,
                   bool group, bool fuse, hipStream_t s, const volatile uint8_t* cancel, const ListSpec* list = nullptr)
{
    int rc = RTOW_SUCCESS;
    for (int first = 0; first < count && rc == RTOW_SUCCESS;) {
        const int n = fuse ? std::min(count - first, (int)kMaxChain) : 1;
        const RtowAccumBuffers* src = (group || first == 0) ? in : out;
        const RtowAccumBuffers* dst = group ? &out[first] : out;
        if (n == 1) {
            rc = launchSample(ctx, &params[first], src, dst, diagnostics ? diagnostics[first] : nullptr, s, cancel != nullptr, nullptr, nullptr, list);
        } else {
            uint32_t seeds[kMaxChain];
            for (int b = 0; b < n; b++) seeds[b] = params[first + b].seed;
            const ChainSpec spec{n, seeds, diagnostics ? diagnostics + first : nullptr, group ? out + first : nullptr};
            rc = launchSample(ctx, &params[first], src, dst, nullptr, s, cancel != nullptr, &spec, nullptr, list);
        }
        if (rc == RTOW_SUCCESS && cancel) rc = waitWithCancel(ctx, cancel);
        first += n;
    }
    return rc;
}

// The sample entry points' common start, in this order (the same bad input gets the same code): every batch's params - validateParams, where a trace depth beyond 64
// is RTOW_ERROR_CAPACITY - each followed by the call's own per-batch check; the four input buffers and, unless `out` is null (groups check theirs per batch), the four
// output buffers; then the lock, the scene, the device (calls come from a different worker thread each time), the stream (null: the context's) and a clear cancel word.
template <typename BatchCheck>
int beginSample(RtowContext ctx, std::unique_lock<std::mutex>& lock, int count, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* out,
                BatchCheck check, void* stream, hipStream_t* s)
{
    if (!ctx || !in || !params || count < 1) return RTOW_ERROR_INVALID_VALUE;
    for (int b = 0; b < count; b++) {
        int v = validateParams(&params[b]);
        if (v == RTOW_SUCCESS) v = check(b);
        if (v != RTOW_SUCCESS) return v;
    }
    if (!in->color || !in->normal || !in->albedo || !in->sampleCountWeight) return RTOW_ERROR_INVALID_VALUE;
    if (out && (!out->color || !out->normal || !out->albedo || !out->sampleCountWeight)) return RTOW_ERROR_INVALID_VALUE;
    lock = std::unique_lock<std::mutex>(ctx->mu);
    if (!ctx->haveScene) return RTOW_ERROR_NO_SCENE;
    RTOW_TRY(useDevice(ctx, stream, s));
    *ctx->hCancel = 0u;
    return RTOW_SUCCESS;
}
int noBatchCheck(int) { return RTOW_SUCCESS; }

// The host-buffer calls: the caller's inputs -> staging (one DMA per buffer: pinned when the caller registered its pools, pageable otherwise), the batches into `out`
// (null: in place in the staging - each lane reads its pixel before writing it), and a wait.  The reference's hit list grows without bound (UTIL/HybridCollections.cs:65-71).
// Here a ray that outgrew the lists made the batches invalid and the lists twice as long (hitListCapacity 0: growHitList): the batches run again from the caller's
// inputs - if nothing has overwritten them (inputsSurvive) - until they fit or the scene's own bound / the memory is reached.
int sampleFromHost(RtowContext ctx, int count, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* out, void* const* diagnostics, bool fuse,
                   bool inputsSurvive, const volatile uint8_t* cancel)
{
    const size_t n = (size_t)(int)params[0].size.x * (size_t)(int)params[0].size.y;
    const RtowAccumBuffers dev{ctx->dColor, ctx->dNormal, ctx->dAlbedo, ctx->dScw};
    hipStream_t s = ctx->stream;
    for (;;) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dColor, in->color, n * 16, hipMemcpyHostToDevice, s), RTOW_ERROR_LAUNCH_FAILURE);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dNormal, in->normal, n * 12, hipMemcpyHostToDevice, s), RTOW_ERROR_LAUNCH_FAILURE);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dAlbedo, in->albedo, n * 12, hipMemcpyHostToDevice, s), RTOW_ERROR_LAUNCH_FAILURE);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->dScw, in->sampleCountWeight, n * 4, hipMemcpyHostToDevice, s), RTOW_ERROR_LAUNCH_FAILURE);
        *ctx->hCancel = 0u;
        ctx->overflowGrew = false;
        int rc = enqueueBatches(ctx, count, params, &dev, out ? out : &dev, diagnostics, false, fuse, s, cancel);
        if (rc == RTOW_SUCCESS && !cancel) rc = waitWithCancel(ctx, nullptr);
        if (rc == RTOW_ERROR_CAPACITY && ctx->overflowGrew && inputsSurvive) continue;
        return rc;
    }
}

// copy back ONLY the rows this slice owns from the staging - skipped pixels write nothing (JOBS/SampleBatchJob.cs:69-70) - and each batch's diagnostics (devDiag[b])
int copyOwnedRows(RtowContext ctx, const RtowSampleParams* p, const RtowAccumBuffers* out, int count, void* const* diagnostics, void* const* devDiag)
{
    const int rows = ownedRows(p);
    if (rows <= 0) return RTOW_SUCCESS;
    const size_t w = (size_t)(int)p->size.x, D = (size_t)p->sliceDivider, O = (size_t)p->sliceOffset;
    auto copyRows = [&](void* dst, const void* src, size_t bytesPerPixel) -> hipError_t {
        const size_t rowBytes = w * bytesPerPixel;
        return hipMemcpy2DAsync((uint8_t*)dst + O * rowBytes, D * rowBytes, (const uint8_t*)src + O * rowBytes, D * rowBytes, rowBytes, (size_t)rows,
                                hipMemcpyDeviceToHost, ctx->stream);
    };
    HIP_TRY(ctx, copyRows(out->color, ctx->dColor, 16), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, copyRows(out->normal, ctx->dNormal, 12), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, copyRows(out->albedo, ctx->dAlbedo, 12), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, copyRows(out->sampleCountWeight, ctx->dScw, 4), RTOW_ERROR_LAUNCH_FAILURE);
    if (diagnostics)
        for (int b = 0; b < count; b++)
            if (diagnostics[b]) HIP_TRY(ctx, copyRows(diagnostics[b], devDiag[b], (size_t)p->diagnosticsStride), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

} // namespace

extern "C" {

RTOW_API int rtowGetApiVersion(void) { return RTOW_API_VERSION; }

RTOW_API const char* rtowErrorString(int result)
{
    switch (result) {
        case RTOW_SUCCESS: return "success";
        case RTOW_ERROR_INVALID_VALUE: return "invalid value";
        case RTOW_ERROR_MEMORY_ALLOCATION: return "memory allocation failed";
        case RTOW_ERROR_NO_DEVICE: return "no usable HIP device (gfx950 required; there is no CPU fallback)";
        case RTOW_ERROR_NO_SCENE: return "no scene uploaded";
        case RTOW_ERROR_UNSUPPORTED: return "feature not built yet";
        case RTOW_ERROR_LAUNCH_FAILURE: return "kernel launch or stream failure";
        case RTOW_ERROR_CANCELLED: return "cancelled";
        case RTOW_ERROR_CAPACITY: return "capacity exceeded";
        case RTOW_ERROR_INTERNAL: return "internal error";
    }
    return "unknown error";
}

RTOW_API int rtowCreateContext(const RtowContextOptions* options, RtowContext* outContext)
{
    if (!outContext) return RTOW_ERROR_INVALID_VALUE;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return RTOW_ERROR_NO_DEVICE;
    const int ordinal = options ? options->deviceOrdinal : 0;
    if (ordinal < 0 || ordinal >= count) return RTOW_ERROR_INVALID_VALUE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ordinal) != hipSuccess) return RTOW_ERROR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RTOW_ERROR_NO_DEVICE; // the code object is gfx950 only
    if (hipSetDevice(ordinal) != hipSuccess) return RTOW_ERROR_NO_DEVICE;

    RtowContext ctx = new (std::nothrow) RtowContext_t();
    if (!ctx) return RTOW_ERROR_MEMORY_ALLOCATION;
    ctx->device = ordinal;
    ctx->cuCount = prop.multiProcessorCount;
    if (options) {
        ctx->logCb = options->logCallback; ctx->logData = options->logCallbackData; ctx->logLevel = options->logCallbackLevel;
        ctx->flags = options->flags;
        if ((ctx->flags & RTOW_CONTEXT_EXACT_TIES_ALWAYS) && (ctx->flags & RTOW_CONTEXT_EXACT_TIES_NEVER)) { delete ctx; return RTOW_ERROR_INVALID_VALUE; }
        if (options->ldsSceneBudgetBytes > 0) ctx->ldsSceneBudget = (uint32_t)options->ldsSceneBudgetBytes;
        if (options->hitListCapacity < 0) { delete ctx; return RTOW_ERROR_INVALID_VALUE; }
        if (options->sliceBlockThreads != 0 && options->sliceBlockThreads != 1024) { delete ctx; return RTOW_ERROR_INVALID_VALUE; }     // reserved (round 3: 256 / 512)
        ctx->hitListCapacity = (uint32_t)options->hitListCapacity;
        bool anyTune = false;
        for (int i = 0; i < 9; i++) anyTune = anyTune || (i != 7 && options->schedulerTune[i] != 0);
        if (anyTune) {
            // stage thresholds below 1 mean "any lane" (1); a zero hand-over count or walk slice means "the built-in value" (3; per scene at upload), as in API v6
            for (int i = 0; i < 9; i++) ctx->tune[i] = options->schedulerTune[i] < 1 ? 1 : options->schedulerTune[i];
            if (options->schedulerTune[6] < 1) ctx->tune[6] = 3;
            ctx->userSliceDefault = options->schedulerTune[8] < 1;
        }
        ctx->userTune = anyTune;
    }
    // schedulerTune[7] is its own knob: it says nothing about the thresholds (0, or no options: the default word)
    if (!decodeSchedulerKnob(options ? options->schedulerTune[7] : 0, &ctx->knob)) {
        logf(ctx, 2, "rtow", "schedulerTune[7] = %d: the low four bits must be 1, 2, 3, 4 or 8 (or 0 for the default)", options->schedulerTune[7]);
        delete ctx;
        return RTOW_ERROR_INVALID_VALUE;
    }
    bool ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreate(&ctx->evStart) == hipSuccess && hipEventCreate(&ctx->evStop) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ctx->evBatchDone, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ctx->evGatherDone, hipEventDisableTiming) == hipSuccess;
    ok = ok && hipEventCreateWithFlags(&ctx->evMetricsDone, hipEventDisableTiming) == hipSuccess;
    ok = ok && ctx->dWorkCounter.ensure(sizeof(unsigned int)) == hipSuccess;
    ok = ok && ctx->dPartials.ensure(sizeof(MetricsPartial) * kMetricsBlocks) == hipSuccess;
    // the finalize pass may be given any stream later: the table is complete before the context exists for the caller
    ok = ok && ctx->dByteThresholds.ensure(kByteThresholdTableBytes) == hipSuccess;
    ok = ok && launchBuildByteThresholds(ctx->dByteThresholds, ctx->stream) == hipSuccess && hipStreamSynchronize(ctx->stream) == hipSuccess;
    ok = ok && ctx->pinned.allocate(256, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess;
    void* pinnedDevice = nullptr;
    ok = ok && hipHostGetDevicePointer(&pinnedDevice, ctx->pinned.get(), 0) == hipSuccess;
    if (!ok) { rtowDestroyContext(ctx); return RTOW_ERROR_MEMORY_ALLOCATION; }
    ctx->hCancel = (volatile uint32_t*)ctx->pinned.get();
    ctx->hMetricsRecord = (volatile RtowMetrics*)((uint8_t*)ctx->pinned.get() + 64);        // where the blocking metrics reduction has its record written by the device
    ctx->dMetricsRecord = (RtowMetrics*)((uint8_t*)pinnedDevice + 64);
    ctx->hCancel[0] = 0u;
    ctx->hCancel[1] = 0u;
    ctx->hCancel[2] = 0u;
    ctx->hCancel[3] = 0u;          // [3]: a watched launch of an all-triangle scene listed thousands of tied pixels (read at the next launch: triWatchOff)
    logf(ctx, 4, "rtow", "context on device %d (%s, %d CUs)", ordinal, prop.gcnArchName, ctx->cuCount);
    // chained launches hand accumulators over inside an XCD with plain stores + sc1 loads: measured on THIS device before it is relied on
    if (ctx->flags & RTOW_CONTEXT_NO_CHAIN_FUSION) {
        ctx->chainFusion = false;
    } else {
        // stale > 0: the hand-over is unsafe on this device.  timeouts > 0 with nothing stale: inconclusive - the litmus needs its 2 x CU workgroups resident at the same time,
        // which a device shared with other work may not grant within its bounded waits - so it runs once more before chains are given up (RtowSceneInfo does not say so; the log does)
        unsigned pairs = 0, stale = 0, timeouts = 0;
        hipError_t le = hipSuccess;
        for (int attempt = 0; attempt < 2; attempt++) {
            le = runXcdCoherenceLitmus(ctx->cuCount, ctx->stream, &pairs, &stale, &timeouts);
            if (le != hipSuccess || stale != 0 || (pairs > 0 && timeouts == 0)) break;
            logf(ctx, 3, "rtow", "same-XCD hand-over litmus inconclusive (%u pairs, %u timeouts): %s", pairs, timeouts, attempt == 0 ? "once more" : "giving up");
        }
        ctx->chainFusion = le == hipSuccess && pairs > 0 && stale == 0 && timeouts == 0;
        if (le != hipSuccess) (void)hipGetLastError();
        logf(ctx, ctx->chainFusion ? 4 : 3, "rtow", "same-XCD hand-over litmus: %u pairs, %u stale dwords, %u timeouts%s", pairs, stale, timeouts,
             ctx->chainFusion ? "" : stale ? " - unsafe here: chained batches will run one launch per batch" : " - inconclusive: chained batches will run one launch per batch");
    }
    *outContext = ctx;
    return RTOW_SUCCESS;
}

RTOW_API int rtowDestroyContext(RtowContext ctx)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    dropThresholdTuning(ctx);
    releaseComm(ctx);
    for (const RtowContext_t::HostRange& r : ctx->hostRanges) (void)hipHostUnregister(r.base);
    delete ctx;
    return RTOW_SUCCESS;
}

RTOW_API int rtowUploadScene(RtowContext ctx, const RtowSceneDesc* scene)
{
    if (!ctx || !scene) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    CompiledScene compiled;
    std::string err;
    // the library's own tree is always built to the LDS stack's depth; scene->maxBvhDepth (the host's tree) only decides the order of
    // hits at identical distances (rtow_reforder.h)
    const int rc = compileScene(scene, RTOW_STACK_CAPACITY, &compiled, &err);
    if (rc != RTOW_SUCCESS) {
        logf(ctx, 2, "scene", "%s", err.c_str());
        return rc;
    }
    HIP_TRY(ctx, hipDeviceSynchronize(), RTOW_ERROR_LAUNCH_FAILURE);   // no batch (on whatever stream it was given) may still be reading the old scene
    RTOW_TRY(growDevice(ctx, {{&ctx->dScene, compiled.blob.size()}}));
    HIP_TRY(ctx, hipMemcpy(ctx->dScene, compiled.blob.data(), compiled.blob.size(), hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    if (!compiled.entityOfPrim.empty()) {      // all-triangle scenes: the device queries report the host's entity index, as rtowProbeNearestHit does
        const size_t n = compiled.entityOfPrim.size();
        RTOW_TRY(growDevice(ctx, {{&ctx->dEntityOfPrim, n * sizeof(int32_t)}}));
        HIP_TRY(ctx, hipMemcpy(ctx->dEntityOfPrim, compiled.entityOfPrim.data(), n * sizeof(int32_t), hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    }
    // ... and rtowShadeHitsDevice goes the other way, from the entity index the queries reported to the primitive: the inverse map, -1 for an entity without a primitive
    ctx->dPrimOfEntity.release();
    ctx->primOfEntityCount = 0;      // (the device is idle)
    if (!compiled.entityOfPrim.empty() && compiled.entityCount > 0) {
        std::vector<int32_t> primOfEntity((size_t)compiled.entityCount, -1);
        for (size_t prim = 0; prim < compiled.entityOfPrim.size(); prim++) {
            const int32_t entity = compiled.entityOfPrim[prim];
            if (entity >= 0 && entity < compiled.entityCount) primOfEntity[(size_t)entity] = (int32_t)prim;
        }
        RTOW_TRY(growDevice(ctx, {{&ctx->dPrimOfEntity, primOfEntity.size() * sizeof(int32_t)}}));
        HIP_TRY(ctx, hipMemcpy(ctx->dPrimOfEntity, primOfEntity.data(), primOfEntity.size() * sizeof(int32_t), hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
        ctx->primOfEntityCount = compiled.entityCount;
    }
    if (!compiled.texBlob.empty()) {
        RTOW_TRY(growDevice(ctx, {{&ctx->dTexBlob, compiled.texBlob.size()}}));
        HIP_TRY(ctx, hipMemcpy(ctx->dTexBlob, compiled.texBlob.data(), compiled.texBlob.size(), hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
        compiled.texBlob.clear();
        compiled.texBlob.shrink_to_fit();                                     // the host copy is not needed again
    }
    if (ctx->flags & RTOW_CONTEXT_REFERENCE_DIAGNOSTICS) {
        // the counters' walk keeps one stack entry per level of the reference tree (+1): 64 entries of scratch
        if (compiled.refTreeDepth > 62) { logf(ctx, 2, "scene", "RTOW_CONTEXT_REFERENCE_DIAGNOSTICS supports MaxBvhDepth <= 62"); return RTOW_ERROR_CAPACITY; }
        RTOW_TRY(growDevice(ctx, {{&ctx->dRefTree, compiled.refTree.size()}}));
        HIP_TRY(ctx, hipMemcpy(ctx->dRefTree, compiled.refTree.data(), compiled.refTree.size(), hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    }
    compiled.refTree.clear();
    compiled.refTree.shrink_to_fit();
    HIP_TRY(ctx, launchPrepareMaterials(ctx->dScene, compiled.layout, ctx->stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, launchPrepareEntities(ctx->dScene, compiled.layout, ctx->stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), RTOW_ERROR_LAUNCH_FAILURE);
    // rtowProbeNearestHit walks the HOST image of the scene: bring back what the device derived for the entities (inverse rotations / translations of the GpuPrim records)
    if (compiled.layout.sceneKind >= SCENE_KIND_GENERAL && compiled.entityCount > 0)
        HIP_TRY(ctx, hipMemcpy(compiled.blob.data() + compiled.layout.primOffset, ctx->dScene + compiled.layout.primOffset, (size_t)compiled.entityCount * sizeof(GpuPrim), hipMemcpyDeviceToHost),
                RTOW_ERROR_LAUNCH_FAILURE);
    if (ctx->flags & (RTOW_CONTEXT_EXACT_TIES_ALWAYS | RTOW_CONTEXT_EXACT_TIES_NEVER)) {   // exact-tie kernels for every scene without volumes (slower), or never
        const bool volumes = compiled.layout.sceneKind == SCENE_KIND_VOLUMES || compiled.layout.sceneKind == SCENE_KIND_VOLUMES_TEXTURED;
        if (!volumes) compiled.layout.exactTies = (ctx->flags & RTOW_CONTEXT_EXACT_TIES_ALWAYS) ? 1u : 0u;
    }
    {
        // Rays whose hit list outgrows a lane's own 24 entries (every hit is kept in volume scenes and by the exact-tie procedure) continue in HBM
        const int rc = sizeHitSpill(ctx, compiled.layout.sceneKind, compiled.layout.exactTies != 0, compiled.entityCount);
        if (rc != RTOW_SUCCESS) return rc;
    }
    // every scene kind has kernels with 32-bit codes (volume kinds included: a triangle-mesh scene with one fog volume among the meshes)
    const bool wide = compiled.entityCount > 65535 || compiled.layout.nodeCount > 65535u || (ctx->flags & RTOW_CONTEXT_FORCE_WIDE_CODES) != 0;
    ctx->wideCodes = wide;
    if (!ctx->userTune) {
        // Box-walk slice (node visits per trip).  16 for trees whose nodes come from LDS or L2 (with the hand-over at 3 candidates: cover 12 / 16 / 20
        // visits 9.34 / 9.48 / 9.23 Gsamples/s; 10 000 spheres, tree partly in LDS, 16 / 20 / 24: 8.00 / 7.81 / 7.45).  A tree of hundreds of
        // thousands of nodes is read from HBM at several times the latency per visit, and a ray visits twice as many nodes: longer slices amortise the
        // trip around them (250 882-triangle mesh, 24 / 32 / 40 visits: 2.04 / 1.97 / 1.86 Gsamples/s; gpurun_out/r03bc.  With walks that ran until the
        // candidate list was full the optima were 16 / 20 / 32: r03h, r03ap).
        const int* base = kThresholdFamilies[compiled.layout.sceneKind <= SCENE_KIND_SPHERES_MOTION ? 0 : 1];      // measured per family: see RTOW_DEFAULT_TUNE
        for (int k = 0; k < 9; k++) ctx->tune[k] = base[k];
        // (round 6: on the rank-rule triangle kernel that traces meshes now, 12 / 16 / 20 / 24 / 32 visits run 2 374 / 2 361 / 2 326 / 2 343 / 2 231 Msamples/s: the 24 of
        // round 3's exact-tie kernel is no better than the 16 everything else uses, profiles/r06n_mesh_scheduler_sweep.json)
    } else if (ctx->userSliceDefault) {
        ctx->tune[8] = 16;
    }
    std::lock_guard<std::mutex> sceneLock(ctx->sceneMu);          // rtowProbeNearestHit reads the host image under this lock only
    ctx->scene = std::move(compiled);
    // LDS of a launch: a traversal-stack row per inner level of THIS tree, then the scene image - whole, or the top of the node array (planLds, rtow_kernels.h)
    // (static spheres: with the 80-byte node image of the sign-ordered walk when the tree allows it and the image fits next to the whole scene; the variants that walk it are the
    // launcher's business - launchVariant - the others stage the 64-byte nodes in the same plan)
    const SceneLayout& sl = ctx->scene.layout;
    const bool nodeImage = !wide && sl.sceneKind == SCENE_KIND_SPHERES && !(ctx->flags & RTOW_CONTEXT_NODE_IMAGE_64) &&
                           node_planes_ordered(reinterpret_cast<const GpuNode*>(ctx->scene.blob.data() + sl.nodeOffset), sl.nodeCount, sl.sphereCount > 1u);
    ctx->ldsPlan = planLds(wide, sl, 0u, ctx->ldsSceneBudget, nodeImage);
    ctx->ldsSceneBytes = ctx->ldsPlan.sceneBytes;
    ctx->ldsNodeCount = ctx->ldsPlan.nodeCount;
    ctx->haveScene = true;
    sceneReplaced(ctx, wide);
    logf(ctx, 4, "scene", "%d entities, %u BVH nodes, depth %u, %u bytes (%u in LDS)%s%s", ctx->scene.entityCount, ctx->scene.layout.nodeCount,
         ctx->scene.layout.bvhDepth, ctx->scene.layout.totalBytes, ctx->ldsSceneBytes,
         ctx->scene.layout.exactTies ? ", exact-tie kernels" : "", ctx->ldsPlan.nodeImageBytes ? ", 80-byte node image" : "");
    return RTOW_SUCCESS;
}

RTOW_API int rtowUploadSkyCubemap(RtowContext ctx, const RtowCubemapDesc* cubemap)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    if (!cubemap || !cubemap->faces) {                       // drop it: Cubemap.Sample returns default when the data pointer is null
        HIP_TRY(ctx, hipDeviceSynchronize(), RTOW_ERROR_LAUNCH_FAILURE);
        ctx->dCubemap.release();
        ctx->cubemap = RtowCubemapDesc{};
        return RTOW_SUCCESS;
    }
    if (cubemap->faceWidth <= 0 || cubemap->faceHeight <= 0 || cubemap->faceWidth > 32768 || cubemap->faceHeight > 32768) return RTOW_ERROR_INVALID_VALUE;
    if (cubemap->channelType != RTOW_CUBEMAP_UNSIGNED_BYTE && cubemap->channelType != RTOW_CUBEMAP_SIGNED_HALF) return RTOW_ERROR_INVALID_VALUE;
    const int minStride = cubemap->channelType == RTOW_CUBEMAP_SIGNED_HALF ? 6 : 3;            // r, g, b are read
    if (cubemap->pixelStride < minStride || cubemap->pixelStride > 64) return RTOW_ERROR_INVALID_VALUE;
    if (cubemap->channelType == RTOW_CUBEMAP_SIGNED_HALF && (cubemap->pixelStride & 1)) return RTOW_ERROR_INVALID_VALUE;
    const size_t bytes = (size_t)6 * (size_t)cubemap->faceWidth * (size_t)cubemap->faceHeight * (size_t)cubemap->pixelStride;
    if (bytes > 0x7fffffffull) return RTOW_ERROR_CAPACITY;                                      // Cubemap.Sample's strides are int32 here as in the reference (RT/Texture.cs:146-148)
    HIP_TRY(ctx, hipDeviceSynchronize(), RTOW_ERROR_LAUNCH_FAILURE);                            // no batch may still be reading the old faces
    bool grew = false;
    const int reserved = growDevice(ctx, {{&ctx->dCubemap, bytes}}, &grew);
    if (grew) ctx->cubemap = RtowCubemapDesc{};
    RTOW_TRY(reserved);
    HIP_TRY(ctx, hipMemcpy(ctx->dCubemap, cubemap->faces, bytes, hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->cubemap = *cubemap;
    ctx->cubemap.faces = nullptr;
    logf(ctx, 3, "sky", "cubemap %dx%d, %s, stride %d (%zu bytes)", cubemap->faceWidth, cubemap->faceHeight,
         cubemap->channelType == RTOW_CUBEMAP_SIGNED_HALF ? "half" : "byte", cubemap->pixelStride, bytes);
    return RTOW_SUCCESS;
}

RTOW_API int rtowUploadBlueNoise(RtowContext ctx, const RtowBlueNoiseDesc* noise)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    HIP_TRY(ctx, hipDeviceSynchronize(), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->dBlueNoise.release();
    ctx->blueRowStride = ctx->blueTextureCount = 0;
    if (!noise || !noise->texels) return RTOW_SUCCESS;
    if (noise->rowStride == 0 || noise->rowStride > 16384 || noise->textureCount == 0 || noise->textureCount > 4096) return RTOW_ERROR_INVALID_VALUE;
    const size_t bytes = (size_t)noise->rowStride * noise->rowStride * noise->textureCount * 8u;      // half4 texels
    RTOW_TRY(growDevice(ctx, {{&ctx->dBlueNoise, bytes}}));
    HIP_TRY(ctx, hipMemcpy(ctx->dBlueNoise, noise->texels, bytes, hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->blueRowStride = noise->rowStride;
    ctx->blueTextureCount = noise->textureCount;
    return RTOW_SUCCESS;
}

RTOW_API int rtowUploadStbNoise(RtowContext ctx, const RtowStbNoiseDesc* noise)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    HIP_TRY(ctx, hipDeviceSynchronize(), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->dStbNoise.release();
    ctx->stbRowStride = ctx->stbTextureCount = 0;
    if (!noise) return RTOW_SUCCESS;
    if (!noise->scalar || !noise->vector2 || !noise->cosineUnitVector3 || !noise->unitVector2 || !noise->unitVector3) return RTOW_ERROR_INVALID_VALUE;
    if (noise->rowStride == 0 || noise->rowStride > 16384 || noise->textureCount == 0 || noise->textureCount > 4096) return RTOW_ERROR_INVALID_VALUE;
    const size_t all = (size_t)noise->rowStride * noise->rowStride * noise->textureCount;
    RTOW_TRY(growDevice(ctx, {{&ctx->dStbNoise, all * 14u}}));                                        // 1 + 3 + 4 + 3 + 3 bytes per texel
    HIP_TRY(ctx, hipMemcpy(ctx->dStbNoise, noise->scalar, all, hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipMemcpy(ctx->dStbNoise + all, noise->vector2, all * 3, hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipMemcpy(ctx->dStbNoise + all * 4, noise->cosineUnitVector3, all * 4, hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipMemcpy(ctx->dStbNoise + all * 8, noise->unitVector2, all * 3, hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipMemcpy(ctx->dStbNoise + all * 11, noise->unitVector3, all * 3, hipMemcpyHostToDevice), RTOW_ERROR_LAUNCH_FAILURE);
    ctx->stbRowStride = noise->rowStride;
    ctx->stbTextureCount = noise->textureCount;
    return RTOW_SUCCESS;
}

RTOW_API int rtowGetSceneInfo(RtowContext ctx, RtowSceneInfo* info)
{
    if (!ctx || !info) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->haveScene) return RTOW_ERROR_NO_SCENE;
    if (ctx->tuning.state == ctx->tuning.Pending && hipSetDevice(ctx->device) == hipSuccess) (void)finishThresholdTuning(ctx, /*wait*/ false);     // a measurement whose probes are done by now
    info->entityCount = ctx->scene.entityCount;
    info->materialCount = ctx->scene.materialCount;
    info->bvhNodeCount = (int32_t)ctx->scene.layout.nodeCount;
    info->bvhDepth = (int32_t)ctx->scene.layout.bvhDepth;
    info->ldsBytesScene = (int32_t)(ctx->ldsSceneBytes + ctx->ldsPlan.nodeImageBytes);      // with the 80-byte node image where the register-history kernels stage it
    info->sceneInLds = ctx->ldsSceneBytes == ctx->scene.layout.totalBytes ? 1 : 0;
    info->sceneBytesDevice = ctx->scene.layout.totalBytes;
    info->hitSpillBytes = (uint64_t)ctx->hitSpillEntries * (uint64_t)ctx->cuCount * (uint64_t)kBlockThreads * sizeof(uint4);
    const bool keepsLists = ctx->scene.layout.exactTies || ctx->scene.layout.sceneKind == SCENE_KIND_VOLUMES || ctx->scene.layout.sceneKind == SCENE_KIND_VOLUMES_TEXTURED;
    // sphere scenes under the rank rule keep no lists in the fast kernel, but their tie fix-up launch (the exact-tie kernel over the marked pixels) does: its capacity is what a
    // RTOW_ERROR_CAPACITY of such a scene has just doubled (growHitList), and what a device-resident caller compares across the error
    const bool tieWatch = ctx->scene.layout.sceneKind <= SCENE_KIND_SPHERES_MOTION && !ctx->scene.layout.exactTies && ctx->scene.entityCount > 16 && !(ctx->flags & RTOW_CONTEXT_EXACT_TIES_NEVER);
    info->hitListCapacity = keepsLists ? (int32_t)(ctx->hitSpillEntries + (uint32_t)kLocalHitEntries)
                                       : tieWatch ? (int32_t)std::min<uint64_t>((uint64_t)ctx->scene.entityCount, listCapacity(ctx, false)) : 0;
    info->wideCodes = ctx->wideCodes ? 1 : 0;
    info->thresholdSet = ctx->tuning.winner;             // (-1 until the scene's measurement has settled)
    for (int k = 0; k < 9; k++) info->schedulerTune[k] = ctx->tune[k];
    info->schedulerTune[7] = ctx->knob.word;
    return RTOW_SUCCESS;
}

// What the camera-ray lists the context holds look like: a reduction over them on demand, behind the batch that last used them; blocks until it is done
RTOW_API int rtowGetCameraRayListStats(RtowContext ctx, RtowCameraRayListStats* stats)
{
    if (!ctx || !stats) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    memset(stats, 0, sizeof(*stats));
    if (!ctx->haveScene) return RTOW_ERROR_NO_SCENE;
    RtowContext_t::CameraLists& lists = ctx->cameraLists;
    const CameraListKey* key = lists.key.get();
    if (!key || key->sceneSerial != ctx->sceneSerial || !lists.dLists) return RTOW_SUCCESS;      // nothing built, built for an earlier upload, or no block: no lists, valid = 0
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, nullptr, &s));
    RTOW_TRY(growDevice(ctx, {{&lists.dStats, 10 * sizeof(unsigned long long)}}));
    if (ctx->haveBatchDone) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evBatchDone, 0), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, launchCameraListStats(lists.dLists, lists.ownedPixels, key->frame.width, key->frame.sliceOffset, key->frame.sliceDivider, ctx->wideCodes, lists.dStats, s),
            RTOW_ERROR_LAUNCH_FAILURE);
    unsigned long long counts[10];
    HIP_TRY(ctx, hipMemcpyAsync(counts, lists.dStats, sizeof(counts), hipMemcpyDeviceToHost, s), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipStreamSynchronize(s), RTOW_ERROR_LAUNCH_FAILURE);
    for (int k = 0; k < 9; k++) stats->pixelsWithEntries[k] = counts[k];
    stats->pixelsWithoutList = counts[9];
    stats->ownedPixels = lists.ownedPixels;
    stats->pruned = key->pruned ? 1 : 0;
    stats->valid = 1;
    return RTOW_SUCCESS;
}

RTOW_API int rtowSampleBatchDevice(RtowContext ctx, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* out,
                                   void* diagnostics, void* stream, const volatile uint8_t* cancel)
{
    if (!out) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginSample(ctx, lock, 1, params, in, out, noBatchCheck, stream, &s));
    return enqueueBatches(ctx, 1, params, in, out, &diagnostics, false, false, s, cancel);
}

RTOW_API int rtowSampleBatchChainDevice(RtowContext ctx, int32_t count, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* out,
                                        void* const* diagnostics, void* stream, const volatile uint8_t* cancel)
{
    if (!out) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginSample(ctx, lock, count, params, in, out, noBatchCheck, stream, &s));
    return enqueueBatches(ctx, count, params, in, out, diagnostics, false, canFuse(ctx, count, params, diagnostics, /*handOver*/ true, false), s, cancel);
}

// The adaptive schedule fed from the device (rtow.h).  Batches that differ in nothing but Seed and SampleCountWeightExtrema run as chained launches of at most `lag`
// batches (kMaxChain), so every extrema value a batch of a launch reads was written by an EARLIER launch - after its tie fix-up - and no batch of a launch waits for
// another batch of the same launch to end frame-wide.  A launch cannot reduce batch k's accumulators after it ends (batch k + 1 overwrote them in place): the kernel
// folds every batch's weights at store time into extrema keys (SampleKernelArgs.extremaKeys; the fix-up launch folds the pixels it renders again, the kernel skips the
// ones it marked), an init pass folds the rows of a sliced frame the launch never writes, and a decode pass writes extremaOut.  Per-sample policies, partial
// diagnostics, contexts without chain fusion, frames of 2^27 pixels or more and lag 1 run batch by batch, each launch reading its extrema through SampleKernelArgs.extremaIn
// and followed by the two-stage reduction of the frame into extremaOut[k].
RTOW_API int rtowSampleBatchChainAdaptiveDevice(RtowContext ctx, int32_t count, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* out,
                                                void* const* diagnostics, const RtowAdaptiveFeed* feed, void* stream, const volatile uint8_t* cancel)
{
    if (!out || !feed || feed->lag < 1 || !feed->extremaOut || feed->reserved != 0) return RTOW_ERROR_INVALID_VALUE;
    auto oneFrame = [&](int b) -> int {         // the reduction behind every batch covers the same W x H pixels
        return memcmp(&params[b].size, &params[0].size, sizeof(RtowFloat2)) != 0 || params[b].sliceOffset != params[0].sliceOffset ||
                       params[b].sliceDivider != params[0].sliceDivider || params[b].diagnosticsStride != params[0].diagnosticsStride
                   ? RTOW_ERROR_INVALID_VALUE : RTOW_SUCCESS;
    };
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginSample(ctx, lock, count, params, in, out, oneFrame, stream, &s));
    RTOW_TRY(growDevice(ctx, {{&ctx->dExtremaPartials, sizeof(RtowFloat2) * kMetricsBlocks}}));
    const int pixels = (int)params[0].size.x * (int)params[0].size.y;
    const int lag = feed->lag;
    auto source = [&](int k) -> const RtowFloat2* { return k < lag ? (feed->extremaIn ? feed->extremaIn + k : nullptr) : feed->extremaOut + (k - lag); };
    // what a chain fuses, with the extrema free to differ - and a launch of at most `lag` batches, so lag 1 runs batch by batch
    const bool fusable = lag > 1 && canFuse(ctx, count, params, diagnostics, /*handOver*/ true, /*extremaFree*/ true);
    if (fusable) RTOW_TRY(growDevice(ctx, {{&ctx->dExtremaKeys, 2u * sizeof(unsigned) * kMaxChain}}));
    for (int first = 0; first < count;) {
        int n = fusable ? std::min(count - first, std::min(lag, (int)kMaxChain)) : 1;
        // a batch without a device source reads the launch's kernarg extrema, i.e. batch `first`'s: the others must carry the same values
        for (int b = 1; b < n; b++)
            if (!source(first + b) && memcmp(&params[first + b].sampleCountWeightExtrema, &params[first].sampleCountWeightExtrema, sizeof(RtowFloat2)) != 0) n = 1;
        const RtowAccumBuffers* src = first == 0 ? in : out;
        int rc;
        if (n == 1) {
            rc = launchSample(ctx, &params[first], src, out, diagnostics ? diagnostics[first] : nullptr, s, cancel != nullptr, nullptr, source(first));
            if (rc != RTOW_SUCCESS) return rc;
            HIP_TRY(ctx, launchReduceWeightExtrema(pixels, out->color, out->sampleCountWeight, ctx->dExtremaPartials, feed->extremaOut + first, s), RTOW_ERROR_LAUNCH_FAILURE);
        } else {
            uint32_t seeds[kMaxChain];
            const RtowFloat2* sources[kMaxChain];
            for (int b = 0; b < n; b++) { seeds[b] = params[first + b].seed; sources[b] = source(first + b); }
            // the keys are the context's: after the previous batch's decode, whatever stream that was
            if (ctx->haveBatchDone) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->evBatchDone, 0), RTOW_ERROR_LAUNCH_FAILURE);
            HIP_TRY(ctx, launchInitExtremaKeys(ctx->dExtremaKeys, (unsigned)n, (int)params[0].size.x, (int)params[0].size.y, params[0].sliceOffset, params[0].sliceDivider,
                                               out->color, out->sampleCountWeight, s), RTOW_ERROR_LAUNCH_FAILURE);
            ChainSpec chain{n, seeds, diagnostics ? diagnostics + first : nullptr, nullptr};
            chain.extrema = sources;
            chain.extremaKeys = ctx->dExtremaKeys;
            rc = launchSample(ctx, &params[first], src, out, nullptr, s, cancel != nullptr, &chain);
            if (rc != RTOW_SUCCESS) return rc;
            HIP_TRY(ctx, launchDecodeExtremaKeys(ctx->dExtremaKeys, (unsigned)n, feed->extremaOut + first, s), RTOW_ERROR_LAUNCH_FAILURE);
        }
        // the batch ends with its extrema: the next batch of this context, on whatever stream, starts after them (it may read them; partials and keys are the context's)
        HIP_TRY(ctx, hipEventRecord(ctx->evBatchDone, s), RTOW_ERROR_LAUNCH_FAILURE);
        if (cancel) {
            rc = waitWithCancel(ctx, cancel);
            if (rc != RTOW_SUCCESS) return rc;
        }
        first += n;
    }
    return RTOW_SUCCESS;
}

RTOW_API int rtowSampleBatchGroupDevice(RtowContext ctx, int32_t count, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* outs,
                                        void* const* diagnostics, void* stream, const volatile uint8_t* cancel)
{
    if (!outs) return RTOW_ERROR_INVALID_VALUE;
    auto ownOutputs = [&](int b) -> int {
        if (!outs[b].color || !outs[b].normal || !outs[b].albedo || !outs[b].sampleCountWeight) return RTOW_ERROR_INVALID_VALUE;
        for (int c = 0; c < b; c++)                                                 // every batch its own outputs (a batch may store over the shared inputs only if it is alone)
            if (outs[b].color == outs[c].color || outs[b].normal == outs[c].normal || outs[b].albedo == outs[c].albedo || outs[b].sampleCountWeight == outs[c].sampleCountWeight) return RTOW_ERROR_INVALID_VALUE;
        if (count > 1 && (outs[b].color == in->color || outs[b].normal == in->normal || outs[b].albedo == in->albedo || outs[b].sampleCountWeight == in->sampleCountWeight)) return RTOW_ERROR_INVALID_VALUE;
        return RTOW_SUCCESS;
    };
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginSample(ctx, lock, count, params, in, nullptr, ownOutputs, stream, &s));
    return enqueueBatches(ctx, count, params, in, outs, diagnostics, /*group*/ true, canFuse(ctx, count, params, diagnostics, /*handOver*/ false, false), s, cancel);
}

RTOW_API int rtowSampleBatchChain(RtowContext ctx, int32_t count, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* out,
                                  void* const* diagnostics, const volatile uint8_t* cancel)
{
    if (!out) return RTOW_ERROR_INVALID_VALUE;
    auto oneStaging = [&](int b) -> int {       // one staging set serves the whole chain: the batches share the frame and the record format
        return (int)params[b].size.x != (int)params[0].size.x || (int)params[b].size.y != (int)params[0].size.y || params[b].diagnosticsStride != params[0].diagnosticsStride ||
                       params[b].sliceOffset != params[0].sliceOffset || params[b].sliceDivider != params[0].sliceDivider
                   ? RTOW_ERROR_INVALID_VALUE : RTOW_SUCCESS;
    };
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginSample(ctx, lock, count, params, in, out, oneStaging, nullptr, &s));
    std::vector<void*> devDiag;
    RTOW_TRY(prepareStaging(ctx, count, params, diagnostics, devDiag));
    // the chain accumulates in place in the staging buffers (its batches read what their predecessors wrote there); only the final
    // accumulators and each batch's diagnostics travel back - so the caller's inputs are untouched, and a chain whose lists have grown runs again
    const bool fuse = canFuse(ctx, count, params, diagnostics, /*handOver*/ true, false);
    RTOW_TRY(sampleFromHost(ctx, count, params, in, nullptr, diagnostics ? devDiag.data() : nullptr, fuse, /*inputsSurvive*/ true, cancel));
    RTOW_TRY(copyOwnedRows(ctx, &params[0], out, count, diagnostics, devDiag.data()));
    HIP_TRY(ctx, hipStreamSynchronize(s), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowSampleBatch(RtowContext ctx, const RtowSampleParams* params, const RtowAccumBuffers* in, const RtowAccumBuffers* out,
                             void* diagnostics, const volatile uint8_t* cancel)
{
    if (!out) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    RTOW_TRY(beginSample(ctx, lock, 1, params, in, out, noBatchCheck, nullptr, &s));
    void* const* diagList = diagnostics ? &diagnostics : nullptr;
    std::vector<void*> devDiag;
    RTOW_TRY(prepareStaging(ctx, 1, params, diagList, devDiag));
    // outputs: when every output buffer (and the diagnostics) lies in registered host memory the kernel stores straight into it - each
    // pixel's 48 + stride bytes leave over PCIe when that pixel finishes, spread over the whole batch, and there is no copy-back at all.
    // Pixels skipped by the slice test are not touched either way (JOBS/SampleBatchJob.cs:69-70).
    const size_t n = (size_t)(int)params->size.x * (size_t)(int)params->size.y;
    RtowAccumBuffers direct{(float*)mappedHost(ctx, out->color, n * 16), (float*)mappedHost(ctx, out->normal, n * 12), (float*)mappedHost(ctx, out->albedo, n * 12),
                            (float*)mappedHost(ctx, out->sampleCountWeight, n * 4)};
    uint8_t* directDiag = diagnostics ? mappedHost(ctx, diagnostics, n * (size_t)params->diagnosticsStride) : nullptr;
    const bool zeroCopyOut = direct.color && direct.normal && direct.albedo && direct.sampleCountWeight && (!diagnostics || directDiag);
    // (stores that go straight into the caller's OUTPUT arrays leave its input arrays alone unless they are the same arrays: only then a batch cannot be run twice)
    const bool inputsSurvive = !zeroCopyOut || (in->color != out->color && in->normal != out->normal && in->albedo != out->albedo && in->sampleCountWeight != out->sampleCountWeight);
    void* diag = diagnostics ? (zeroCopyOut ? (void*)directDiag : devDiag[0]) : nullptr;
    RTOW_TRY(sampleFromHost(ctx, 1, params, in, zeroCopyOut ? &direct : nullptr, &diag, false, inputsSurvive, cancel));
    if (!zeroCopyOut) RTOW_TRY(copyOwnedRows(ctx, params, out, 1, diagList, devDiag.data()));
    HIP_TRY(ctx, hipStreamSynchronize(s), RTOW_ERROR_LAUNCH_FAILURE);
    if (ctx->haveBatchDone) HIP_TRY(ctx, hipEventSynchronize(ctx->evBatchDone), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowRegisterHostBuffer(RtowContext ctx, void* pointer, size_t sizeInBytes)
{
    if (!ctx || !pointer || sizeInBytes == 0) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    for (const RtowContext_t::HostRange& r : ctx->hostRanges)
        if ((uint8_t*)pointer < r.base + r.size && r.base < (uint8_t*)pointer + sizeInBytes) return RTOW_ERROR_INVALID_VALUE;   // overlaps a live registration
    HIP_TRY(ctx, hipHostRegister(pointer, sizeInBytes, hipHostRegisterMapped | hipHostRegisterPortable), RTOW_ERROR_MEMORY_ALLOCATION);
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, pointer, 0) != hipSuccess || !dev) {
        (void)hipHostUnregister(pointer);
        return RTOW_ERROR_MEMORY_ALLOCATION;
    }
    ctx->hostRanges.push_back(RtowContext_t::HostRange{(uint8_t*)pointer, sizeInBytes, (uint8_t*)dev});
    return RTOW_SUCCESS;
}

RTOW_API int rtowUnregisterHostBuffer(RtowContext ctx, void* pointer)
{
    if (!ctx || !pointer) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    for (size_t i = 0; i < ctx->hostRanges.size(); i++)
        if (ctx->hostRanges[i].base == (uint8_t*)pointer) {
            if (ctx->haveBatchDone) (void)hipEventSynchronize(ctx->evBatchDone);      // no kernel may still be storing into it
            (void)hipStreamSynchronize(ctx->stream);
            HIP_TRY(ctx, hipHostUnregister(pointer), RTOW_ERROR_INVALID_VALUE);
            ctx->hostRanges.erase(ctx->hostRanges.begin() + (long)i);
            return RTOW_SUCCESS;
        }
    return RTOW_ERROR_INVALID_VALUE;
}

RTOW_API int rtowRecordPathsDevice(RtowContext ctx, const RtowSampleParams* batch, const RtowRecordPathsParams* params, const RtowPixelList* list, const float* inColor,
                                   const float* inSampleCountWeight, RtowPathSummary* summaries, RtowPathSegment* segments, void* stream)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    RTOW_TRY(validateRecordPaths(batch, params, list, inColor, inSampleCountWeight, summaries, segments));
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->haveScene) return RTOW_ERROR_NO_SCENE;
    const uint32_t kind = ctx->scene.layout.sceneKind;
    if (kind == SCENE_KIND_VOLUMES || kind == SCENE_KIND_VOLUMES_TEXTURED) return RTOW_ERROR_UNSUPPORTED;      // the volume branch needs every hit of a ray
    // the batch planner's arguments for these params - scene, textures, cubemap, the noise set (RTOW_ERROR_INVALID_VALUE: not uploaded) - and nothing of a batch's state:
    // no event, no counter, no cost map, no threshold probe, no hit-list spill
    SampleKernelArgs a{};
    const RtowAccumBuffers in{const_cast<float*>(inColor), nullptr, nullptr, const_cast<float*>(inSampleCountWeight)}, out{};
    RTOW_TRY(buildArgs(ctx, batch, &in, &out, nullptr, false, nullptr, nullptr, a));
    if (list->capacity == 0u) return RTOW_SUCCESS;
    hipStream_t s;
    RTOW_TRY(useDevice(ctx, stream, &s));
    // without `segments` the lanes' stacks live in the context's block: grow-only, allocated here on first use (freeing the smaller block waits for a launch that uses it)
    if (!segments) RTOW_TRY(growDevice(ctx, {{&ctx->dPathStack, (size_t)list->capacity * (size_t)batch->traceDepth * 24u}}));
    HIP_TRY(ctx, launchRecordPaths(a, queryScene(ctx), *params, list->words, list->capacity, summaries, segments, segments ? nullptr : ctx->dPathStack.get(), s),
            RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowGetLastSampleKernelMs(RtowContext ctx, float* outMs)
{
    if (!ctx || !outMs) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->haveTiming) return RTOW_ERROR_INVALID_VALUE;
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    HIP_TRY(ctx, hipEventSynchronize(ctx->evStop), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipEventElapsedTime(outMs, ctx->evStart, ctx->evStop), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowSamplePixelsDevice(RtowContext ctx, int32_t count, const RtowSampleParams* params, const RtowPixelList* list, const RtowAccumBuffers* in,
                                    const RtowAccumBuffers* out, void* const* diagnostics, void* stream, const volatile uint8_t* cancel)
{
    if (!out || !list || !list->words || count > kMaxChain) return RTOW_ERROR_INVALID_VALUE;
    std::unique_lock<std::mutex> lock;
    hipStream_t s;
    const auto check = [&](int b) {
        const RtowSampleParams& q = params[b];
        if ((int64_t)(int)q.size.x * (int)q.size.y > RTOW_PIXEL_LIST_MAX_PIXELS) return (int)RTOW_ERROR_INVALID_VALUE;     // an entry keeps the batch number above bit 27
        if (q.sliceOffset != 0 || q.sliceDivider != 1) return (int)RTOW_ERROR_INVALID_VALUE;                                // the list alone says which pixels
        if ((int)q.size.x != (int)params[0].size.x || (int)q.size.y != (int)params[0].size.y) return (int)RTOW_ERROR_INVALID_VALUE;      // one list, one frame
        return (int)RTOW_SUCCESS;
    };
    RTOW_TRY(beginSample(ctx, lock, count, params, in, out, check, stream, &s));
    // what has no list-capable kernel (REDO_CAPABLE, rtow_sample_kernel.hip.h), and what those kernels would not reproduce: nothing is enqueued
    const uint32_t kind = ctx->scene.layout.sceneKind;
    if (kind > SCENE_KIND_SPHERES_MOTION && !triangleKind(kind)) return RTOW_ERROR_UNSUPPORTED;
    if (ctx->flags & RTOW_CONTEXT_EXACT_TIES_NEVER) return RTOW_ERROR_UNSUPPORTED;
    for (int b = 0; b < count; b++)
        if (params[b].rngPolicy != RTOW_RNG_REFERENCE) return RTOW_ERROR_UNSUPPORTED;
    const ListSpec spec{list->words, list->capacity};
    return enqueueBatches(ctx, count, params, in, out, diagnostics, false, canFuse(ctx, count, params, diagnostics, /*handOver*/ false, false), s, cancel, &spec);
}

RTOW_API int rtowDeviceAlloc(RtowContext ctx, size_t sizeInBytes, void** outPointer)
{
    if (!ctx || !outPointer || sizeInBytes == 0) return RTOW_ERROR_INVALID_VALUE;
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    HIP_TRY(ctx, hipMalloc(outPointer, sizeInBytes), RTOW_ERROR_MEMORY_ALLOCATION);
    return RTOW_SUCCESS;
}

RTOW_API int rtowDeviceFree(RtowContext ctx, void* pointer)
{
    if (!ctx || !pointer) return RTOW_ERROR_INVALID_VALUE;
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    HIP_TRY(ctx, hipFree(pointer), RTOW_ERROR_INVALID_VALUE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowDeviceCopy(RtowContext ctx, const void* source, void* destination, size_t sizeInBytes, int kind)
{
    if (!ctx || !source || !destination) return RTOW_ERROR_INVALID_VALUE;
    hipMemcpyKind k;
    switch (kind) {
        case RTOW_MEMCPY_HOST_TO_HOST: k = hipMemcpyHostToHost; break;
        case RTOW_MEMCPY_HOST_TO_DEVICE: k = hipMemcpyHostToDevice; break;
        case RTOW_MEMCPY_DEVICE_TO_HOST: k = hipMemcpyDeviceToHost; break;
        case RTOW_MEMCPY_DEVICE_TO_DEVICE: k = hipMemcpyDeviceToDevice; break;
        default: return RTOW_ERROR_INVALID_VALUE;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipMemcpy(destination, source, sizeInBytes, k), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowDeviceMemset(RtowContext ctx, void* pointer, int value, size_t sizeInBytes)
{
    if (!ctx || !pointer) return RTOW_ERROR_INVALID_VALUE;
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    HIP_TRY(ctx, hipMemsetAsync(pointer, value, sizeInBytes, ctx->stream), RTOW_ERROR_LAUNCH_FAILURE);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), RTOW_ERROR_LAUNCH_FAILURE);
    return RTOW_SUCCESS;
}

RTOW_API int rtowGetBatchStatus(RtowContext ctx)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    // the last batch may have been enqueued on a caller's stream: its end is evBatchDone, not the end of ctx->stream
    if (ctx->haveBatchDone) HIP_TRY(ctx, hipEventSynchronize(ctx->evBatchDone), RTOW_ERROR_LAUNCH_FAILURE);
    return takeOverflow(ctx);
}

RTOW_API int rtowSynchronize(RtowContext ctx)
{
    if (!ctx) return RTOW_ERROR_INVALID_VALUE;
    std::lock_guard<std::mutex> lock(ctx->mu);
    HIP_TRY(ctx, hipSetDevice(ctx->device), RTOW_ERROR_NO_DEVICE);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream), RTOW_ERROR_LAUNCH_FAILURE);
    if (ctx->haveBatchDone) HIP_TRY(ctx, hipEventSynchronize(ctx->evBatchDone), RTOW_ERROR_LAUNCH_FAILURE);
    return takeOverflow(ctx);
}

} // extern "C"
