// rtow_rectify_history.hip - rtowRectifyHistoryDevice: what deals with carried history that is WRONG.  rtowReprojectAccumDevice and rtowReprojectMomentsDevice carry a
// pixel's sums across a camera move by where its first hit was; a mirror, a glass sphere or a defocused edge shows something else from the new position, and up to
// maxHistory stale samples then sit under a handful of new ones.  After the first batches of the new view exist this pass compares each pixel's carried mean luminance
// with the statistics of the NEW samples in its guide-weighted neighbourhood - the variance clipping of temporal anti-aliasing, the history rejection of A-SVGF - and
// where the two disagree it scales the history down to the weight the disagreement allows, or drops it (all zeros: a hole the list builder and
// rtowEstimateMomentsDevice already treat).  The numeric specification is in include/rtow.h next to the entry point (and DESIGN.md 5);
// tests/rectify_history_reference.py restates it in numpy and the GPU tests compare the two bit for bit.
//
// Launch shape.  The 64 x 4 pixel workgroup tile and grid-stride tile loop of estimate_moments_kernel; a wave is 64 pixels of one row.  A workgroup
// first asks whether any of its pixels has a valid history: a tile of holes copies through (writes nothing but outKeep in place) and reads neither the fresh colour nor
// the guides.  Otherwise it stages the part of its 70 x 10 halo region that `radius` reaches into LDS once - L(q) of the fresh colour and the guides - and the
// (2 r + 1)^2 taps run from there: the staging and the tap loop of rtow_guided_halo.hip.h, which estimate_moments_kernel shares.  A lane reads history and moments
// at its own pixel only, before it writes them: every output may be the matching input.  Statistics are integers (rtow_noise_mask.hip): counts by wave ballot into
// LDS, and when the workgroup is through with its tiles one global atomic per non-zero counter; none at all without outStats.
#include "rtow_kernels.h"
#include "rtow_guided_halo.hip.h"

namespace rtow {

namespace {

using namespace taps;

// Tiles beyond this many workgroups are walked by the grid-stride loop, and a workgroup adds its counts to the record once, when it is through: the memory side takes
// device-wide atomics on one cache line one after the other (rtow_noise_mask.hip measured 0.1 ms per 1000 workgroups of some 20 atomics).  2048 workgroups are the
// 8 x 256 a device holds at once; at most four atomics each.
constexpr unsigned kMaxBlocks = 2048;

// the words of the record (RtowRectifyStats)
enum : unsigned { kJudged = 0, kKept = 1, kCut = 2, kDropped = 3 };
static_assert(sizeof(RtowRectifyStats) == 16 && sizeof(RtowRectifyParams) == 40, "the layouts of include/rtow.h");

struct RectifyArgs {
    int width, height;
    TileGrid grid;                      // the 64 x 4 pixel tiles
    int radius, minTaps, normalSharpness, matchEntity;
    float depthTolerance;
    float K2, R2;                       // sigmaScale^2, relativeTolerance^2
    const float *hColor, *hNormal, *hAlbedo, *hWeight;      // history
    const float* fresh;
    const float* distance;
    const int32_t* entity;
    const float* normal;
    const float* inMoments;
    float *oColor, *oNormal, *oAlbedo, *oWeight;
    float* outMoments;
    float* outKeep;
    unsigned* outStats;
};

// The kernel's one argument where it lies in the kernarg segment (a by-value struct starts at offset 0).  What a phase needs of it - the pointers of the staging, of the
// write phase and of the record, the band's constants - is read THERE, tile by tile: scalar loads the scalar cache serves.  Loaded once and held across the tap loop
// next to everything else, they do not fit the scalar registers of a wave at 8 waves per SIMD, and the compiler parks them in the lanes of a VGPR.  The empty asm
// keeps the loads where they are written; it emits nothing.
using KernelArgs = const RectifyArgs __attribute__((address_space(4)))*;
__device__ __forceinline__ KernelArgs args_here()
{
    KernelArgs K = (KernelArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(K));
    return K;
}

enum : int { kUnjudged = 0, kKeptPixel = 1, kCutPixel = 2, kDroppedPixel = 3 };

// what a pixel's outcome does to a float3 of its history (normal, albedo, moments) that is `out` at p: copied unless in place, scaled by k, or zeroed
__device__ __forceinline__ void write3(const float* in, float* out, size_t p, int outcome, float k)
{
    if (outcome < kCutPixel) {
        if (in != out) reinterpret_cast<P3*>(out)[p] = ld3(in, p);
        return;
    }
    P3 v{0.0f, 0.0f, 0.0f};
    if (outcome == kCutPixel) {
        v = ld3(in, p);
        v = P3{v.x * k, v.y * k, v.z * k};
    }
    reinterpret_cast<P3*>(out)[p] = v;
}

__global__ void __launch_bounds__(256, 8) rectify_history_kernel(RectifyArgs A)
{
    __shared__ float sL[halo::kHalo], sT[halo::kHalo], sNx[halo::kHalo], sNy[halo::kHalo], sNz[halo::kHalo];
    __shared__ int sE[halo::kHalo];
    __shared__ unsigned sCount[4];
    const halo::Planes planes{sL, sE, sT, sNx, sNy, sNz};
    const int lx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);
    if (threadIdx.x < 4) sCount[threadIdx.x] = 0u;          // the first barrier of the tile loop comes before any lane counts
    for (unsigned t = blockIdx.x; t < A.grid.tiles; t += gridDim.x) {          // the same tiles for every lane of the workgroup: the barriers below are uniform
        const int x0 = (int)(t % A.grid.tilesX) * kGroupW, y0 = (int)(t / A.grid.tilesX) * kGroupH;
        const int x = x0 + lx, y = y0 + ly;
        const bool inside = x < A.width && y < A.height;
        const size_t p = (size_t)y * (size_t)A.width + (size_t)x;
        P4 h{0.0f, 0.0f, 0.0f, 0.0f};
        float lh = 0.0f;
        bool valid = false;
        if (inside) {
            const KernelArgs K = args_here();
            h = reinterpret_cast<const P4*>(K->hColor)[p];
            if (__builtin_isfinite(h.x) && __builtin_isfinite(h.y) && __builtin_isfinite(h.z) && __builtin_isfinite(h.w) && h.w >= 1.0f) {
                lh = lum(h.x / h.w, h.y / h.w, h.z / h.w);
                valid = __builtin_isfinite(lh);
            }
        }
        int outcome = kUnjudged;
        float k = 1.0f, newW = 0.0f;
        // a barrier as well: every lane is through with the planes of the previous tile before they are staged again
        if (__syncthreads_or(valid ? 1 : 0)) {                            // else a tile of holes: no fresh colour, no guide is read
            const KernelArgs K = args_here();
            halo::stage(planes, x0, y0, A.width, A.height, A.radius, K->fresh, K->entity, K->distance, K->normal);
            __syncthreads();
            const int centre = halo::centre_of(lx, ly);
            if (valid && sL[centre] == sL[centre]) {                      // a pixel without a valid fresh L of its own is not judged
                const halo::Sums s = halo::neighbourhood(planes, centre, A.radius, A.matchEntity, A.depthTolerance, A.normalSharpness);
                if (s.taps >= A.minTaps) {
                    const float mu = s.S1 / s.W, b = s.S2 / s.W;
                    if (__builtin_isfinite(mu) && __builtin_isfinite(b)) {
                        const KernelArgs K = args_here();
                        float var = b - mu * mu;
                        var = var > 0.0f ? var : 0.0f;
                        const float d = lh - mu;
                        const float T = (K->K2 * var + K->R2 * (mu * mu)) + 0x1p-20f;
                        const float r = (d * d) / T;
                        outcome = kKeptPixel;
                        if (r > 1.0f) {                                   // a NaN r keeps
                            const float m = h.w / r;
                            newW = __builtin_truncf(m);
                            outcome = newW >= 1.0f ? kCutPixel : kDroppedPixel;
                            k = outcome == kCutPixel ? newW / h.w : 0.0f;
                        }
                    }
                }
            }
        }
        if (inside) {
            const KernelArgs K = args_here();
            const float *hNormal = K->hNormal, *hAlbedo = K->hAlbedo, *hWeight = K->hWeight, *inMoments = K->inMoments;
            float *oColor = K->oColor, *oNormal = K->oNormal, *oAlbedo = K->oAlbedo, *oWeight = K->oWeight, *outMoments = K->outMoments, *outKeep = K->outKeep;
            if (outcome < kCutPixel) {                                    // unchanged: bit for bit, nothing in place
                if (K->hColor != oColor) reinterpret_cast<P4*>(oColor)[p] = h;
                if (hWeight != oWeight) oWeight[p] = hWeight[p];
            } else {
                reinterpret_cast<P4*>(oColor)[p] = outcome == kCutPixel ? P4{h.x * k, h.y * k, h.z * k, newW} : P4{0.0f, 0.0f, 0.0f, 0.0f};
                oWeight[p] = outcome == kCutPixel ? hWeight[p] * k : 0.0f;
            }
            write3(hNormal, oNormal, p, outcome, k);
            write3(hAlbedo, oAlbedo, p, outcome, k);
            if (outMoments) write3(inMoments, outMoments, p, outcome, k);
            if (outKeep) outKeep[p] = k;
        }
        const KernelArgs K = args_here();
        if (K->outStats) {                                                // uniform: every lane of the wave votes
            const unsigned long long kb = __ballot(outcome == kKeptPixel), cb = __ballot(outcome == kCutPixel), db = __ballot(outcome == kDroppedPixel);
            if (lx == 0) {
                if (kb) atomicAdd(&sCount[kKept], (unsigned)__popcll(kb));
                if (cb) atomicAdd(&sCount[kCut], (unsigned)__popcll(cb));
                if (db) atomicAdd(&sCount[kDropped], (unsigned)__popcll(db));
            }
        }
    }
    const KernelArgs K = args_here();
    unsigned* const outStats = K->outStats;
    if (!outStats) return;
    __syncthreads();
    // the workgroup's statistics into the record: one global atomic per non-zero word
    if (threadIdx.x >= 1 && threadIdx.x < 4 && sCount[threadIdx.x]) atomicAdd(outStats + threadIdx.x, sCount[threadIdx.x]);
    if (threadIdx.x == 0) {
        const unsigned judged = sCount[kKept] + sCount[kCut] + sCount[kDropped];
        if (judged) atomicAdd(outStats + kJudged, judged);
    }
}

}  // namespace

hipError_t launchRectifyHistory(const RtowRectifyParams& p, const RtowAccumBuffers& history, const float* fresh, const RtowHitBuffers& hits, const float* inMoments,
                                const RtowAccumBuffers& out, float* outMoments, float* outKeep, RtowRectifyStats* outStats, hipStream_t stream)
{
    RectifyArgs A{};
    A.width = p.width;
    A.height = p.height;
    A.grid = tileGrid(p.width, p.height);
    A.radius = p.radius;
    A.minTaps = p.minTaps;
    A.normalSharpness = p.normalSharpness;
    A.matchEntity = (p.flags & RTOW_RECTIFY_MATCH_ENTITY) != 0;
    A.depthTolerance = p.depthTolerance;
    A.K2 = p.sigmaScale * p.sigmaScale;
    A.R2 = p.relativeTolerance * p.relativeTolerance;
    A.hColor = history.color; A.hNormal = history.normal; A.hAlbedo = history.albedo; A.hWeight = history.sampleCountWeight;
    A.fresh = fresh;
    A.distance = hits.distance;
    A.entity = hits.entityIndex;
    A.normal = hits.normal;
    A.inMoments = inMoments;
    A.oColor = out.color; A.oNormal = out.normal; A.oAlbedo = out.albedo; A.oWeight = out.sampleCountWeight;
    A.outMoments = outMoments;
    A.outKeep = outKeep;
    A.outStats = reinterpret_cast<unsigned*>(outStats);
    if (outStats) {
        const hipError_t e = hipMemsetAsync(outStats, 0, sizeof(RtowRectifyStats), stream);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(rectify_history_kernel, dim3(A.grid.tiles < kMaxBlocks ? A.grid.tiles : kMaxBlocks), dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace rtow
