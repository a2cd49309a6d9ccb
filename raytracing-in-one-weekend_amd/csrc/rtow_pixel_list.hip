// rtow_pixel_list.hip - pixel lists for rtowSamplePixelsDevice: rtowBuildPixelListDevice's kernels (which pixels of a frame qualify, in a deterministic order that
// suits the sample kernel's 64-ticket pulls) and the filter that copies a caller's list into the context's own, dropping entries that name no pixel of the frame.  The
// specification is in include/rtow.h next to RtowPixelListParams (and DESIGN.md 5); tests/pixel_list_reference.py restates it in numpy and the GPU tests compare the
// two word for word.
//
// Launch shape: both are a stable compaction of "units" of 64 candidates - the builder's unit is an 8 x 8 pixel tile (a wave per tile, lane =
// (lane & 7, lane >> 3) as rtowTraceViewDevice maps them), the filter's is 64 consecutive entries - in three plain launches, in stream order:
//   count   one wave per unit: __ballot of the predicate, popcount -> counts[unit]
//   scan    one workgroup: exclusive scan of counts in place, 1024 at a time with a running carry; the total goes to words[0], zeros to words[1..3]
//   write   one wave per unit again: the same predicate, the entry goes to words[4 + counts[unit] + rank], rank = lanes below in the ballot (mbcnt), if below capacity
// No kernel waits for another workgroup (no decoupled look-back, no flags), nothing is allocated, no atomic is used: the order is the units' order, whatever the
// hardware does.  The builder visits only the tiles its rectangle touches.  The scan is one workgroup on purpose: 32 400 tiles (1920 x 1080) are 32 rounds of it.
#include "rtow_kernels.h"

namespace rtow {

namespace {

constexpr int kListBlock = 256;                      // four units
constexpr unsigned kListMaxBlocks = 4096;            // units beyond four times this are walked by the grid-stride loop
constexpr int kScanBlock = 1024;

struct PixelListArgs {
    // the builder's predicate: frame, rectangle clamped to it, slice, count bound, inputs (null: not tested)
    int width;
    int x0, y0, x1, y1;
    unsigned sliceOffset, sliceDivider;
    float minSampleCount;
    const float* color;
    const uint8_t* mask;
    unsigned tileX0, tileY0, tilesX;    // first tile the rectangle touches, tiles per row of tiles it touches
    // the filter's: a caller's list and how many pixels its frame has
    const unsigned* source;
    unsigned sourceCapacity, framePixels;
    // both
    unsigned units;
    unsigned* counts;                   // [units]: count, then (scan) the unit's first place in the list
    unsigned* words;                    // the list written
    unsigned capacity;
};

// whether candidate `lane` of `unit` goes into the list, and as which entry
template <bool FILTER>
__device__ __forceinline__ bool candidate(const PixelListArgs& A, unsigned unit, unsigned lane, unsigned& entry)
{
    entry = 0u;
    if (FILTER) {
        const unsigned listed = A.source[0];
        const unsigned n = listed < A.sourceCapacity ? listed : A.sourceCapacity;
        const size_t i = (size_t)unit * 64u + lane;
        if (i >= n) return false;
        entry = A.source[4u + i];
        return entry < A.framePixels;                   // an entry beyond the frame is dropped here: the sample kernel never sees it
    }
    const int x = (int)((A.tileX0 + unit % A.tilesX) * 8u + (lane & 7u));
    const int y = (int)((A.tileY0 + unit / A.tilesX) * 8u + (lane >> 3));
    if (x < A.x0 || x >= A.x1 || y < A.y0 || y >= A.y1) return false;
    if ((unsigned)y % A.sliceDivider != A.sliceOffset) return false;
    const size_t p = (size_t)y * (size_t)A.width + (size_t)x;
    entry = (unsigned)p;
    if (A.mask && A.mask[p] == 0) return false;
    if (A.color && A.color[4u * p + 3u] >= A.minSampleCount) return false;          // (a NaN count fails the comparison: it qualifies)
    return true;
}

template <bool FILTER>
__global__ void __launch_bounds__(kListBlock) pixel_list_count_kernel(PixelListArgs A)
{
    const unsigned stride = gridDim.x * (kListBlock / 64), lane = threadIdx.x & 63u;
    for (unsigned unit = blockIdx.x * (kListBlock / 64) + (threadIdx.x >> 6); unit < A.units; unit += stride) {      // (unit is the same in every lane of a wave)
        unsigned entry;
        const unsigned long long in = __ballot(candidate<FILTER>(A, unit, lane, entry));
        if (lane == 0u) A.counts[unit] = (unsigned)__popcll(in);
    }
}

__global__ void __launch_bounds__(kScanBlock) pixel_list_scan_kernel(unsigned* counts, unsigned units, unsigned* words)
{
    __shared__ unsigned waveSum[kScanBlock / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned running = 0u;                                       // every lane keeps the same value
    for (unsigned base = 0u; base < units; base += kScanBlock) {
        const unsigned i = base + tid;
        const unsigned v = i < units ? counts[i] : 0u;
        unsigned s = v;                                          // inclusive scan inside the wave
        for (unsigned d = 1u; d < 64u; d <<= 1) { const unsigned t = __shfl_up(s, d); if (lane >= d) s += t; }
        if (lane == 63u) waveSum[wave] = s;
        __syncthreads();
        unsigned before = 0u, total = 0u;
        for (unsigned k = 0u; k < kScanBlock / 64; ++k) { const unsigned w = waveSum[k]; before += k < wave ? w : 0u; total += w; }
        if (i < units) counts[i] = running + before + (s - v);
        running += total;                                        // at most 2^27 in all (the frame's pixels; a list's capacity for the filter)
        __syncthreads();
    }
    if (tid < 4u) words[tid] = tid == 0u ? running : 0u;
}

template <bool FILTER>
__global__ void __launch_bounds__(kListBlock) pixel_list_write_kernel(PixelListArgs A)
{
    const unsigned stride = gridDim.x * (kListBlock / 64), lane = threadIdx.x & 63u;
    for (unsigned unit = blockIdx.x * (kListBlock / 64) + (threadIdx.x >> 6); unit < A.units; unit += stride) {
        unsigned entry;
        const bool ok = candidate<FILTER>(A, unit, lane, entry);
        const unsigned long long in = __ballot(ok);
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(in >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)in, 0u));
        const unsigned place = A.counts[unit] + rank;            // below 2^27 + 64: no wrap
        if (ok && place < A.capacity) A.words[4u + (size_t)place] = entry;
    }
}

template <bool FILTER>
hipError_t compact(const PixelListArgs& A, hipStream_t stream)
{
    const unsigned groups = (A.units + kListBlock / 64 - 1) / (kListBlock / 64);
    const dim3 grid(groups < kListMaxBlocks ? groups : kListMaxBlocks), block(kListBlock);
    if (A.units) hipLaunchKernelGGL(pixel_list_count_kernel<FILTER>, grid, block, 0, stream, A);        // (a grid of zero workgroups is not a valid launch)
    hipLaunchKernelGGL(pixel_list_scan_kernel, dim3(1), dim3(kScanBlock), 0, stream, A.counts, A.units, A.words);
    if (A.units && A.capacity) hipLaunchKernelGGL(pixel_list_write_kernel<FILTER>, grid, block, 0, stream, A);
    return hipGetLastError();
}

}  // namespace

hipError_t launchBuildPixelList(const RtowPixelListParams& p, const float* color, const uint8_t* mask, unsigned* scratch, unsigned* words, unsigned capacity, hipStream_t stream)
{
    PixelListArgs A{};
    A.width = p.width;
    A.x0 = p.x0 > 0 ? p.x0 : 0; A.x1 = p.x1 < p.width ? p.x1 : p.width;
    A.y0 = p.y0 > 0 ? p.y0 : 0; A.y1 = p.y1 < p.height ? p.y1 : p.height;
    A.sliceOffset = (unsigned)p.sliceOffset; A.sliceDivider = (unsigned)p.sliceDivider;
    A.minSampleCount = p.minSampleCount;
    A.color = color; A.mask = mask;
    if (A.x0 < A.x1 && A.y0 < A.y1) {
        A.tileX0 = (unsigned)A.x0 / 8u; A.tileY0 = (unsigned)A.y0 / 8u;
        A.tilesX = ((unsigned)A.x1 + 7u) / 8u - A.tileX0;
        A.units = A.tilesX * (((unsigned)A.y1 + 7u) / 8u - A.tileY0);          // at most the frame's tiles: RTOW_PIXEL_LIST_SCRATCH_BYTES
    }
    A.counts = scratch; A.words = words; A.capacity = capacity;
    return compact<false>(A, stream);
}

hipError_t launchFilterPixelList(const unsigned* source, unsigned capacity, unsigned framePixels, unsigned* scratch, unsigned* words, hipStream_t stream)
{
    PixelListArgs A{};
    A.source = source; A.sourceCapacity = capacity; A.framePixels = framePixels;
    A.units = (unsigned)(((uint64_t)capacity + 63u) / 64u);
    A.counts = scratch; A.words = words; A.capacity = capacity;
    return compact<true>(A, stream);
}

}  // namespace rtow
