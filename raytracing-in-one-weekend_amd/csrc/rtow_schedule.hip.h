// rtow_schedule.hip.h - the kernels that decide the order in which a launch hands out its work, and their host launchers: the launch order of the 64-pixel
// ticket chunks (launchBuildChunkOrder) and the ticket map - which pixels share a wave (launchInitTicketMap, launchRegroupTickets).  None of them changes a
// result, only which lane renders which pixel and when.
//
// Inside the library this header is included by rtow_kernels.hip ALONE (the launchers below are ordinary external definitions, declared in rtow_kernels.h: a
// second translation unit of the library that included it would define them twice).  tests/native/schedule_parity.hip includes it too, as a library of its own,
// and runs the launchers over caller-supplied costs and maps; tests/test_gpu_schedule.py compares what comes back with tests/schedule_reference.py.
#pragma once
#include "rtow_kernels.h"

namespace rtow {

namespace {

// Launch order of the 64-pixel ticket chunks: most expensive first (longest-processing-time-first), from the per-chunk ray
// counts of the previous launch.  Counting sort on a 1024-bucket quantisation of the cost; the order inside a bucket is
// arbitrary - it only changes which lane renders which pixel, never a result.
constexpr int kOrderBuckets = 1024;
constexpr unsigned kOrderSingleBlockChunks = 65536u;      // beyond this many chunks the order is built by several workgroups (order_*_kernel)
static_assert(kChunkOrderScratchWords >= kOrderBuckets + 1, "histogram + maximum");
// cost[0..n) = ray count per chunk, cost[n..2n) = ray count of the chunk's most expensive pixel.  byMax: order by the most
// expensive pixel first (what decides when the last lanes retire), ties by the chunk total; otherwise by the total (used for
// the 1-sample probe, whose per-pixel counts are too noisy).
__device__ __forceinline__ float chunk_key(const unsigned* cost, unsigned n, unsigned i, int byMax)
{
    return byMax ? (float)cost[n + i] * 64.0f + (float)cost[i] * (1.0f / 64.0f) : (float)cost[i];
}

// pixelCost[64 * chunk .. +63] -> cost[chunk] = sum, cost[n + chunk] = max; one wave per chunk
__global__ void __launch_bounds__(256) reduce_chunk_cost_kernel(const unsigned short* __restrict__ pixelCost, unsigned n, unsigned* __restrict__ cost)
{
    const unsigned chunk = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (chunk >= n) return;
    unsigned v = pixelCost[(size_t)chunk * 64u + (threadIdx.x & 63u)];
    unsigned sum = v, mx = v;
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_xor(sum, off, 64);
        const unsigned o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63u) == 0) { cost[chunk] = sum; cost[n + chunk] = mx; }
}
__global__ void __launch_bounds__(1024) build_chunk_order_kernel(const unsigned* __restrict__ cost, unsigned n, unsigned* __restrict__ order, int byMax)
{
    __shared__ unsigned hist[kOrderBuckets];
    __shared__ unsigned maxKeyBits;
    const unsigned t = threadIdx.x;
    hist[t] = 0;
    if (t == 0) maxKeyBits = __float_as_uint(1.0f);
    __syncthreads();
    float m = 0;
    for (unsigned i = t; i < n; i += 1024) m = fmaxf(m, chunk_key(cost, n, i, byMax));
    atomicMax(&maxKeyBits, __float_as_uint(m));                     // non-negative floats order like their bit patterns
    __syncthreads();
    const float scale = (float)(kOrderBuckets - 1) / __uint_as_float(maxKeyBits);
    for (unsigned i = t; i < n; i += 1024) atomicAdd(&hist[(kOrderBuckets - 1) - (unsigned)(chunk_key(cost, n, i, byMax) * scale)], 1u);   // bucket 0 = most expensive
    __syncthreads();
    if (t == 0) {
        unsigned run = 0;
        for (int b = 0; b < kOrderBuckets; b++) { const unsigned c = hist[b]; hist[b] = run; run += c; }
    }
    __syncthreads();
    for (unsigned i = t; i < n; i += 1024) order[atomicAdd(&hist[(kOrderBuckets - 1) - (unsigned)(chunk_key(cost, n, i, byMax) * scale)], 1u)] = i;
}

// The same order over several workgroups, for launches of hundreds of thousands of chunks (the per-sample policies' units at 1080p: 518 400 chunks, 0.67 ms in the one
// workgroup above = 1.1 % of a batch): maximum, histogram, prefix and scatter as four small launches over a 1 025-word scratch behind the cost array
// (scratch[0 .. 1023] = histogram / cursors, scratch[1024] = bits of the largest key).  Same buckets, same (unspecified) order inside a bucket.
__global__ void __launch_bounds__(256) order_max_kernel(const unsigned* __restrict__ cost, unsigned n, int byMax, unsigned* __restrict__ scratch)
{
    float m = 1.0f;                                                  // (the single-workgroup kernel starts from 1 too)
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) m = fmaxf(m, chunk_key(cost, n, i, byMax));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    if ((threadIdx.x & 63u) == 0) atomicMax(scratch + kOrderBuckets, __float_as_uint(m));
}
// (a workgroup counts its 2 048 chunks in LDS and touches every global bucket once: the keys of a launch crowd into a few buckets - per-sample units cost alike - and half a
// million global atomics on a handful of addresses took longer than the single workgroup they were meant to replace)
constexpr unsigned kOrderChunksPerBlock = 2048u;
__global__ void __launch_bounds__(256) order_hist_kernel(const unsigned* __restrict__ cost, unsigned n, int byMax, unsigned* __restrict__ scratch)
{
    __shared__ unsigned hist[kOrderBuckets];
    for (unsigned b = threadIdx.x; b < (unsigned)kOrderBuckets; b += 256u) hist[b] = 0u;
    __syncthreads();
    const float scale = (float)(kOrderBuckets - 1) / __uint_as_float(scratch[kOrderBuckets]);
    const unsigned first = blockIdx.x * kOrderChunksPerBlock, last = first + kOrderChunksPerBlock < n ? first + kOrderChunksPerBlock : n;
    for (unsigned i = first + threadIdx.x; i < last; i += 256u) atomicAdd(&hist[(kOrderBuckets - 1) - (unsigned)(chunk_key(cost, n, i, byMax) * scale)], 1u);
    __syncthreads();
    for (unsigned b = threadIdx.x; b < (unsigned)kOrderBuckets; b += 256u) if (hist[b]) atomicAdd(&scratch[b], hist[b]);
}
__global__ void __launch_bounds__(1024) order_prefix_kernel(unsigned* __restrict__ scratch)
{
    __shared__ unsigned sums[kOrderBuckets];
    const unsigned t = threadIdx.x, c = scratch[t];
    sums[t] = c;
    __syncthreads();
    for (unsigned d = 1; d < (unsigned)kOrderBuckets; d <<= 1) {      // inclusive scan
        const unsigned v = t >= d ? sums[t - d] : 0u;
        __syncthreads();
        sums[t] += v;
        __syncthreads();
    }
    scratch[t] = sums[t] - c;                                          // exclusive: where bucket t starts
}
__global__ void __launch_bounds__(256) order_scatter_kernel(const unsigned* __restrict__ cost, unsigned n, int byMax, unsigned* __restrict__ scratch, unsigned* __restrict__ order)
{
    __shared__ unsigned hist[kOrderBuckets];       // this workgroup's count per bucket, then its cursor inside the range it reserved in that bucket
    for (unsigned b = threadIdx.x; b < (unsigned)kOrderBuckets; b += 256u) hist[b] = 0u;
    __syncthreads();
    const float scale = (float)(kOrderBuckets - 1) / __uint_as_float(scratch[kOrderBuckets]);
    const unsigned first = blockIdx.x * kOrderChunksPerBlock, last = first + kOrderChunksPerBlock < n ? first + kOrderChunksPerBlock : n;
    for (unsigned i = first + threadIdx.x; i < last; i += 256u) atomicAdd(&hist[(kOrderBuckets - 1) - (unsigned)(chunk_key(cost, n, i, byMax) * scale)], 1u);
    __syncthreads();
    for (unsigned b = threadIdx.x; b < (unsigned)kOrderBuckets; b += 256u) if (hist[b]) hist[b] = atomicAdd(&scratch[b], hist[b]);      // reserve; hist[b] = where this workgroup's share starts
    __syncthreads();
    for (unsigned i = first + threadIdx.x; i < last; i += 256u) order[atomicAdd(&hist[(kOrderBuckets - 1) - (unsigned)(chunk_key(cost, n, i, byMax) * scale)], 1u)] = i;
}

// ------------------------------------------------------------------------------------------------------------
// Which pixels share a wave (SampleKernelArgs.ticketMap).  A chunk's 64 tickets go to the 64 lanes of one wave; numbered in tiles they are an 8 x 8 block of the image - but a tile on
// a sphere's edge holds sky pixels (one ray per sample), ground pixels and glass pixels, whose lanes wait for each other's stages.  The reference hands pixels out in no
// defined order (Schedule(W * H, 1), UNITY/Raytracer.cs:730), so the numbering is free: per super-tile of side x side tiles this kernel sorts the super-tile's pixels by the ray
// count the last launch measured for them - most expensive first; equal counts (sky: exactly one ray per sample) keep their tile order - and deals them out to the super-tile's own
// chunks 64 at a time.  A super-tile's accumulator lines stay with the few CUs that take its chunks.  One workgroup per super-tile, bitonic sort in LDS of
// (cost + 1) << 32 | owned-pixel number (0 = padding).  In place: ticketMap and pixelCost (permuted along, so that it stays in ticket order under the new map).
// ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) init_ticket_map_kernel(unsigned* __restrict__ map, unsigned n)
{
    const unsigned i = blockIdx.x * 1024u + threadIdx.x;
    if (i < n) map[i] = i;
}
__global__ void __launch_bounds__(1024) regroup_tickets_kernel(unsigned short* __restrict__ pixelCost, unsigned* __restrict__ ticketMap, unsigned tilesPerRow, unsigned tileRows, unsigned side,
                                                              unsigned t1, unsigned t2, unsigned t3)
{
    extern __shared__ unsigned long long regroupKeys[];
    const unsigned perRow = (tilesPerRow + side - 1u) / side;
    const unsigned sty = blockIdx.x / perRow, stx = blockIdx.x - sty * perRow;
    const unsigned tx0 = stx * side, ty0 = sty * side;
    const unsigned w = tilesPerRow - tx0 < side ? tilesPerRow - tx0 : side, h = tileRows - ty0 < side ? tileRows - ty0 : side;
    const unsigned n = w * h * 64u;
    unsigned N = 64u;
    while (N < n) N <<= 1;
    auto ticketOf = [&](unsigned e) { const unsigned k = e >> 6, ky = k / w, kx = k - ky * w; return ((ty0 + ky) * tilesPerRow + tx0 + kx) * 64u + (e & 63u); };
    for (unsigned e = threadIdx.x; e < N; e += 1024u) {
        unsigned long long key = 0ull;
        if (e < n) {
            const unsigned t = ticketOf(e);
            const unsigned cost = pixelCost[t];
            // key = primary << 48 | owned-pixel number << 16 | cost: the primary key is the ray count itself (t1 == 0) or its class (cost classes t1 < t2 < t3: sky only / ... ),
            // equal primaries keep their tile order, the ray count travels along
            const unsigned primary = t1 == 0u ? cost + 1u : 1u + (cost > t1 ? 1u : 0u) + (cost > t2 ? 1u : 0u) + (cost > t3 ? 1u : 0u);
            // (the sort is descending: the pixel number goes in complemented, so that equal primaries come out in ASCENDING pixel order - their tile order)
            key = ((unsigned long long)(primary > 0xffffu ? 0xffffu : primary) << 48) | ((unsigned long long)(0xffffffffu - ticketMap[t]) << 16) | (unsigned long long)cost;
        }
        regroupKeys[e] = key;
    }
    __syncthreads();
    for (unsigned k = 2u; k <= N; k <<= 1) {
        for (unsigned j = k >> 1; j > 0u; j >>= 1) {
            for (unsigned e = threadIdx.x; e < N; e += 1024u) {
                const unsigned p = e ^ j;
                if (p > e) {
                    const unsigned long long a = regroupKeys[e], b = regroupKeys[p];
                    const bool descending = (e & k) == 0u;                       // the whole array ends up descending: padding (0) last
                    if (descending ? a < b : a > b) { regroupKeys[e] = b; regroupKeys[p] = a; }
                }
            }
            __syncthreads();
        }
    }
    for (unsigned e = threadIdx.x; e < n; e += 1024u) {
        const unsigned long long key = regroupKeys[e];
        const unsigned t = ticketOf(e);
        ticketMap[t] = 0xffffffffu - (unsigned)(key >> 16);
        pixelCost[t] = (unsigned short)(key & 0xffffull);
    }
}

// The same map with the tiles left as they are: only the ORDER of a tile's 64 tickets changes - most expensive pixel first.  A wave's lanes take the tickets of its chunk one by one
// as they finish their previous pixels (the first tickets go within microseconds, the last ones when the slowest lanes of the previous chunk are done, a pixel-time later), so a chunk's
// expensive pixel that happens to be its 60th ticket starts tens of milliseconds after the chunk was handed out - and ends the launch.  The wave still traces the same 64 neighbours.
// One wave per tile: 64 keys (cost + 1) << 32 | owned-pixel number, bitonic sort through cross-lane moves, descending.
__global__ void __launch_bounds__(256) order_tile_tickets_kernel(unsigned short* __restrict__ pixelCost, unsigned* __restrict__ ticketMap, unsigned tiles, unsigned levels)
{
    const unsigned tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= tiles) return;
    const unsigned t = tile * 64u + lane;
    const unsigned cost = pixelCost[t], pixel = ticketMap[t];
    // primary key: the ray count itself (levels == 0), or its level among `levels` equal parts of the tile's range [0, max] - pixels of one level keep the order they had, so
    // that a tile of like pixels (all sky; a patch of ground) is still taken row by row and its accumulator lines are touched once, and only the pixels that stand out move to the front
    unsigned top = cost;
    for (int off = 32; off > 0; off >>= 1) { const unsigned o = (unsigned)__shfl_xor((int)top, off, 64); top = o > top ? o : top; }
    const unsigned primary = levels ? (cost * levels) / (top + 1u) : cost;
    unsigned key = (primary << 12) | ((63u - lane) << 6) | lane;                 // descending: higher level first, then the earlier place; the low six bits say where the element came from
    for (unsigned k = 2u; k <= 64u; k <<= 1) {
        for (unsigned j = k >> 1; j > 0u; j >>= 1) {
            const unsigned other = (unsigned)__shfl_xor((int)key, (int)j, 64);
            const bool upper = (lane & j) != 0u;                                 // this lane holds the later element of the pair
            const bool descending = (lane & k) == 0u;
            const bool keepLarger = descending != upper;                         // the earlier place of a descending run keeps the larger key
            key = keepLarger ? (key > other ? key : other) : (key < other ? key : other);
        }
    }
    const int from = (int)(key & 63u);
    ticketMap[t] = (unsigned)__shfl((int)pixel, from, 64);
    pixelCost[t] = (unsigned short)__shfl((int)cost, from, 64);
}

} // namespace

hipError_t launchBuildChunkOrder(const unsigned short* pixelCost, unsigned* cost, unsigned chunkCount, unsigned* order, int byMax, hipStream_t stream)
{
    hipLaunchKernelGGL(reduce_chunk_cost_kernel, dim3((chunkCount + 3u) / 4u), dim3(256), 0, stream, pixelCost, chunkCount, cost);
    if (chunkCount > kOrderSingleBlockChunks) {
        unsigned* scratch = cost + 2u * (size_t)chunkCount;            // kChunkOrderScratchWords behind the two cost columns (rtow_api.hip allocates them)
        const unsigned blocks = (chunkCount + kOrderChunksPerBlock - 1u) / kOrderChunksPerBlock;        // order_hist / order_scatter: one workgroup per 2 048 chunks
        hipError_t e = hipMemsetAsync(scratch, 0, (size_t)kChunkOrderScratchWords * sizeof(unsigned), stream);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(order_max_kernel, dim3(blocks), dim3(256), 0, stream, cost, chunkCount, byMax, scratch);
        hipLaunchKernelGGL(order_hist_kernel, dim3(blocks), dim3(256), 0, stream, cost, chunkCount, byMax, scratch);
        hipLaunchKernelGGL(order_prefix_kernel, dim3(1), dim3(1024), 0, stream, scratch);
        hipLaunchKernelGGL(order_scatter_kernel, dim3(blocks), dim3(256), 0, stream, cost, chunkCount, byMax, scratch, order);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(build_chunk_order_kernel, dim3(1), dim3(1024), 0, stream, cost, chunkCount, order, byMax);
    return hipGetLastError();
}

hipError_t launchInitTicketMap(unsigned* ticketMap, unsigned count, hipStream_t stream)
{
    if (count == 0u) return hipSuccess;
    hipLaunchKernelGGL(init_ticket_map_kernel, dim3((count + 1023u) / 1024u), dim3(1024), 0, stream, ticketMap, count);
    return hipGetLastError();
}
hipError_t launchRegroupTickets(unsigned short* pixelCost, unsigned* ticketMap, unsigned tilesPerRow, unsigned tileRows, unsigned side, const unsigned classes[3], hipStream_t stream)
{
    if (tilesPerRow == 0u || tileRows == 0u) return hipSuccess;
    if (side == 1u) {                                                            // the tiles as they are, their tickets most expensive first
        const unsigned tiles = tilesPerRow * tileRows;
        hipLaunchKernelGGL(order_tile_tickets_kernel, dim3((tiles + 3u) / 4u), dim3(256), 0, stream, pixelCost, ticketMap, tiles, classes[0]);      // classes[0]: levels (0 = by the ray count itself)
        return hipGetLastError();
    }
    if (side < 2u || side > kRegroupMaxSide) return hipErrorInvalidValue;
    const unsigned blocks = ((tilesPerRow + side - 1u) / side) * ((tileRows + side - 1u) / side);
    unsigned N = 64u;
    while (N < side * side * 64u) N <<= 1;
    hipLaunchKernelGGL(regroup_tickets_kernel, dim3(blocks), dim3(1024), (size_t)N * sizeof(unsigned long long), stream, pixelCost, ticketMap, tilesPerRow, tileRows, side, classes[0], classes[1], classes[2]);
    return hipGetLastError();
}

} // namespace rtow
