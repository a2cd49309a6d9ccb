// rtow_noise_mask.hip - rtowNoiseMaskDevice: from the luminance moments (s1, s2, n) to the byte mask rtowBuildPixelListDevice accepts - the link between the variance a
// frame carries (rtowAccumulateMomentsDevice, rtowReprojectMomentsDevice, rtowEstimateMomentsDevice) and the list launches that spend samples on chosen pixels
// (rtowSamplePixelsDevice).  A pixel's error is the variance of its mean (relative to mean^2 + floor^2 unless ABSOLUTE), filtered by the 3 x 3 tent of
// rtowDenoiseVarianceDevice; it qualifies at or above a threshold, and the mask is the qualifying set dilated by 0..3 pixels.  A 288-byte record tells the host how many
// pixels qualify and how the error is distributed (64 bins, one per binade); with a budget the threshold is raised to the bin edge that keeps the qualifying count within
// it.  The numeric specification is in include/rtow.h next to the entry point (and DESIGN.md 5); tests/noise_mask_reference.py restates it in numpy and the GPU tests
// compare the two bit for bit.
//
// Launch shape.  The 64 x 4 pixel workgroup tile and grid-stride tile loop of the denoise levels and of estimate_moments_kernel; a wave is 64 pixels of one
// row.  A workgroup stages e(q) for its tile plus a halo of dilate + 1 into LDS once (a 72 x 12 plane at dilate 3; -1 for "unknown or outside the image"), computes
// "qualifies" from it for the region the dilation reads (70 x 10) into a second plane, and each lane ORs its (2 dilate + 1)^2 window from there.  Consecutive lanes read
// consecutive words of a plane: no bank conflict, no padding.  The planes and the workgroup's statistics take 6.7 KB of LDS: it does not cap the 8 waves per SIMD.
// Statistics are integers: counts by wave ballot and histogram bins by LDS atomics per workgroup, one global atomic per non-empty word when the workgroup is through
// with its tiles, the maximum as an atomic max on the bit pattern (g >= 0).  No float is summed, so two runs give identical bits.  The last workgroup to finish
// copies the record from the scratch to outStats.
#include "rtow_kernels.h"
#include "rtow_denoise_taps.hip.h"
#include "rtow_moments_variance.hip.h"

namespace rtow {

namespace {

using namespace taps;

// Tiles beyond this many workgroups are walked by the grid-stride loop, and a workgroup flushes its statistics once: every workgroup costs some 20 device-wide atomics
// on the three cache lines of the record, which the memory side serialises (measured: 0.1 ms per 1000 workgroups).  Timed on one box in one run at 256 / 512 / 1024 /
// 2048 (dilate 0, no budget): 1920 x 1080 0.156 / 0.117 / 0.134 / 0.233 ms, 3840 x 2160 0.538 / 0.315 / 0.266 / 0.356 ms (profiles/r14_noise_mask.json).
constexpr unsigned kMaxBlocks = 1024;
constexpr int kMaxDilate = 3;
constexpr int kQW = kGroupW + 2 * kMaxDilate, kQH = kGroupH + 2 * kMaxDilate;      // 70 x 10: the "qualifies" plane
constexpr int kEW = kQW + 2, kEH = kQH + 2;                                       // 72 x 12: the e plane
constexpr float kUnknown = -1.0f;
constexpr int kBins = 64;

static_assert(sizeof(RtowNoiseStats) == RTOW_NOISE_MASK_SCRATCH_BYTES && sizeof(RtowNoiseStats) == 72 * 4, "the scratch is one record of 72 words");

// the words of the record (RtowNoiseStats); in the scratch reserved[0] counts the workgroups of the publishing pass that are through
enum : unsigned { kKnown = 0, kUnknownCount = 1, kQualifying = 2, kMasked = 3, kThreshold = 4, kMaxError = 5, kDone = 6, kHistogram = 8, kWords = 72 };

struct NoiseArgs {
    int width, height;
    TileGrid grid;                      // the 64 x 4 pixel tiles
    int dilate, absolute, unknownQualifies;
    int thresholdFromRecord;            // the second pass of a budget: T is what the pick step left in the record
    float threshold;                    // errorThreshold
    float F2;                           // luminanceFloor * luminanceFloor
    const float* moments;
    uint8_t* outMask;
    float* outError;
    unsigned* outStats;
    unsigned* record;                   // the scratch
};

// e(q) of the specification, -1 when unknown
__device__ __forceinline__ float own_error(const NoiseArgs& A, size_t q)
{
    const P3 m = ld3(A.moments, q);
    float mean, v;
    if (!finite3(m) || !mean_variance(m, mean, v)) return kUnknown;          // without the first test the clamp of d would turn a NaN sum into a variance of zero
    const float e = A.absolute ? v : v / (mean * mean + A.F2);
    return __builtin_isfinite(e) ? e : kUnknown;
}

// g at the position whose e is sE[k], -1 when unknown.  A tap outside the image holds -1 like an unknown one.
__device__ __forceinline__ float filtered_error(const float* sE, int k)
{
    if (!(sE[k] >= 0.0f)) return kUnknown;
    float num = 0.0f, den = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const float eq = sE[k + j * kEW + i];
            const bool tap = eq >= 0.0f;                                   // selects, not branches: an unknown tap leaves both sums as they are
            const float w = (i == 0 ? 0.5f : 0.25f) * (j == 0 ? 0.5f : 0.25f);
            num = tap ? num + w * eq : num;
            den = tap ? den + w : den;
        }
    }
    const float g = num / den;
    return __builtin_isfinite(g) ? g : kUnknown;
}

// kStats: the pass counts known / unknown, fills the histogram and the maximum, and writes outError.  kMask: the pass has its threshold, writes the mask, counts
// qualifying / masked and publishes the record.  Without a budget one pass does both; with one the pick step runs between a kStats and a kMask pass.
template <bool kStats, bool kMask>
__global__ void __launch_bounds__(256, 8) noise_mask_kernel(NoiseArgs A)
{
    __shared__ float sE[kEW * kEH];
    __shared__ unsigned sQ[kQW * kQH];
    __shared__ unsigned sHist[kBins], sCount[4], sMax, sLast;
    const int lx = (int)(threadIdx.x & 63u), ly = (int)(threadIdx.x >> 6);
    if (threadIdx.x < kBins) sHist[threadIdx.x] = 0u;
    if (threadIdx.x < 4) sCount[threadIdx.x] = 0u;
    if (threadIdx.x == 0) sMax = 0u;
    const int D = kMask ? A.dilate : 0;          // a pass that only counts reads no neighbour beyond the 3 x 3 filter's
    float T = A.threshold;
    if (kMask && A.thresholdFromRecord) T = __uint_as_float(A.record[kThreshold]);          // written by the launch before this one
    // the parts of the planes this dilate reads: e over (66 + 2 D) x (6 + 2 D) from (2 - D, 2 - D), qualifies over (64 + 2 D) x (4 + 2 D) from (3 - D, 3 - D)
    // (whole rows of the planes are walked, so that the row and the column of a word come from divisions by constants)
    const int e0 = kMaxDilate - D, e1 = kEW - e0, eBegin = e0 * kEW, eEnd = (kEH - e0) * kEW;
    const int q0 = kMaxDilate - D, q1 = kQW - q0, qBegin = q0 * kQW, qEnd = (kQH - q0) * kQW;
    for (unsigned t = blockIdx.x; t < A.grid.tiles; t += gridDim.x) {          // the same tiles for every lane of the workgroup: the barriers below are uniform
        const int x0 = (int)(t % A.grid.tilesX) * kGroupW, y0 = (int)(t / A.grid.tilesX) * kGroupH;
        const int x = x0 + lx, y = y0 + ly;
        const bool inside = x < A.width && y < A.height;
        const size_t p = (size_t)y * (size_t)A.width + (size_t)x;
        __syncthreads();          // every lane is through with the planes of the previous tile (and the statistics are cleared) before they are staged again
#pragma unroll 1
        for (int k = eBegin + (int)threadIdx.x; k < eEnd; k += 256) {
            const int cx = k % kEW, cy = k / kEW;                         // in the 72 x 12 plane, whose (0, 0) is the pixel (x0 - 4, y0 - 4)
            if (cx < e0 || cx >= e1) continue;
            const int qx = x0 - (kMaxDilate + 1) + cx, qy = y0 - (kMaxDilate + 1) + cy;
            float e = kUnknown;
            if (qx >= 0 && qx < A.width && qy >= 0 && qy < A.height) e = own_error(A, (size_t)qy * (size_t)A.width + (size_t)qx);
            sE[k] = e;
        }
        __syncthreads();
        // the lane's own pixel: g stays in a register for the statistics and outError
        const float g = filtered_error(sE, (ly + kMaxDilate + 1) * kEW + lx + kMaxDilate + 1);
        const bool known = inside && g >= 0.0f;
        if (kStats) {
            if (inside && A.outError) A.outError[p] = g;
            const unsigned long long kb = __ballot(known), ub = __ballot(inside && !known);
            if (lx == 0) {
                if (kb) atomicAdd(&sCount[kKnown], (unsigned)__popcll(kb));
                if (ub) atomicAdd(&sCount[kUnknownCount], (unsigned)__popcll(ub));
            }
            if (known) {
                const unsigned bits = __float_as_uint(g);
                const int b = (int)(bits >> 23) - 96;
                atomicAdd(&sHist[b < 0 ? 0 : b > kBins - 1 ? kBins - 1 : b], 1u);
                atomicMax(&sMax, bits);                                   // non-negative floats order like their bit patterns
            }
        }
        if (kMask) {
            const bool qualifies = inside && (known ? g >= T : A.unknownQualifies != 0);
            sQ[(ly + kMaxDilate) * kQW + lx + kMaxDilate] = qualifies ? 1u : 0u;
            // the halo of the qualifies plane: pixels of other tiles (counted there) or outside the image (never qualifying)
#pragma unroll 1
            for (int k = qBegin + (int)threadIdx.x; k < qEnd; k += 256) {
                const int cx = k % kQW, cy = k / kQW;                     // in the 70 x 10 plane, whose (0, 0) is the pixel (x0 - 3, y0 - 3)
                if (cx < q0 || cx >= q1) continue;
                if (cx >= kMaxDilate && cx < kMaxDilate + kGroupW && cy >= kMaxDilate && cy < kMaxDilate + kGroupH) continue;
                const int qx = x0 - kMaxDilate + cx, qy = y0 - kMaxDilate + cy;
                unsigned q = 0u;
                if (qx >= 0 && qx < A.width && qy >= 0 && qy < A.height) {
                    const float gq = filtered_error(sE, (cy + 1) * kEW + cx + 1);
                    q = (gq >= 0.0f ? gq >= T : A.unknownQualifies != 0) ? 1u : 0u;
                }
                sQ[k] = q;
            }
            __syncthreads();
            unsigned m = 0u;
            const int centre = (ly + kMaxDilate) * kQW + lx + kMaxDilate;
#pragma unroll 1
            for (int j = -D; j <= D; ++j)
#pragma unroll 1
                for (int i = -D; i <= D; ++i) m |= sQ[centre + j * kQW + i];
            const bool masked = inside && m != 0u;
            if (inside) A.outMask[p] = masked ? 1 : 0;
            const unsigned long long qb = __ballot(qualifies), mb = __ballot(masked);
            if (lx == 0) {
                if (qb) atomicAdd(&sCount[kQualifying], (unsigned)__popcll(qb));
                if (mb) atomicAdd(&sCount[kMasked], (unsigned)__popcll(mb));
            }
        }
    }
    __syncthreads();
    // the workgroup's statistics into the record: one global atomic per non-empty word
    if (kStats && threadIdx.x < kBins && sHist[threadIdx.x]) atomicAdd(A.record + kHistogram + threadIdx.x, sHist[threadIdx.x]);
    if (threadIdx.x >= 64 && threadIdx.x < 68 && sCount[threadIdx.x - 64]) atomicAdd(A.record + (threadIdx.x - 64), sCount[threadIdx.x - 64]);
    if (kStats && threadIdx.x == 68 && sMax) atomicMax(A.record + kMaxError, sMax);
    if (!kMask) return;
    // the last workgroup through publishes the record
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) sLast = __hip_atomic_fetch_add(A.record + kDone, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u ? 1u : 0u;
    __syncthreads();
    if (!sLast || !A.outStats || threadIdx.x >= kWords) return;
    __threadfence();
    unsigned w = __hip_atomic_load(A.record + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == kThreshold) w = __float_as_uint(T);
    if (threadIdx.x == kDone || threadIdx.x == kDone + 1) w = 0u;
    A.outStats[threadIdx.x] = w;
}

// T of the specification from the histogram the first pass left in the record: one wave, lane 0 walks the 64 bins from the top
__global__ void __launch_bounds__(64) noise_pick_kernel(unsigned* record, float errorThreshold, unsigned maxQualifying, int unknownQualifies)
{
    if (threadIdx.x != 0) return;
    const unsigned U = unknownQualifies ? record[kUnknownCount] : 0u;
    const unsigned R = maxQualifying > U ? maxQualifying - U : 0u;
    int best = -1;
    unsigned tail = 0u;                                                    // at most width * height <= INT32_MAX
    for (int b = kBins - 1; b >= 0; --b) {
        tail += record[kHistogram + b];
        if (tail > R) break;                                               // the tails only grow towards bin 0
        best = b;
    }
    float T = __builtin_inff();
    if (best >= 0) {
        const float L = best == 0 ? 0.0f : __uint_as_float((unsigned)(best + 96) << 23);      // 2^(b-31)
        T = errorThreshold > L ? errorThreshold : L;
    }
    record[kThreshold] = __float_as_uint(T);
}

}  // namespace

hipError_t launchNoiseMask(const RtowNoiseMaskParams& p, const float* moments, uint8_t* outMask, float* outError, RtowNoiseStats* outStats, void* scratch,
                           hipStream_t stream)
{
    NoiseArgs A{};
    A.width = p.width;
    A.height = p.height;
    A.grid = tileGrid(p.width, p.height);
    A.dilate = p.dilate;
    A.absolute = (p.flags & RTOW_NOISE_MASK_ABSOLUTE) != 0;
    A.unknownQualifies = (p.flags & RTOW_NOISE_MASK_UNKNOWN_QUALIFIES) != 0;
    A.threshold = p.errorThreshold;
    A.F2 = p.luminanceFloor * p.luminanceFloor;
    A.moments = moments;
    A.outMask = outMask;
    A.outError = outError;
    A.outStats = reinterpret_cast<unsigned*>(outStats);
    A.record = static_cast<unsigned*>(scratch);
    const dim3 blocks(A.grid.tiles < kMaxBlocks ? A.grid.tiles : kMaxBlocks);
    hipError_t e = hipMemsetAsync(scratch, 0, RTOW_NOISE_MASK_SCRATCH_BYTES, stream);
    if (e != hipSuccess) return e;
    if (p.maxQualifying == 0) {
        hipLaunchKernelGGL((noise_mask_kernel<true, true>), blocks, dim3(256), 0, stream, A);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((noise_mask_kernel<true, false>), blocks, dim3(256), 0, stream, A);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(noise_pick_kernel, dim3(1), dim3(64), 0, stream, A.record, p.errorThreshold, (unsigned)p.maxQualifying, A.unknownQualifies);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    A.thresholdFromRecord = 1;
    hipLaunchKernelGGL((noise_mask_kernel<false, true>), blocks, dim3(256), 0, stream, A);
    return hipGetLastError();
}

}  // namespace rtow
