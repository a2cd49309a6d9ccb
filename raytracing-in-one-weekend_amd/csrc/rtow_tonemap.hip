// rtow_tonemap.hip - rtowMeterExposureDevice and rtowFinalizeToneMappedDevice: the exposure a frame asks for, measured on the device, and the finalize pass with that
// exposure and a tone curve in front of the colour's byte conversion (the line the reference left commented out, JOBS/FinalizeTexturesJob.cs:28, with the curves of
// UTIL/Tools.cs:194-234).  The numeric specification of both is in include/rtow.h next to the entry points (and DESIGN.md 5); tests/tonemap_reference.py restates it in
// numpy and the GPU tests compare the two bit for bit.
//
// Launch shape.  The meter is two plain launches in stream order.  exposure_histogram_kernel: at most 256 workgroups of 256 lanes in a grid-stride loop
// over groups of four pixels - twelve floats, three 16-byte loads, the widest the 4-byte alignment of a float3 stream allows - with the next group's loads issued before
// this group is counted.  Each wave counts into a 256-bin row of its own in LDS, so the lanes of a wave contend only with each other; the workgroup stores the sums of
// its four rows to its slab of the scratch.  No global atomic (rtow_noise_mask.hip measured what they cost: 0.1 ms per 1000 workgroups) and no clear: every word a later
// step reads has been stored by the step before it.  exposure_resolve_kernel: one workgroup, a lane per bin sums the slabs, a scan gives every bin its ranks, a
// reduction the trimmed sum, and lane 0 resolves the record.  Counts are integers, so the result does not depend on which workgroup counted which pixel.
// tonemap_finalize_kernel<CURVE>: the software-pipelined streaming shape of finalize_kernel (rtow_kernels.hip) over the same step table; the curve is a template
// parameter, so CLAMP carries no ACES code, and with both guide pairs present the nine conversions of a pixel run as one batch, as there.
#include "rtow_kernels.h"
#include "rtow_vecmath.hip.h"
#define RTOW_FINALIZE_NO_TABLE_BUILDER 1      // the table is built by rtow_kernels.hip; this unit only reads it
#include "rtow_finalize.hip.h"

namespace rtow {

namespace {

constexpr unsigned kMeterBlocks = 256;            // at most: RTOW_EXPOSURE_SCRATCH_BYTES holds a slab for each
constexpr int kBins = 256;
static_assert(RTOW_EXPOSURE_SCRATCH_BYTES == (size_t)kMeterBlocks * kBins * sizeof(unsigned), "one slab of 256 sums per workgroup");
static_assert(sizeof(RtowExposureState) == 1056 && sizeof(RtowExposureParams) == 40 && sizeof(RtowToneMapParams) == 24, "include/rtow.h states these sizes");

struct __attribute__((packed, aligned(4))) F3 { float x, y, z; };
struct __attribute__((packed, aligned(4))) F4 { float x, y, z, w; };       // 16 bytes at a 4-byte boundary: one global_load_dwordx4
__device__ __forceinline__ V3 load3(const float* p, size_t index) { const F3 v = reinterpret_cast<const F3*>(p)[index]; return v3(v.x, v.y, v.z); }

// the bin of one pixel, -1 when it is not metered
__device__ __forceinline__ int exposure_bin(float r, float g, float b)
{
    const float l = (0.2126f * r + 0.7152f * g) + 0.0722f * b;
    if (!(l >= 0x1p-16f && l < __builtin_inff())) return -1;              // NaN fails the first comparison
    const int bin = (int)(__float_as_uint(l) >> 20) - 0x378;
    return bin < kBins - 1 ? bin : kBins - 1;
}

__device__ __forceinline__ void count_pixel(unsigned* row, float r, float g, float b)
{
    const int bin = exposure_bin(r, g, b);
    if (bin >= 0) atomicAdd(row + bin, 1u);
}

__global__ void __launch_bounds__(256) exposure_histogram_kernel(int n, const float* __restrict__ inColor, unsigned* __restrict__ slabs)
{
    __shared__ unsigned sRows[4][kBins];
    for (int w = 0; w < 4; ++w) sRows[w][threadIdx.x] = 0u;
    __syncthreads();
    unsigned* row = sRows[threadIdx.x >> 6];
    const int quads = n >> 2, stride = (int)(gridDim.x * blockDim.x);
    const F4* in4 = reinterpret_cast<const F4*>(inColor);
    int q = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    F4 a{}, b{}, c{};
    if (q < quads) { a = in4[3 * (size_t)q]; b = in4[3 * (size_t)q + 1]; c = in4[3 * (size_t)q + 2]; }
    while (q < quads) {
        const int q2 = q + stride;
        F4 a2{}, b2{}, c2{};
        if (q2 < quads) { a2 = in4[3 * (size_t)q2]; b2 = in4[3 * (size_t)q2 + 1]; c2 = in4[3 * (size_t)q2 + 2]; }
        count_pixel(row, a.x, a.y, a.z);
        count_pixel(row, a.w, b.x, b.y);
        count_pixel(row, b.z, b.w, c.x);
        count_pixel(row, c.y, c.z, c.w);
        a = a2; b = b2; c = c2;
        q = q2;
    }
    // the one to three pixels behind the last group of four
    const int tail = 4 * quads + (int)threadIdx.x;
    if (blockIdx.x == 0 && tail < n) { const V3 p = load3(inColor, (size_t)tail); count_pixel(row, p.x, p.y, p.z); }
    __syncthreads();
    slabs[(size_t)blockIdx.x * kBins + threadIdx.x] = (sRows[0][threadIdx.x] + sRows[1][threadIdx.x]) + (sRows[2][threadIdx.x] + sRows[3][threadIdx.x]);
}

struct ResolveArgs {
    unsigned pixels;                    // width * height
    unsigned slabs;                     // workgroups of the histogram launch
    unsigned lowPermille, highPermille;
    float compensation, minStops, maxStops, rate;
};

__device__ __forceinline__ float sel_min(float a, float b) { return a < b ? a : b; }
__device__ __forceinline__ float sel_max(float a, float b) { return a > b ? a : b; }

__global__ void __launch_bounds__(256) exposure_resolve_kernel(ResolveArgs A, const unsigned* __restrict__ slabs, RtowExposureState* state)
{
    __shared__ unsigned sCum[kBins];
    __shared__ unsigned long long sSum[kBins];
    const unsigned b = threadIdx.x;
    unsigned h = 0u;
#pragma unroll 8
    for (unsigned s = 0; s < A.slabs; ++s) h += slabs[(size_t)s * kBins + b];
    // inclusive scan of the 256 counts (their sum is at most width * height <= INT32_MAX)
    sCum[b] = h;
    __syncthreads();
    for (unsigned d = 1; d < (unsigned)kBins; d <<= 1) {
        const unsigned add = b >= d ? sCum[b - d] : 0u;
        __syncthreads();
        sCum[b] += add;
        __syncthreads();
    }
    const unsigned long long metered = sCum[kBins - 1], end = sCum[b], begin = end - h;
    const unsigned long long lo = metered * A.lowPermille / 1000ull, hi = metered * A.highPermille / 1000ull, N = hi - lo;
    // the ranks of bin b inside [lo, hi)
    const unsigned long long from = begin > lo ? begin : lo, to = end < hi ? end : hi;
    sSum[b] = to > from ? (unsigned long long)b * (to - from) : 0ull;     // at most 255 * 2^31
    __syncthreads();
    for (unsigned s = kBins / 2; s > 0; s >>= 1) {
        if (b < s) sSum[b] += sSum[b + s];
        __syncthreads();
    }
    state->histogram[b] = h;
    if (b != 0) return;
    const unsigned valid = state->valid;
    const float stops = state->stops;
    float meanLog2 = 0.0f, target = valid ? stops : 0.0f;
    if (N > 0) {
        const unsigned long long Q = (sSum[0] * 256ull + N / 2ull) / N;       // at most 255 * 256
        meanLog2 = ((float)Q * 0x1p-11f - 16.0f) + 0x1p-4f;
        target = A.compensation - meanLog2;
    }
    const float targetStops = sel_min(sel_max(target, A.minStops), A.maxStops);
    const float s = (valid != 0u && A.rate < 1.0f) ? stops + (targetStops - stops) * A.rate : targetStops;
    const float newStops = sel_min(sel_max(s, A.minStops), A.maxStops);
    state->exposure = det_exp2(newStops);
    state->stops = newStops;
    state->targetStops = targetStops;
    state->meanLog2 = meanLog2;
    state->valid = N > 0 ? 1u : valid;
    state->metered = (unsigned)metered;
    state->ignored = A.pixels - (unsigned)metered;
    state->reserved = 0u;
}

// x of the specification: c * s, NaN and negatives to 0, at most 65536
__device__ __forceinline__ float tone_operand(float c, float s)
{
    const float x = c * s;
    const float p = x > 0.0f ? x : 0.0f;
    return p < 65536.0f ? p : 65536.0f;
}

__device__ __forceinline__ float aces_fit(float v)
{
    const float a = v * (v + 0.0245786f) - 0.000090537f;
    const float b = v * (0.983729f * v + 0.4329510f) + 0.238081f;
    return a / b;
}

template <int CURVE>
__device__ __forceinline__ V3 tone_curve(V3 c, float s)
{
    const V3 x = v3(tone_operand(c.x, s), tone_operand(c.y, s), tone_operand(c.z, s));
    if (CURVE == RTOW_TONE_ACES_FILM) {
        return v3((x.x * (2.51f * x.x + 0.03f)) / (x.x * (2.43f * x.x + 0.59f) + 0.14f),
                  (x.y * (2.51f * x.y + 0.03f)) / (x.y * (2.43f * x.y + 0.59f) + 0.14f),
                  (x.z * (2.51f * x.z + 0.03f)) / (x.z * (2.43f * x.z + 0.59f) + 0.14f));
    }
    if (CURVE == RTOW_TONE_ACES_FITTED) {
        // ACESInputMat, RRTAndODTFit, ACESOutputMat (UTIL/Tools.cs:198-215)
        const float wr = aces_fit((0.59719f * x.x + 0.35458f * x.y) + 0.04823f * x.z);
        const float wg = aces_fit((0.07600f * x.x + 0.90834f * x.y) + 0.01566f * x.z);
        const float wb = aces_fit((0.02840f * x.x + 0.13383f * x.y) + 0.83777f * x.z);
        return v3((1.60475f * wr + -0.53108f * wg) + -0.07367f * wb,
                  (-0.10208f * wr + 1.10813f * wg) + -0.00605f * wb,
                  (-0.00327f * wr + -0.07276f * wg) + 1.07602f * wb);
    }
    return x;
}

__device__ __forceinline__ void store_bytes3(uchar4* out, int i, V3 v, const float* T, const ByteZones& Z)
{
    const float in[3] = {v.x, v.y, v.z};
    unsigned b[3];
    to_bytes_table<3>(in, b, T, Z);
    out[i] = make_uchar4((unsigned char)b[0], (unsigned char)b[1], (unsigned char)b[2], 255);
}

template <int CURVE>
__global__ void __launch_bounds__(256, 8) tonemap_finalize_kernel(int n, float exposure, const RtowExposureState* __restrict__ state, const float* __restrict__ inColor,
                                                                  const float* __restrict__ inNormal, const float* __restrict__ inAlbedo, uchar4* __restrict__ outColor,
                                                                  uchar4* __restrict__ outNormal, uchar4* __restrict__ outAlbedo, const float* __restrict__ thresholds)
{
    __shared__ float T[kByteThresholdFloats];
    for (int i = (int)threadIdx.x; i < kByteThresholdFloats; i += (int)blockDim.x) T[i] = thresholds[i];
    __syncthreads();
    const ByteZones Z = load_byte_zones(T);
    float s = exposure;
    if (state) s = exposure * (state->valid ? state->exposure : 1.0f);      // what the meter left, read here and not by the host
    // software pipelined like finalize_kernel: the next pixel's loads are issued before this pixel's conversions
    const int stride = (int)(gridDim.x * blockDim.x);
    int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    V3 c = v3(0, 0, 0), nm = v3(0, 0, 0), al = v3(0, 0, 0);
    if (i < n) {
        c = load3(inColor, (size_t)i);
        if (inNormal) nm = load3(inNormal, (size_t)i);
        if (inAlbedo) al = load3(inAlbedo, (size_t)i);
    }
    while (i < n) {
        const int j = n - i > stride ? i + stride : n;          // no step past INT32_MAX
        V3 c2 = v3(0, 0, 0), nm2 = v3(0, 0, 0), al2 = v3(0, 0, 0);
        if (j < n) {
            c2 = load3(inColor, (size_t)j);
            if (inNormal) nm2 = load3(inNormal, (size_t)j);
            if (inAlbedo) al2 = load3(inAlbedo, (size_t)j);
        }
        const V3 y = tone_curve<CURVE>(c, s);
        if (inNormal && inAlbedo) {
            // nine independent conversions (rtow_finalize.hip.h): their LDS reads are in flight together
            const float v[9] = {y.x, y.y, y.z, nm.x * 0.5f + 0.5f, nm.y * 0.5f + 0.5f, nm.z * 0.5f + 0.5f, al.x, al.y, al.z};
            unsigned b[9];
            to_bytes_table<9>(v, b, T, Z);
            outColor[i] = make_uchar4((unsigned char)b[0], (unsigned char)b[1], (unsigned char)b[2], 255);
            outNormal[i] = make_uchar4((unsigned char)b[3], (unsigned char)b[4], (unsigned char)b[5], 255);
            outAlbedo[i] = make_uchar4((unsigned char)b[6], (unsigned char)b[7], (unsigned char)b[8], 255);
        } else {
            // a guide pair is missing: the colour, and the guide that is there, three conversions at a time
            store_bytes3(outColor, i, y, T, Z);
            if (inNormal) store_bytes3(outNormal, i, v3(nm.x * 0.5f + 0.5f, nm.y * 0.5f + 0.5f, nm.z * 0.5f + 0.5f), T, Z);
            if (inAlbedo) store_bytes3(outAlbedo, i, al, T, Z);
        }
        c = c2; nm = nm2; al = al2;
        i = j;
    }
}

template <int CURVE>
hipError_t launchCurve(int n, float exposure, const RtowExposureState* state, const float* inColor, const float* inNormal, const float* inAlbedo, uint8_t* outColor,
                       uint8_t* outNormal, uint8_t* outAlbedo, const float* thresholds, hipStream_t stream)
{
    // the grid of the streaming post passes (rtow_kernels.hip): one workgroup per 256 pixels, dispatched in order
    constexpr int kMaxBlocks = 1048576;
    const int blocks = n < 256 * kMaxBlocks ? (n + 255) / 256 : kMaxBlocks;
    hipLaunchKernelGGL((tonemap_finalize_kernel<CURVE>), dim3(blocks > 0 ? blocks : 1), dim3(256), 0, stream, n, exposure, state, inColor, inNormal, inAlbedo,
                       reinterpret_cast<uchar4*>(outColor), reinterpret_cast<uchar4*>(outNormal), reinterpret_cast<uchar4*>(outAlbedo), thresholds);
    return hipGetLastError();
}

}  // namespace

hipError_t launchMeterExposure(const RtowExposureParams& p, const float* inColor, void* scratch, RtowExposureState* state, hipStream_t stream)
{
    const int n = p.width * p.height;
    const unsigned quads = (unsigned)n / 4u;
    const unsigned want = (quads + 255u) / 256u;
    const unsigned blocks = want < 1u ? 1u : want > kMeterBlocks ? kMeterBlocks : want;
    hipLaunchKernelGGL(exposure_histogram_kernel, dim3(blocks), dim3(256), 0, stream, n, inColor, static_cast<unsigned*>(scratch));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    ResolveArgs A{};
    A.pixels = (unsigned)n;
    A.slabs = blocks;
    A.lowPermille = (unsigned)p.lowPermille;
    A.highPermille = (unsigned)p.highPermille;
    A.compensation = p.compensation;
    A.minStops = p.minStops;
    A.maxStops = p.maxStops;
    A.rate = p.rate;
    hipLaunchKernelGGL(exposure_resolve_kernel, dim3(1), dim3(256), 0, stream, A, static_cast<const unsigned*>(scratch), state);
    return hipGetLastError();
}

hipError_t launchFinalizeToneMapped(const RtowToneMapParams& p, const RtowExposureState* state, const float* inColor, const float* inNormal, const float* inAlbedo,
                                    uint8_t* outColor, uint8_t* outNormal, uint8_t* outAlbedo, const float* thresholds, hipStream_t stream)
{
    switch (p.curve) {
    case RTOW_TONE_CLAMP: return launchCurve<RTOW_TONE_CLAMP>(p.pixelCount, p.exposure, state, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo, thresholds, stream);
    case RTOW_TONE_ACES_FITTED: return launchCurve<RTOW_TONE_ACES_FITTED>(p.pixelCount, p.exposure, state, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo, thresholds, stream);
    case RTOW_TONE_ACES_FILM: return launchCurve<RTOW_TONE_ACES_FILM>(p.pixelCount, p.exposure, state, inColor, inNormal, inAlbedo, outColor, outNormal, outAlbedo, thresholds, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace rtow
