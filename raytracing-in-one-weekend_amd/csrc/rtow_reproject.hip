// rtow_reproject.hip - rtowReprojectAccumDevice's kernel: the previous view's accumulated sums, gathered to the pixels of a new view (backward reprojection of a
// static scene by the first hit of each pixel's camera ray, nearest neighbour).  The numeric specification is in include/rtow.h next to RtowReprojectParams
// (and DESIGN.md 5); tests/reproject_reference.py restates it in numpy and the GPU tests compare the two bit for bit.
//
// Launch shape: one lane per output pixel, a wave is an 8 x 8 pixel tile (as rtowTraceViewDevice maps them), so the 64 gathers of a wave from the
// previous frame land in a few rows of it; a workgroup is four tiles, and tiles beyond the grid limit are walked by a grid-stride loop.  No LDS, no barrier.
#include "rtow_kernels.h"

#include "rtow_vecmath.hip.h"

namespace rtow {

namespace {

constexpr int kReprojectBlock = 256;                      // four 8 x 8 tiles
constexpr unsigned kReprojectMaxBlocks = 4096;            // two rounds of the 2048 workgroups an MI355X holds at 8 waves per SIMD; tile groups beyond this (frames from
                                                          // about 1024 x 1024) are walked by the grid-stride loop

struct ReprojectArgs {
    int width, height;
    unsigned tilesX, tiles;             // 8 x 8 pixel tiles per row / in all
    RtowFloat3 origin, forward, right, up;      // of previousView
    ReprojectConstants k;
    float depthTolerance, maxHistory;   // (float)maxHistory
    int matchEntity;
    const RtowRay* rays;
    const float* distance;
    const int32_t* entity;
    const float* prevDistance;
    const int32_t* prevEntity;
    const float *prevColor, *prevNormal, *prevAlbedo, *prevScw;
    float *outColor, *outNormal, *outAlbedo, *outScw;
    int32_t* outSource;
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, RtowFloat3 b) { return (ax * b.x + ay * b.y) + az * b.z; }

// the previous pixel that pixel `i` carries, or -1 (steps 1 - 3 of the specification)
__device__ __forceinline__ int source_pixel(const ReprojectArgs& A, size_t i)
{
    const Ray8 ray = reinterpret_cast<const Ray8*>(A.rays)[i];
    const float t = A.distance[i];
    const int e = A.entity[i];
    float wx = ray.dx, wy = ray.dy, wz = ray.dz, r = 0.0f;
    if (e >= 0) {
        const float px = ray.ox + t * ray.dx, py = ray.oy + t * ray.dy, pz = ray.oz + t * ray.dz;
        wx = px - A.origin.x; wy = py - A.origin.y; wz = pz - A.origin.z;
        r = exact_sqrt((wx * wx + wy * wy) + wz * wz);
    }
    const float s = dot3(wx, wy, wz, A.forward) / A.k.LF;
    if (!(s > 0.0f)) return -1;
    const float u = (dot3(wx, wy, wz, A.right) / s - A.k.LR) / A.k.HR;
    const float v = (dot3(wx, wy, wz, A.up) / s - A.k.LU) / A.k.VU;
    const float sizeX = (float)A.width, sizeY = (float)A.height;
    const float fx = u * sizeX, fy = v * sizeY;
    if (!(fx >= 0.0f && fx < sizeX && fy >= 0.0f && fy < sizeY)) return -1;          // NaN fails
    const int qx = (int)fx, qy = (int)fy;
    if (qx >= A.width || qy >= A.height) return -1;        // only where (float)width > width (sizes beyond 2^24): never outside the frame
    const int q = qy * A.width + qx;
    const int pe = A.prevEntity[q];
    if (e < 0) return pe < 0 ? q : -1;
    if (pe < 0 || (A.matchEntity && pe != e)) return -1;
    const float pt = A.prevDistance[q];
    return __builtin_fabsf(pt - r) <= A.depthTolerance * r ? q : -1;
}

__global__ void __launch_bounds__(kReprojectBlock) reproject_kernel(ReprojectArgs A)
{
    const unsigned stride = gridDim.x * (kReprojectBlock / 64);       // at most 4 x kReprojectMaxBlocks: no wrap below
    for (unsigned tile = blockIdx.x * (kReprojectBlock / 64) + (threadIdx.x >> 6); tile < A.tiles; tile += stride) {
        // wave = 8 x 8 pixel tile, lane = (lane & 7, lane >> 3) inside it
        const int cx = (int)(tile % A.tilesX) * 8 + (int)(threadIdx.x & 7u);
        const int cy = (int)(tile / A.tilesX) * 8 + (int)((threadIdx.x >> 3) & 7u);
        if (cx >= A.width || cy >= A.height) continue;
        const size_t i = (size_t)cy * (size_t)A.width + (size_t)cx;
        int q = source_pixel(A, i);
        P4 c{0.0f, 0.0f, 0.0f, 0.0f};
        P3 n{0.0f, 0.0f, 0.0f}, a{0.0f, 0.0f, 0.0f};
        float w = 0.0f;
        if (q >= 0) {
            c = reinterpret_cast<const P4*>(A.prevColor)[q];
            const bool finite = __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z) && __builtin_isfinite(c.w);
            if (finite && c.w >= 1.0f) {
                n = reinterpret_cast<const P3*>(A.prevNormal)[q];
                a = reinterpret_cast<const P3*>(A.prevAlbedo)[q];
                w = A.prevScw[q];
                if (c.w > A.maxHistory) {                  // the sums of color.w samples scaled to maxHistory of them
                    const float k = A.maxHistory / c.w;
                    c = P4{c.x * k, c.y * k, c.z * k, A.maxHistory};
                    n = P3{n.x * k, n.y * k, n.z * k};
                    a = P3{a.x * k, a.y * k, a.z * k};
                    w = w * k;
                }
            } else {
                q = -1;
                c = P4{0.0f, 0.0f, 0.0f, 0.0f};
            }
        }
        reinterpret_cast<P4*>(A.outColor)[i] = c;
        reinterpret_cast<P3*>(A.outNormal)[i] = n;
        reinterpret_cast<P3*>(A.outAlbedo)[i] = a;
        A.outScw[i] = w;
        if (A.outSource) A.outSource[i] = q;
    }
}

}  // namespace

hipError_t launchReproject(const RtowReprojectParams& p, const ReprojectConstants& k, const RtowRay* rays, const RtowHitBuffers& hits, const RtowHitBuffers& previousHits,
                           const RtowAccumBuffers& previous, const RtowAccumBuffers& out, int32_t* outSource, hipStream_t stream)
{
    ReprojectArgs A{};
    A.width = p.width;
    A.height = p.height;
    A.tilesX = ((unsigned)p.width + 7u) / 8u;
    A.tiles = (unsigned)((uint64_t)A.tilesX * (((uint64_t)p.height + 7u) / 8u));      // (w / 8 + 1) (h / 8 + 1) < 2^29 for w h < 2^31
    A.origin = p.previousView.origin;
    A.forward = p.previousView.forward;
    A.right = p.previousView.right;
    A.up = p.previousView.up;
    A.k = k;
    A.depthTolerance = p.depthTolerance;
    A.maxHistory = (float)p.maxHistory;
    A.matchEntity = (p.flags & RTOW_REPROJECT_MATCH_ENTITY) != 0;
    A.rays = rays;
    A.distance = hits.distance;
    A.entity = hits.entityIndex;
    A.prevDistance = previousHits.distance;
    A.prevEntity = previousHits.entityIndex;
    A.prevColor = previous.color; A.prevNormal = previous.normal; A.prevAlbedo = previous.albedo; A.prevScw = previous.sampleCountWeight;
    A.outColor = out.color; A.outNormal = out.normal; A.outAlbedo = out.albedo; A.outScw = out.sampleCountWeight;
    A.outSource = outSource;
    const unsigned groups = (A.tiles + kReprojectBlock / 64 - 1) / (kReprojectBlock / 64);
    const unsigned blocks = groups < kReprojectMaxBlocks ? groups : kReprojectMaxBlocks;
    hipLaunchKernelGGL(reproject_kernel, dim3(blocks), dim3(kReprojectBlock), 0, stream, A);
    return hipGetLastError();
}

}  // namespace rtow
