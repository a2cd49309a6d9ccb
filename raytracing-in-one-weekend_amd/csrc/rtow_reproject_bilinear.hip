// rtow_reproject_bilinear.hip - rtowReprojectAccumBilinearDevice's kernel: the previous view's accumulated sums, gathered to the pixels of a new view through the
// four previous pixels around the reprojected point (SVGF's temporal reprojection, Schied et al., HPG 2017, section 4.1: every tap validated on its own, the
// bilinear weights renormalised over the valid ones), and with moments given the luminance moments through the same taps in the same pass.  The numeric
// specification is in include/rtow.h next to the entry point (and DESIGN.md 5); tests/reproject_bilinear_reference.py restates it in numpy and the GPU tests compare
// the two bit for bit.  Steps 1 to 3 are rtowReprojectAccumDevice's (rtow_reproject_steps.hip.h).
//
// Launch shape: the sibling's - one lane per output pixel, a wave is an 8 x 8 pixel tile, so the 4 x 64 gathers of a wave from the previous frame
// land in a few rows of it; a workgroup is four tiles, and tiles beyond the grid limit are walked by a grid-stride loop.  No LDS, no barrier.  The taps are
// processed one after another (a rolled loop: one tap's records live at a time); the kernel is a template on whether moments are carried, so that a call without
// them pays no registers for them.  A pixel with exactly one valid tap is written from that tap's records, read again (they are in cache), by step 4 of the sibling:
// the sums of a single tap do not reproduce its bits.
#include "rtow_reproject_steps.hip.h"

namespace rtow {

namespace {

struct ReprojectMomentsArgs {
    const float* previous;      // float3 per previous pixel
    float* out;                 // float3 per pixel
    float maxBatches;           // (float)maxBatches
};

__device__ __forceinline__ bool finite4(const P4& c) { return __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z) && __builtin_isfinite(c.w); }
__device__ __forceinline__ bool finite3(const P3& c) { return __builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z); }

template <bool kMoments>
__global__ void __launch_bounds__(kReprojectBlock) reproject_bilinear_kernel(ReprojectArgs A, ReprojectMomentsArgs M)
{
    const unsigned stride = gridDim.x * (kReprojectBlock / 64);       // at most 4 x kReprojectMaxBlocks: no wrap below
    for (unsigned tile = blockIdx.x * (kReprojectBlock / 64) + (threadIdx.x >> 6); tile < A.tiles; tile += stride) {
        // wave = 8 x 8 pixel tile, lane = (lane & 7, lane >> 3) inside it
        const int cx = (int)(tile % A.tilesX) * 8 + (int)(threadIdx.x & 7u);
        const int cy = (int)(tile / A.tilesX) * 8 + (int)((threadIdx.x >> 3) & 7u);
        if (cx >= A.width || cy >= A.height) continue;
        const size_t i = (size_t)cy * (size_t)A.width + (size_t)cx;

        // the ten sums (colour xyz, normal, albedo, sampleCountWeight), the weight B and the history n of the valid taps; the same of the moments
        float sc0 = 0.0f, sc1 = 0.0f, sc2 = 0.0f, sn0 = 0.0f, sn1 = 0.0f, sn2 = 0.0f, sa0 = 0.0f, sa1 = 0.0f, sa2 = 0.0f, sw = 0.0f;
        float B = 0.0f, n = 0.0f, best = 0.0f;
        int valid = 0, source = -1;
        float m1 = 0.0f, m2 = 0.0f, Bm = 0.0f, nm = 0.0f;
        int taking = 0, only = -1;           // taps whose moments take part; the last of them

        float fx, fy, r;
        int e;
        if (project_point(A, i, fx, fy, e, r)) {
            const float gx = fx - 0.5f, gy = fy - 0.5f;
            const float flx = __builtin_floorf(gx), fly = __builtin_floorf(gy);
            const int x0 = (int)flx, y0 = (int)fly;         // -1 .. W - 1, -1 .. H - 1
            const float ax = gx - (float)x0, ay = gy - (float)y0;
#pragma unroll 1
            for (int k = 0; k < 4; ++k) {
                const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                const float bx = (k & 1) ? ax : 1.0f - ax, by = (k >> 1) ? ay : 1.0f - ay;
                const float b = bx * by;
                const bool inside = qx >= 0 && qx < A.width && qy >= 0 && qy < A.height && b > 0.0f;
                const int q = inside ? qy * A.width + qx : 0;                 // pixel 0 stands in as the address of a tap that is not read for its value
                if (!(inside && tap_matches_unbranched(A, q, e, r))) continue;
                const P4 c = reinterpret_cast<const P4*>(A.prevColor)[q];
                if (!(finite4(c) && c.w >= 1.0f)) continue;
                const P3 pn = reinterpret_cast<const P3*>(A.prevNormal)[q];
                const P3 pa = reinterpret_cast<const P3*>(A.prevAlbedo)[q];
                const float pw = A.prevScw[q];
                const float u = b / c.w;
                B = B + b;
                sc0 = sc0 + u * c.x; sc1 = sc1 + u * c.y; sc2 = sc2 + u * c.z;
                sn0 = sn0 + u * pn.x; sn1 = sn1 + u * pn.y; sn2 = sn2 + u * pn.z;
                sa0 = sa0 + u * pa.x; sa1 = sa1 + u * pa.y; sa2 = sa2 + u * pa.z;
                sw = sw + u * pw;
                const float h = c.w < A.maxHistory ? c.w : A.maxHistory;
                n = (valid == 0 || h < n) ? h : n;
                ++valid;
                if (b > best) { best = b; source = q; }    // the first of equal weights stays
                if constexpr (kMoments) {
                    const P3 m = reinterpret_cast<const P3*>(M.previous)[q];
                    if (finite3(m) && m.z >= 1.0f) {
                        const float um = b / m.z;
                        Bm = Bm + b;
                        m1 = m1 + um * m.x; m2 = m2 + um * m.y;
                        const float hm = m.z < M.maxBatches ? m.z : M.maxBatches;
                        nm = (taking == 0 || hm < nm) ? hm : nm;
                        ++taking;
                        only = q;
                    }
                }
            }
        }

        P4 c{0.0f, 0.0f, 0.0f, 0.0f};
        P3 pn{0.0f, 0.0f, 0.0f}, pa{0.0f, 0.0f, 0.0f};
        float pw = 0.0f;
        if (valid == 1) {                                  // step 4 of rtowReprojectAccumDevice at the one tap
            c = reinterpret_cast<const P4*>(A.prevColor)[source];
            pn = reinterpret_cast<const P3*>(A.prevNormal)[source];
            pa = reinterpret_cast<const P3*>(A.prevAlbedo)[source];
            pw = A.prevScw[source];
            if (c.w > A.maxHistory) {
                const float s = A.maxHistory / c.w;
                c = P4{c.x * s, c.y * s, c.z * s, A.maxHistory};
                pn = P3{pn.x * s, pn.y * s, pn.z * s};
                pa = P3{pa.x * s, pa.y * s, pa.z * s};
                pw = pw * s;
            }
        } else if (valid > 1) {
            c = P4{(sc0 / B) * n, (sc1 / B) * n, (sc2 / B) * n, n};
            pn = P3{(sn0 / B) * n, (sn1 / B) * n, (sn2 / B) * n};
            pa = P3{(sa0 / B) * n, (sa1 / B) * n, (sa2 / B) * n};
            pw = (sw / B) * n;
        }
        reinterpret_cast<P4*>(A.outColor)[i] = c;
        reinterpret_cast<P3*>(A.outNormal)[i] = pn;
        reinterpret_cast<P3*>(A.outAlbedo)[i] = pa;
        A.outScw[i] = pw;
        if (A.outSource) A.outSource[i] = source;
        if constexpr (kMoments) {
            P3 m{0.0f, 0.0f, 0.0f};
            if (taking == 1) {                             // the rule of rtowReprojectMomentsDevice at the one tap
                m = reinterpret_cast<const P3*>(M.previous)[only];
                if (m.z > M.maxBatches) {
                    const float s = M.maxBatches / m.z;
                    m = P3{m.x * s, m.y * s, M.maxBatches};
                }
            } else if (taking > 1) {
                m = P3{(m1 / Bm) * nm, (m2 / Bm) * nm, nm};
            }
            reinterpret_cast<P3*>(M.out)[i] = m;
        }
    }
}

}  // namespace

hipError_t launchReprojectBilinear(const RtowReprojectParams& p, const ReprojectConstants& k, const RtowRay* rays, const RtowHitBuffers& hits,
                                   const RtowHitBuffers& previousHits, const RtowAccumBuffers& previous, const RtowAccumBuffers& out, const float* previousMoments,
                                   int maxBatches, float* outMoments, int32_t* outSource, hipStream_t stream)
{
    const ReprojectArgs A = reprojectArgs(p, k, rays, hits, previousHits, previous, out, outSource);
    const ReprojectMomentsArgs M{previousMoments, outMoments, (float)maxBatches};
    if (outMoments)
        hipLaunchKernelGGL(reproject_bilinear_kernel<true>, dim3(reprojectBlocks(A)), dim3(kReprojectBlock), 0, stream, A, M);
    else
        hipLaunchKernelGGL(reproject_bilinear_kernel<false>, dim3(reprojectBlocks(A)), dim3(kReprojectBlock), 0, stream, A, M);
    return hipGetLastError();
}

}  // namespace rtow
