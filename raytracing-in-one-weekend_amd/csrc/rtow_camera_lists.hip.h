// rtow_camera_lists.hip.h - which leaf children of a pixel's beam can be left off its camera-ray node list (primary_candidates_kernel, rtow_kernels.hip).
// Plain floats in, a verdict out, no device-only builtins: the kernel calls these functions once per view, a host shim (tests/native/camera_lists_shim.cpp)
// holds them to their contract without a GPU.  Nothing here is on the batch path; the arithmetic is double, so that what is left to bound is the rounding of
// the SAMPLE kernel's fp32 programs and not this file's own.
//
// The beam.  Every camera ray of the pixel is p(s) = ro + s * u, |ro - o| <= R, u a unit vector, and the centre ray q(s) = o + s * dc stays within
//     width(s) = (R + (s + R) * spread) * 1.01 + 1e-5 * (1 + s)
// of it (the kernel's own bound and its own slack, primary_candidates_kernel: `delta` with far = s).  The sample kernel's ray is (ro, rd) in fp32 with
// rd = normalize(...): |rd| = 1 within 2^-22, so its parameter t and the arc length s differ by that relative amount.
//
// What sphere_hit (rtow_hit_tests.hip.h) can report.  With oc = ro - c (each component rounded once: the centre seen by the test is off by at most u |oc|,
// u = 2^-24), X = |oc|, rho = |radius|, A = dot(rd, rd), B = dot(oc, rd), m = the ray's true miss distance of the centre:
//     b    = fl(dot(oc, rd))            |b - B|          <= 3 u X |rd|        (three rounded products, two rounded sums)
//     c    = fl(fl(dot(oc, oc)) - fl(r r))   |c - (X^2 - rho^2)| <= 4 u X^2 + 2 u rho^2
//     disc = fl(fl(b b) - fl(a c))      true value D = B^2 - A (X^2 - rho^2) = A (rho^2 - m^2)
//     |fl(b b) - B^2| <= 7 u X^2,  |fl(a c) - A C| <= 8 u X^2 + 6 u rho^2 (a's own 3 u included),  the last subtraction <= 2 u X^2 + u rho^2
//     => |disc - D| <= 17 u X^2 + 7 u rho^2 (A = 1 within 2^-22)  <  E(X, rho) = 32 u (X^2 + rho^2) = 2^-19 (X^2 + rho^2)         [the allowance]
// A hit is reported only if disc > 0, hence only if m^2 < rho^2 + E: the test sees a ball of radius  rhoSeen = sqrt(rho^2 + E)  at most (for rho = 0.01 at
// X = 1000 that is 1.38: the far, small sphere of the comment at the leaf boxes in rtow_bvh.cpp), and it is certain to see one of  sqrt(rho^2 - E).
// A reported t is (-b -+ sq) / a with sq = sqrt(disc) <= sqrt(D + E): the point ro + t rd then lies within rhoSeen + 3 u X of the centre, whichever root.
//
// shift(c) = 2^-21 (|o| + |c| + R): the rounding of ro = fl(o + offset) and of oc = fl(ro - c), eight times over.
//
// Rule (a), unreachable.  A reported hit of (c, rho) puts a point p(s) of the ray within rhoSeen + 3 u X of c, so q(s) lies within rhoSeen + 3 u X + width(s) + shift
// of c for that same s >= 0.  width is linear in s: if the centre ray stays outside the ball that grows with it, for every s >= 0 (a quadratic in s, its least value
// in closed form), no ray of the pixel is ever reported as hitting the sphere.  A bound at the sphere's far end instead (one width for all s) keeps the ground
// (rho = 1000, far end 2000 away) under pixels that look a whole unit above the horizon at 1080p; this one follows the beam.
//
// Rule (b), hidden.  A static sphere (cA, rhoA) COVERS the pixel when every ray of the pixel is certain to be reported as hitting it:
//   * the closest approach of the centre ray lies ahead, tcA > 0, and  mMax = |q(tcA) - cA| + width(tcA) + shift  bounds every ray's miss distance;
//     Dlow = rhoA^2 - mMax^2 - E > 0 bounds disc (and D) from below for every ray, and sqrt(Dlow) >= 2^-16 (X + rhoA + |cA|): the ray passes the ball's inside
//     over a length of 2 sqrt(Dlow) at least, far more than the rounding of the slab test (a few u of its distances) and of the leaf's box [cA -+ rhoA] in fp32 -
//     a ray through the shrunk ball passes the guard box that encloses the sphere, so the exact test of A runs;
//   * the origin and the lens lie outside the ball A sees: gap = |cA - o| - R - rhoSeenA - shift, and the first root's numerator n0 = -b - sq is positive for
//     every ray: -B - sqrt(D) = A t0 >= gap (1 - 2^-22), |b - B| <= 3 u X, |sq - sqrt(D)| <= E / (2 sqrt(Dlow)) + 2 u rhoA, so gap > 0.001 + 4 (the sum of these)
//     leaves the hit beyond the reference's 0.001 with room to spare; the quotient of a positive finite n0 by a = 1 is positive and finite: the FIRST root is reported;
//   * that root is (-b - sq) / a <= -b / a whatever the error of sq, and -B / A is the ray's own closest approach to cA, at most tcA + |cA - o| * spread + R in
//     arc length: every ray of the pixel reports A at  t <= tA = (tcA + width(|cA - o|) + 2^-21 X) (1 + 2^-20)  (width(|cA - o|) >= |cA - o| * spread + R;
//     2^-20: the roundings of n0 and of the quotient, and |rd| against 1).
// Then no ray's nearest hit lies beyond tA, and a static sphere (cB, rhoB) can go if no ray of the pixel can be reported as hitting it at t <= tA: such a report
// puts q(s), for some s <= tA (1 + 2^-20), within rB = rhoSeenB + 3 u X + width(tA) + shift of cB.  With the origin outside that ball the centre ray enters it at
// sIn = tcB - sqrt(rB^2 - dB^2) (dB its miss distance; never, if dB >= rB or tcB <= 0): B goes if sIn > tA (1 + 2^-19) + 1e-6 - strictly and with a margin, so a
// tie at a bit-identical distance never involves B.  Among several covering spheres the smallest tA counts.
//
// What the margins cost (cover scene, 1920 x 1080, pinhole; HISTORY.md, profiles/r20_camera_lists.json): the lists hold 0.81 nodes on average instead of 2.14.  The
// allowance E is relative to X^2 + rho^2, so the ground (rho = 1000) is seen 0.002 units larger than it is; a growth RELATIVE to its radius (0.1 %) would be a whole
// unit, which in a CPU restatement of an earlier form of these rules kept 13 % more nodes on the lists (1.28 instead of 1.13 a list).
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define RTOW_CAMERA_LISTS_OWN_QUALIFIERS 1
#endif

namespace rtow {

// The pixel's beam as primary_candidates_kernel computes it, and whether anything may be pruned in this pixel at all
struct CameraBeam {
    double ox, oy, oz;      // view origin
    double dx, dy, dz;      // centre direction (unit within fp32 rounding)
    double R, spread;       // lens bound and angular spread, both with the kernel's slack
    double oLen;            // |o|
    double dd;              // |dc|^2
    bool prunable;          // false: every verdict is "stays" and nothing covers
};

__host__ __device__ inline bool camera_lists_finite(double x) { return x - x == 0.0; }

// ok: the kernel's own `ok` (gmin > 4 R, chord and gmin not NaN).  A pixel is left alone too when any quantity is not finite, when the lens bound is not below
// a quarter of the nearest image-plane distance, or when a direction component is zero (its reciprocal is not finite before the kernel clamps it).
__host__ __device__ inline CameraBeam camera_beam(float ox, float oy, float oz, float dx, float dy, float dz, float R, float spread, float gmin, bool ok)
{
    CameraBeam b;
    b.ox = ox; b.oy = oy; b.oz = oz; b.dx = dx; b.dy = dy; b.dz = dz; b.R = R; b.spread = spread;
    const double oo = b.ox * b.ox + b.oy * b.oy + b.oz * b.oz, dd = b.dx * b.dx + b.dy * b.dy + b.dz * b.dz;
    b.oLen = __builtin_sqrt(oo);
    b.dd = dd;
    b.prunable = ok && camera_lists_finite(oo) && camera_lists_finite(dd) && camera_lists_finite((double)R) && camera_lists_finite((double)spread) &&
                 camera_lists_finite((double)gmin) && (double)gmin > 4.0 * (double)R && R >= 0.0f && spread >= 0.0f &&
                 dx != 0.0f && dy != 0.0f && dz != 0.0f && dd > 0.999 && dd < 1.001;
    return b;
}

__host__ __device__ inline double camera_beam_width(const CameraBeam& b, double s) { return (b.R + (s + b.R) * b.spread) * 1.01 + 1e-5 * (1.0 + s); }

// A static identity-rotation sphere against the centre ray
struct CameraSphere {
    double tc;        // parameter of the centre ray's closest approach to the centre (may be negative)
    double d;         // the centre's distance from the LINE of the centre ray
    double w;         // |c - o|
    double rho;       // |radius|
    double X;         // the most |oc| can be: w + R
    double E;         // the allowance on disc
    double rhoSeen;   // sqrt(rho^2 + E)
    double cLen;      // |c|
    double shift;
    bool finite;
};

__host__ __device__ inline CameraSphere camera_sphere(const CameraBeam& b, float cx, float cy, float cz, float radius)
{
    CameraSphere s;
    const double wx = (double)cx - b.ox, wy = (double)cy - b.oy, wz = (double)cz - b.oz;
    s.rho = radius < 0 ? -(double)radius : (double)radius;
    s.tc = wx * b.dx + wy * b.dy + wz * b.dz;
    const double px = wx - s.tc * b.dx, py = wy - s.tc * b.dy, pz = wz - s.tc * b.dz;
    s.d = __builtin_sqrt(px * px + py * py + pz * pz);
    s.w = __builtin_sqrt(wx * wx + wy * wy + wz * wz);
    s.X = s.w + b.R;
    s.E = (s.X * s.X + s.rho * s.rho) * (1.0 / 524288.0);                 // 2^-19
    s.rhoSeen = __builtin_sqrt(s.rho * s.rho + s.E);
    s.cLen = __builtin_sqrt((double)cx * cx + (double)cy * cy + (double)cz * cz);
    s.shift = (b.oLen + s.cLen + b.R) * (1.0 / 2097152.0);                  // 2^-21
    s.finite = camera_lists_finite(s.w) && camera_lists_finite(s.rho) && camera_lists_finite(s.cLen) && camera_lists_finite(s.tc) && camera_lists_finite(s.d);
    return s;
}

// 3 u X: the rounding of b as a distance along the ray
__host__ __device__ inline double camera_b_rounding(const CameraSphere& s) { return s.X * (3.0 / 16777216.0); }

// true: the origin or the lens may lie inside the ball the exact test sees - such a sphere is never dropped and never covers
__host__ __device__ inline bool camera_sphere_holds_origin(const CameraBeam& b, const CameraSphere& s)
{
    return !(s.w - b.R - s.rhoSeen - camera_b_rounding(s) - s.shift > 0.0);
}

// Rule (a): no ray of the pixel can be reported as hitting the sphere.  Every doubt says "stays" (false).
__host__ __device__ inline bool camera_sphere_unreachable(const CameraBeam& b, float cx, float cy, float cz, float radius)
{
    if (!b.prunable) return false;
    const CameraSphere s = camera_sphere(b, cx, cy, cz, radius);
    if (!s.finite || camera_sphere_holds_origin(b, s)) return false;
    // |q(s) - c|^2 > (r0 + k s)^2 for every s >= 0, with width(s) = w0 + k s:  (|dc|^2 - k^2) s^2 - 2 (tc + r0 k) s + (w^2 - r0^2) > 0
    const double k = b.spread * 1.01 + 1e-5, w0 = camera_beam_width(b, 0.0);
    const double r0 = s.rhoSeen + camera_b_rounding(s) + w0 + s.shift;
    const double a2 = b.dd - k * k, h = s.tc + r0 * k, c0 = s.w * s.w - r0 * r0;
    if (!(a2 > 0.01) || !(c0 > 0.0)) return false;                       // a beam wider than a right angle, or the origin inside the grown ball: stays
    const double low = h > 0.0 ? c0 - h * h / a2 : c0;                   // the least value over s >= 0
    return low > 1e-9 * (s.w * s.w + r0 * r0);                           // strictly, beyond the rounding of these few double operations
}

// Rule (b), first half: does the sphere cover the pixel, and by which parameter tA is it reported on every ray?  false: it does not (or cannot be shown to)
__host__ __device__ inline bool camera_sphere_covers(const CameraBeam& b, float cx, float cy, float cz, float radius, double& tA)
{
    if (!b.prunable) return false;
    const CameraSphere s = camera_sphere(b, cx, cy, cz, radius);
    if (!s.finite || camera_sphere_holds_origin(b, s) || !(s.tc > 0.0)) return false;
    const double mMax = s.d + camera_beam_width(b, s.tc) + s.shift;
    const double Dlow = s.rho * s.rho - mMax * mMax - s.E;
    if (!(Dlow > 0.0)) return false;
    const double root = __builtin_sqrt(Dlow);
    if (!(root >= (s.X + s.rho + s.cLen) * (1.0 / 65536.0))) return false;   // through the inside by far more than the slab test and the fp32 box round
    const double gap = s.w - b.R - s.rhoSeen - s.shift;
    const double n0Rounding = camera_b_rounding(s) + s.E / (2.0 * root) + s.rho * (2.0 / 16777216.0);
    if (!(gap * (1.0 - 1.0 / 4194304.0) > 0.001 + 4.0 * n0Rounding)) return false;
    const double t = (s.tc + camera_beam_width(b, s.w) + s.X * (1.0 / 2097152.0)) * (1.0 + 1.0 / 1048576.0);
    if (!camera_lists_finite(t)) return false;
    tA = t;
    return true;
}

// Rule (b), second half: no ray of the pixel can be reported as hitting the sphere at t <= tA (tA from camera_sphere_covers, the smallest among the covering spheres)
__host__ __device__ inline bool camera_sphere_hidden(const CameraBeam& b, float cx, float cy, float cz, float radius, double tA)
{
    if (!b.prunable || !(tA > 0.0) || !camera_lists_finite(tA)) return false;
    const CameraSphere s = camera_sphere(b, cx, cy, cz, radius);
    if (!s.finite) return false;
    const double tEnd = tA * (1.0 + 1.0 / 524288.0) + 1e-6;               // strictly beyond tA, with a margin
    const double rB = s.rhoSeen + camera_b_rounding(s) + camera_beam_width(b, tEnd) + s.shift;
    if (!(s.w > rB + b.R)) return false;                                    // the origin or the lens inside the grown ball: stays
    if (!(s.tc > 0.0) || !(s.d < rB)) return s.tc <= 0.0 || s.d >= rB;      // the centre ray never enters the grown ball (NaN: stays)
    const double sIn = s.tc - __builtin_sqrt(rB * rB - s.d * s.d);
    return sIn > tEnd;
}

} // namespace rtow

#ifdef RTOW_CAMERA_LISTS_OWN_QUALIFIERS
#undef __host__
#undef __device__
#undef RTOW_CAMERA_LISTS_OWN_QUALIFIERS
#endif
