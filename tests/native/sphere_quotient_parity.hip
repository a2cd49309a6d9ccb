// Test-only program for rtow::sphere_hit_shared_rcp (raytracing-in-one-weekend_amd/csrc/rtow_hit_tests.hip.h): the exact sphere test of the TEST stage, which takes its
// one quotient a candidate from the run's reciprocal, against rtow::sphere_hit on the same operands - the hit flag and the bits of t.
//
// Part 1 - the two functions on about 2^25 rays and spheres, a = dot(d, d), its range test and RN(1 / a) formed the way the TEST stage forms them:
//   (half)  random rays against random spheres: origins outside, inside and on the sphere; directions normalised, reflected and not renormalised, or scaled by
//           2^-20 .. 2^20 (a on both sides of 2^-31 and 2^33, the ends of the reciprocal's range: biased exponents 95 | 96 and 159 | 160)
//   (0)     the ground sphere: radius 1000, the origin 0.001 above it
//   (1)     axis rays whose first numerator lies around 2^-63 (biased exponents 63 .. 66: the low end of the numerators' range), a in range
//   (2)     axis rays from the surface through the centre whose second numerator lies around 2^64 (biased exponents 189 .. 191) or is infinite: a finite 2^65 and more
//           cannot come out of the function's own arithmetic - n <= |b| + sqrt(disc) with b * b and disc finite, so both terms are below 2^64 - which part 2 makes up for
//   (3)     the cold redo: a first quotient that overflows (a subnormal) with a positive second numerator behind it.  (One that underflows to zero while the second
//           root's does not needs n0 / n1 < 2^-24 next to t1 < 2^-125: out of reach of the function's arithmetic with a finite a.  Part 2 has it.)
//   (4)     a of 0, subnormal, infinite and NaN
//   (5)     exactly tangent rays (discriminant 0: every product and sum exact on small integers times powers of two) and rays that miss (negative discriminant)
// Part 2 - rtow::sphere_root_quotient, the part of the function behind the square root, on 2^25 arbitrary triples (n0, n1, a) against sphere_hit's own text for it:
//   numerators with biased exponents around 63 | 64 and 191 | 192, divisors around 95 | 96 and 159 | 160, arbitrary bit patterns (zeros, subnormals, infinities,
//   NaNs, negative values) among them.
// Every line "<what> <count>" below the two totals says how many cases of a kind the sweep produced; tests/test_gpu_sphere_quotient.py requires each to be positive.
// Exit status 1 with any mismatch.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "../../raytracing-in-one-weekend_amd/csrc/rtow_hit_tests.hip.h"

namespace {

enum Kind {
    K_MISMATCH, K_HIT, K_FAST, K_SECOND_ROOT, K_REDO, K_REDO_HIT, K_DISC_NEG, K_DISC_ZERO, K_ORIGIN_INSIDE, K_ORIGIN_ON, K_ORIGIN_OUTSIDE,
    K_N_EXP_63, K_N_EXP_64, K_N_EXP_191, K_N_EXP_192, K_N_INF, K_A_EXP_95, K_A_EXP_96, K_A_EXP_159, K_A_EXP_160, K_A_ZERO, K_A_SUBNORMAL, K_A_INF, K_A_NAN, K_COUNT
};
const char* const kKindNames[K_COUNT] = {
    "mismatches", "hits", "quotients from the reciprocal", "second root taken", "cold redo entered", "cold redo hits", "negative discriminants", "zero discriminants",
    "origins inside", "origins on the sphere", "origins outside", "numerator exponent 63", "numerator exponent 64", "numerator exponent 191", "numerator exponent 192",
    "numerator infinite", "a exponent 95", "a exponent 96", "a exponent 159", "a exponent 160", "a zero", "a subnormal", "a infinite", "a NaN"};

__device__ __forceinline__ unsigned mix(unsigned long long& s)     // splitmix64, upper half
{
    s += 0x9E3779B97F4A7C15ull;
    unsigned long long z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (unsigned)((z ^ (z >> 31)) >> 32);
}
__device__ __forceinline__ float unit(unsigned long long& s) { return (float)(mix(s) >> 8) * (1.0f / 16777216.0f); }             // [0, 1)
__device__ __forceinline__ float pow2(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }                               // e in [-126, 127]
__device__ __forceinline__ float around(int e, unsigned long long& s) { return pow2(e) * (1.0f + unit(s)); }                      // [2^e, 2^(e+1))
__device__ __forceinline__ rtow::V3 direction(unsigned long long& s)
{
    rtow::V3 v;
    do { v = rtow::v3(2.0f * unit(s) - 1.0f, 2.0f * unit(s) - 1.0f, 2.0f * unit(s) - 1.0f); } while (rtow::dot(v, v) > 1.0f || rtow::dot(v, v) < 0.01f);
    return rtow::normalize(v);
}
__device__ __forceinline__ unsigned biased(float x) { return (__float_as_uint(x) >> 23) & 0xffu; }

struct Tally {
    unsigned n[K_COUNT];
    __device__ void add(int k, bool on = true) { n[k] += on ? 1u : 0u; }
};

__device__ __forceinline__ void classify_a(Tally& t, float a)
{
    const unsigned e = biased(a), m = __float_as_uint(a) & 0x7fffffu;
    t.add(K_A_EXP_95, e == 95); t.add(K_A_EXP_96, e == 96); t.add(K_A_EXP_159, e == 159); t.add(K_A_EXP_160, e == 160);
    t.add(K_A_ZERO, e == 0 && m == 0); t.add(K_A_SUBNORMAL, e == 0 && m != 0); t.add(K_A_INF, e == 255 && m == 0); t.add(K_A_NAN, e == 255 && m != 0);
}

// what the run's TEST stage forms next to `a` (rtow_sample_kernel.hip.h)
__device__ __forceinline__ bool divisor_ok(float a) { return (__float_as_uint(a) - 0x30000000u) < 0x20000000u; }

// sphere_hit's text behind the square root (rtow_hit_tests.hip.h), for part 2.  A copy kept in step BY HAND: whoever changes the two `if (n > 0)` blocks of sphere_hit
// changes these with them (part 1 compares against sphere_hit itself and would show a copy that has fallen behind on every operand the function can produce).
__device__ __forceinline__ bool reference_roots(float n0, float n1, float a, float& tOut)
{
    if (n0 > 0) {
        const float t = n0 / a;
        if (t < __builtin_inff() && t > 0) { tOut = t; return true; }
    }
    if (n1 > 0) {
        const float t = n1 / a;
        if (t < __builtin_inff() && t > 0) { tOut = t; return true; }
    }
    return false;
}

__device__ __forceinline__ void classify_roots(Tally& t, float n0, float n1, float a, bool hit)
{
    const bool first = n0 > 0;
    const float n = first ? n0 : n1;
    if (!(n > 0)) return;
    const unsigned e = biased(n);
    t.add(K_SECOND_ROOT, !first);
    t.add(K_N_EXP_63, e == 63); t.add(K_N_EXP_64, e == 64); t.add(K_N_EXP_191, e == 191); t.add(K_N_EXP_192, e == 192); t.add(K_N_INF, e == 255);
    const bool fast = divisor_ok(a) && e >= 64 && e <= 191;
    t.add(K_FAST, fast);
    if (!fast && first && n1 > 0) {
        const float q = n0 / a;
        const bool redo = !(q < __builtin_inff() && q > 0);
        t.add(K_REDO, redo);
        t.add(K_REDO_HIT, redo && hit);
    }
}

__global__ void sweep_spheres(unsigned perThread, unsigned long long* counts, float* firstBad)
{
    using namespace rtow;
    unsigned long long s = 0x5eed5ull + (unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x) * 0x100000001B3ull;
    Tally tally = {};
    for (unsigned k = 0; k < perThread; k++) {
        const unsigned family = mix(s) % 12u;                     // family 0 six times in twelve, the others once each
        V3 oc, d;
        float radius;
        if (family >= 6u) {
            const V3 centre = v3(20.0f * unit(s) - 10.0f, 20.0f * unit(s) - 10.0f, 20.0f * unit(s) - 10.0f);
            radius = 0.01f + 5.0f * unit(s) * unit(s);
            const unsigned where = mix(s) % 3u;
            V3 origin = v3(20.0f * unit(s) - 10.0f, 20.0f * unit(s) - 10.0f, 20.0f * unit(s) - 10.0f);
            if (where == 1u) origin = add(centre, scale(radius * 0.95f * unit(s), direction(s)));
            if (where == 2u) origin = add(centre, scale(radius, direction(s)));
            d = direction(s);
            if (mix(s) & 1u) d = normalize(sub(add(centre, scale(0.9f * radius * unit(s), direction(s))), origin));      // one ray in two at a point inside the sphere
            const unsigned form = mix(s) % 3u;
            if (form == 1u) d = reflect(d, direction(s));
            if (form == 2u) d = scale(around((int)(mix(s) % 41u) - 20, s), d);
            oc = sub(origin, centre);
            const float side = dot(oc, oc) - radius * radius;
            tally.add(K_ORIGIN_INSIDE, side < 0); tally.add(K_ORIGIN_ON, where == 2u); tally.add(K_ORIGIN_OUTSIDE, side > 0);
        } else if (family == 0u) {
            radius = 1000.0f;
            const V3 up = direction(s);
            oc = scale(1000.0f + 0.001f, v3(up.x, up.y < 0 ? -up.y : up.y, up.z));
            d = direction(s);
        } else if (family == 1u) {
            // oc = (-dist, 0, 0), d = (k, 0, 0), radius = dist (1 - g): n0 = k dist g, about 2^-45 x 2^-18 x [1/2, 2)
            const int kd = (int)(mix(s) % 31u) - 15;
            const float kk = around(kd, s), dist = around(-45 - kd, s);
            radius = dist * (1.0f - pow2(-19) * (1.0f + 3.0f * unit(s)));
            oc = v3(-dist, 0.0f, 0.0f);
            d = v3(kk, 0.0f, 0.0f);
        } else if (family == 2u) {
            // from the surface through the centre: c = 0, n0 = 0, n1 = 2 k radius around 2^64; k radius of 2^64 and more squares to infinity
            const int kd = 1 + (int)(mix(s) % 16u);                // (radius * radius stays finite)
            const float kk = around(kd, s);
            radius = pow2(62 - kd) * (0.5f + 2.0f * unit(s)) * (1.0f + unit(s));
            oc = v3(-radius, 0.0f, 0.0f);
            d = v3(kk, 0.0f, 0.0f);
        } else if (family == 3u) {
            // k = 2^-70 (a subnormal), dist around 2^60, radius half of it: n0 / a around 2^129
            const float dist = around(60, s);
            radius = dist * (0.4f + 0.2f * unit(s));
            oc = v3(-dist, 0.0f, 0.0f);
            d = v3(around(-70, s), 0.0f, 0.0f);
        } else if (family == 4u) {
            // rays at the centre.  0: |d| = 2^-80 against a sphere 2^40 away - dot(d, d) underflows to zero, b * b does not; 1: a subnormal; 2: a infinite, from inside
            // (a * c = -inf: the discriminant and the second numerator are +inf); 3: a NaN
            const unsigned what = mix(s) & 3u;
            const V3 to = direction(s);
            radius = what == 0u ? pow2(39) : 0.5f + unit(s);
            oc = scale(what == 0u ? -pow2(40) : what == 2u ? -0.25f : -3.0f, to);
            d = scale(what == 0u ? around(-80, s) : what == 1u ? around(-70, s) : around(70, s), to);
            if (what == 3u) d = v3(__builtin_nanf(""), unit(s), unit(s));
        } else {
            // small integers times powers of two: every product and sum is exact.  oc = (-i, j, 0) 2^e, d = (2^f, 0, 0), radius j 2^e: tangent; radius below: a miss
            const float e = pow2((int)(mix(s) % 21u) - 10), f = pow2((int)(mix(s) % 21u) - 10);
            const float i = (float)(1u + mix(s) % 15u), j = (float)(2u + mix(s) % 14u);
            radius = (mix(s) & 1u) ? j * e : (j - 1.0f) * e;
            oc = v3(-i * e, j * e, 0.0f);
            d = v3(f, 0.0f, 0.0f);
        }
        const float a = dot(d, d);
        const bool aOk = divisor_ok(a);
        const float ya = RTOW_RCP(a);
        float tRef = 0.0f, tGot = 0.0f;
        const bool ref = sphere_hit(oc, d, a, radius, tRef);
        const bool got = sphere_hit_shared_rcp(oc, d, a, ya, aOk, radius, tGot);
        const bool bad = ref != got || (ref && __float_as_uint(tRef) != __float_as_uint(tGot));
        if (bad && !tally.n[K_MISMATCH] && atomicCAS((unsigned*)&firstBad[15], 0u, 1u) == 0u) {
            firstBad[0] = oc.x; firstBad[1] = oc.y; firstBad[2] = oc.z; firstBad[3] = d.x; firstBad[4] = d.y; firstBad[5] = d.z; firstBad[6] = radius; firstBad[7] = tRef; firstBad[8] = tGot;
        }
        tally.add(K_MISMATCH, bad);
        tally.add(K_HIT, ref);
        classify_a(tally, a);
        // the operands of the quotient, as both functions form them
        const float b = dot(oc, d), c = dot(oc, oc) - radius * radius, disc = b * b - a * c;
        tally.add(K_DISC_NEG, disc < 0); tally.add(K_DISC_ZERO, disc == 0);
        if (disc > 0) {
            const float sq = RTOW_SQRT(disc);
            classify_roots(tally, -b - sq, -b + sq, a, ref);
        }
    }
    for (int k = 0; k < K_COUNT; k++)
        if (tally.n[k]) atomicAdd(&counts[k], (unsigned long long)tally.n[k]);
}

__global__ void sweep_roots(unsigned perThread, unsigned long long* counts, float* firstBad)
{
    unsigned long long s = 0xabcdefull + (unsigned long long)(blockIdx.x * blockDim.x + threadIdx.x) * 0x100000001B3ull;
    Tally tally = {};
    for (unsigned k = 0; k < perThread; k++) {
        unsigned u[3];
        for (int i = 0; i < 3; i++) {
            u[i] = mix(s);
            const unsigned r = mix(s);
            if (r & 3u) {
                // exponents within +-3 of the ends of the two ranges (64, 191 for the numerators; 96, 159 for the divisor); one case in four keeps its arbitrary bits
                const unsigned ends[4] = {64u, 191u, 96u, 159u};
                const unsigned e = ends[(i == 2 ? 2u : 0u) + ((r >> 2) & 1u)] + ((r >> 3) % 7u) - 3u;
                u[i] = (u[i] & 0x807fffffu) | (e << 23);
                if (i == 2 || ((r >> 8) & 3u)) u[i] &= 0x7fffffffu;                    // a = dot(d, d) is not negative; most numerators are positive
            }
            if (i == 2 && ((r >> 12) & 15u) == 0u) {
                // one divisor in sixteen: 0, a subnormal, infinity, a NaN
                const unsigned what = (r >> 16) & 3u;
                u[i] = what == 0u ? 0u : what == 1u ? (u[i] & 0x7fffffu) | 1u : what == 2u ? 0x7f800000u : 0x7fc00000u | (u[i] & 0x3fffffu);
            }
        }
        const float n0 = __uint_as_float(u[0]), n1 = __uint_as_float(u[1]), a = __uint_as_float(u[2]);
        const bool aOk = divisor_ok(a);
        const float ya = RTOW_RCP(a);
        float tRef = 0.0f, tGot = 0.0f;
        const bool ref = reference_roots(n0, n1, a, tRef);
        const bool got = rtow::sphere_root_quotient(n0, n1, a, ya, aOk, tGot);
        const bool bad = ref != got || (ref && __float_as_uint(tRef) != __float_as_uint(tGot));
        if (bad && !tally.n[K_MISMATCH] && atomicCAS((unsigned*)&firstBad[15], 0u, 1u) == 0u) { firstBad[0] = n0; firstBad[1] = n1; firstBad[2] = a; firstBad[7] = tRef; firstBad[8] = tGot; }
        tally.add(K_MISMATCH, bad);
        tally.add(K_HIT, ref);
        classify_a(tally, a);
        classify_roots(tally, n0, n1, a, ref);
    }
    for (int k = 0; k < K_COUNT; k++)
        if (tally.n[k]) atomicAdd(&counts[k], (unsigned long long)tally.n[k]);
}

} // namespace

int main()
{
    unsigned long long* counts; float* first;
    if (hipMalloc(&counts, K_COUNT * sizeof(unsigned long long)) != hipSuccess || hipMalloc(&first, 16 * sizeof(float)) != hipSuccess) return 2;
    unsigned long long total = 0;
    for (int part = 1; part <= 2; part++) {
        unsigned long long h[K_COUNT]; float f[16];
        (void)hipMemset(counts, 0, K_COUNT * sizeof(unsigned long long)); (void)hipMemset(first, 0, 16 * sizeof(float));
        if (part == 1) sweep_spheres<<<1024, 256>>>(128u, counts, first);            // 2^18 threads x 2^7 cases
        else sweep_roots<<<1024, 256>>>(128u, counts, first);
        if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 3; }
        (void)hipMemcpy(h, counts, sizeof(h), hipMemcpyDeviceToHost); (void)hipMemcpy(f, first, sizeof(f), hipMemcpyDeviceToHost);
        printf("part %d %s %llu: %llu mismatches\n", part, part == 1 ? "rays and spheres" : "root triples", 1ull << 25, h[K_MISMATCH]);
        if (h[K_MISMATCH]) {
            if (part == 1) printf("part 1 first: oc %a %a %a d %a %a %a radius %a sphere_hit %a shared %a\n", f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]);
            else printf("part 2 first: n0 %a n1 %a a %a reference %a shared %a\n", f[0], f[1], f[2], f[7], f[8]);
        }
        for (int k = 1; k < K_COUNT; k++) printf("part %d %s %llu\n", part, kKindNames[k], h[k]);
        total += h[K_MISMATCH];
    }
    printf("total %llu mismatches\n", total);
    fflush(stdout);
    return total ? 1 : 0;
}
