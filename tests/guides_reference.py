"""rtowTraceGuideRaysDevice's specification (include/rtow.h) restated in numpy: what every output of every ray must be, bit for bit.  Nothing here comes from the library:
a Python loop per ray over the oracle's nearest hit (OracleScene.nearest_hit: distance, normal and entity of the sample path's FindHits[0]) with steps 2-4 of the
specification in float32, one binary32 operation per numpy operation.  Where several entities are hit at the bit-identical nearest distance, step 1 names the one that
rtowTraceRaysDevice names - the first in the reference tree's leaf order (TieOrder below, from the oracle's own tree and Entity.Hit) - which is FindHits[0] as long as the
reference's sort is stable (up to 16 hits on the ray) and may be another of the tied entities beyond that (twin_row: up to 60 hits on a ray).  The refraction is the
oracle's Material.Refract (oracle_kat_refract); Material.IsPerfectSpecular and Albedo.SampleColor(TexCoords) are tests/shade_hits_reference.py's.
tests/test_guides_reference.py anchors the restatement against the oracle's Material.Scatter and its sample path without a GPU.

A NaN that an operation creates has the sign bit clear on gfx950 and set on x86 (tests/shade_hits_reference.py): compare with its same_bits."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_hits_reference as shade  # noqa: E402

abi = shade.abi
f32 = np.float32
END_SKY, END_SURFACE, END_CUT = 0, 1, 2


def dot(a, b):
    """a.x * b.x + a.y * b.y + a.z * b.z, left to right"""
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def normalize(v):
    """math.normalize: (1 / sqrt(dot(v, v))) * v"""
    return (f32(f32(1) / np.sqrt(dot(v, v), dtype=f32)) * v).astype(f32)


def reflect(i, n):
    """math.reflect: i - (2 * n) * dot(i, n)"""
    return (i - ((f32(2) * n).astype(f32) * dot(i, n)).astype(f32)).astype(f32)


def _c3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def scatter(oracle, material, rd, normal, albedo):
    """step 3: (sdir, tint, took the reflection branch of a dielectric)"""
    if material.type == abi.MATERIAL_STANDARD:
        return reflect(rd, normal), albedo, False
    assert material.type == abi.MATERIAL_DIELECTRIC
    ior = f32(material.parameter)
    rn = normalize(normal)
    if dot(rd, rn) > 0:
        on, nn = (-rn).astype(f32), ior
    else:
        on, nn = rn, f32(f32(1) / ior)
    out = (C.c_float * 3)()
    if oracle.load().oracle_kat_refract(_c3(rd), _c3(on), float(nn), out) == 1:
        return np.asarray(list(out), dtype=f32), albedo, False
    return reflect(rd, rn), np.ones(3, dtype=f32), True


def next_origin(point, sdir, normal):
    """step 4: P + 0.001f * (dot(sdir, N) >= 0 ? N : -N)"""
    off = normal if dot(sdir, normal) >= 0 else (-normal).astype(f32)
    return (point + (f32(0.001) * off).astype(f32)).astype(f32)


class TieOrder:
    """rtowTraceRaysDevice's rule for hits at the bit-identical nearest distance: of the entities whose own box the ray passes (AxisAlignedBoundingBox.Hit) and whose
    Entity.Hit(ray, 0, +inf) distance has the nearest distance's bits, the one that comes first in the reference tree's leaf order (oracle_kat_hit_tie_order)."""

    def __init__(self, oracle, scene, desc):
        self.lib, self.desc, n = oracle.load(), desc, scene.entity_count
        order = (C.c_int * n)()
        assert self.lib.oracle_kat_hit_tie_order(C.byref(desc), order) == n
        self.rank = np.empty(n, np.int64)
        self.rank[np.asarray(list(order))] = np.arange(n)
        self.bounds = np.zeros((n, 6), f32)
        box = (C.c_float * 6)()
        for e in range(n):
            self.lib.oracle_kat_entity_bounds(C.byref(desc.entities[e]), desc.triangles, desc.triangleCount, box)
            self.bounds[e] = list(box)

    def _near(self, ro, rd, t):
        """entities whose box the ray can be inside of at distance t (float64 slabs with slack; a NaN slab excludes nothing): the only ones that can tie at t"""
        with np.errstate(all="ignore"):
            a = (self.bounds[:, :3].astype(np.float64) - ro) / rd.astype(np.float64)
            b = (self.bounds[:, 3:].astype(np.float64) - ro) / rd.astype(np.float64)
            near, far = np.fmax.reduce(np.fmin(a, b), axis=1), np.fmin.reduce(np.fmax(a, b), axis=1)
            slack = 1e-3 * (1.0 + abs(float(t)))
            return np.flatnonzero(~((near - slack > t) | (far + slack < t)))

    def first(self, ro, rd, time, t, entity, normal):
        """(entity, normal) of the hit rtowTraceRaysDevice reports, given FindHits[0]"""
        out = (C.c_float * 9)()
        o, d = _c3(ro), _c3(rd)
        best, best_normal = entity, normal
        for c in self._near(ro, rd, t):
            c = int(c)
            if c == entity or self.rank[c] > self.rank[best]:
                continue
            if self.lib.oracle_kat_aabb_hit(_c3(self.bounds[c, :3]), _c3(self.bounds[c, 3:]), o, d) != 1:
                continue
            if self.lib.oracle_kat_entity_hit(C.byref(self.desc.entities[c]), self.desc.triangles, self.desc.triangleCount, o, d, float(time), 0.0, float("inf"), out) != 1:
                continue
            if f32(out[0]).view(np.uint32) == f32(t).view(np.uint32):
                best, best_normal = c, np.asarray(out[4:7], dtype=f32)
        return best, best_normal


def chain(oracle, osc, ties, scene, desc, origin, direction, time, max_bounces):
    """One ray: the dict of its outputs (scalars and small arrays) plus "tir": dielectric reflections taken on the way."""
    ro, rd = np.asarray(origin, dtype=f32), np.asarray(direction, dtype=f32)
    T, D, b, tir = np.ones(3, dtype=f32), f32(0), 0, 0
    with np.errstate(all="ignore"):
        while True:
            n, rec = osc.nearest_hit(ro, rd, float(time))
            if n == 0:
                t, entity, N, end = f32(np.inf), -1, np.zeros(3, dtype=f32), END_SKY
                break
            t, N, entity = f32(rec[0]), np.asarray(rec[4:7], dtype=f32), int(rec[7])
            entity, N = ties.first(ro, rd, time, t, entity, N)
            D = f32(D + t)
            P = (ro + (t * rd).astype(f32)).astype(f32)
            m = scene.materials[scene.material_index[entity]]
            if not shade.is_perfect_specular(m):
                end = END_SURFACE
                break
            if b == max_bounces:
                end = END_CUT
                break
            uv = np.zeros(2, dtype=f32)
            if scene.types[entity] == abi.ENTITY_TRIANGLE:
                uv = shade.tex_coords(oracle, desc, entity, ro, rd)
            sdir, tint, reflected = scatter(oracle, m, rd, N, shade.sample_color(scene, m.albedo, uv))
            tir += reflected
            T = (T * tint).astype(f32)
            ro, rd = next_origin(P, sdir, N), sdir
            b += 1
    return {"distance": t, "entityIndex": entity, "normal": N, "origin": ro, "direction": rd, "throughput": T, "pathDistance": D, "bounces": b, "end": end, "tir": tir}


def guides(oracle, scene, desc, rays, max_bounces):
    """Every output of rtowTraceGuideRaysDevice for `rays` (abi.RAY_DTYPE), keyed as abi.GUIDE_OUTPUTS, and the number of dielectric reflections the chains took."""
    n = len(rays)
    out = {"distance": np.zeros(n, f32), "entityIndex": np.zeros(n, np.int32), "normal": np.zeros((n, 3), f32), "rays": np.zeros(n, dtype=np.dtype(abi.RAY_DTYPE)),
           "throughput": np.zeros((n, 3), f32), "pathDistance": np.zeros(n, f32), "bounces": np.zeros(n, np.int32), "end": np.zeros(n, np.uint8)}
    reflections = 0
    osc = oracle.OracleScene(desc)
    ties = TieOrder(oracle, scene, desc)
    try:
        for k in range(n):
            c = chain(oracle, osc, ties, scene, desc, rays["origin"][k], rays["direction"][k], rays["time"][k], max_bounces)
            for name in ("distance", "entityIndex", "normal", "throughput", "pathDistance", "bounces", "end"):
                out[name][k] = c[name]
            out["rays"]["origin"][k], out["rays"]["direction"][k], out["rays"]["time"][k] = c["origin"], c["direction"], rays["time"][k]
            reflections += c["tir"]
    finally:
        osc.close()
    return out, reflections


def mirror_scene(rt):
    """The scene of the end-to-end tests: mirrors (two facing rects, three balls), lambert surfaces and one emitter - every perfectly specular surface is a Standard
    material, so the sample path's walk to its first non-specular hit takes no random decision that changes the direction."""
    S = rt.scenes
    s = S.Scene("mirrors")
    s.add_sphere((0, -1000, 0), 1000, S.lambertian((0.5, 0.5, 0.5)))
    s.add_sphere((0, 1, 0), 1, S.metal((0.9, 0.8, 0.7), 0))
    s.add_sphere((-2.2, 1, 0.5), 1, S.metal((0.7, 0.9, 0.8), 0))
    s.add_sphere((2.2, 1, 0.5), 1, S.lambertian((0.8, 0.2, 0.2)))
    s.add_sphere((0.8, 0.4, 2), 0.4, S.standard((0.1, 0.1, 0.1), 0, 0, emission=(2, 1.5, 1)))
    s.add_sphere((-0.9, 0.3, 2.2), 0.3, S.metal((1, 1, 1), 0))
    s.add_rect((0, 1.5, -3), (8, 3), S.metal((0.95, 0.95, 0.95), 0))
    s.add_rect((0, 1.5, 14.5), (8, 3), S.metal((0.95, 0.95, 0.95), 0))
    s.camera = {"position": [1.5, 1.6, 9.0], "target": [0.0, 1.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    return s


def textured_mirror_scene(rt):
    """textured_scene plus a mirror whose albedo is an Image texture (metallic and glossiness the constant 1: perfectly specular), two triangles in front of the back wall:
    the tint of a chain that follows it is the texel at the triangle's UV"""
    S = rt.scenes
    s = S.textured_scene()
    s.name = "textured + image mirror"
    mirror = abi.Material(abi.MATERIAL_STANDARD, S.image_tex(0, (0.9, 0.8, 0.7)), S._const_tex(1.0), S._none_tex(), S._const_tex(1.0), 0.0)
    S._quad(s, (-2.6, 0.4, -2.5), (-2.6, 3.2, -2.5), (1.4, 3.2, -2.5), (1.4, 0.4, -2.5), mirror, uv0=(0.05, 0.1), uv1=(0.95, 0.9))
    return s


def mirror_params(rt, scene, w, h):
    """the one-sample batch whose AOVs the chain's end point equals: 1 spp, jitter off, lens 0, white noise, traceDepth 9"""
    p = rt.scenes.make_params(scene, w, h, spp=1, trace_depth=9, jitter=False, noise_color=abi.NOISE_WHITE)
    p.view.lensRadius = 0.0
    return p


def expected_aovs(scene, environment, end_rays, end_entity, end_normal, surface):
    """What a one-sample batch from zeroed accumulators holds in its albedo and normal buffers where the chain ends at (end_rays, end_entity): 0 + (emission + albedo) and
    0 + N at a hit, 0 + the sky along the last direction and 0 + -direction on a miss (JOBS/SampleBatchJob.cs:316-328,349-370).  surface: albedo / emission of
    rtowShadeHitsDevice (or its restatement) on (end_rays, end_entity)."""
    hit = (np.asarray(end_entity) >= 0)[:, None]
    albedo = shade.expected_albedo_aov(surface, end_entity)
    normal = (f32(0) + np.where(hit, end_normal, -end_rays["direction"])).astype(f32)
    return albedo, normal
