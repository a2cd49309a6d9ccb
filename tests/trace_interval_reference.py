"""Brute-force reference of the interval ray queries (include/rtow.h: rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice / rtowProbeNearestHitInterval), made of
oracle calls only: per ray, the entities e with oracle_kat_aabb_hit(gate box of e, ray) and oracle_kat_entity_hit(e, ray, time, tMin, tMax); of these the
minimum distance, the set of entities at that minimum (by bits) and any-hit.  No tree, no pruning, no tie rule: what every walk of the product must agree with.

The gate box of an entity is the box of the reference tree's leaf that holds it (oracle_kat_leaf_boxes): the entity's own box (oracle_kat_entity_bounds), except in a
leaf forced at RtowSceneDesc.maxBvhDepth, where it is the union of that leaf's boxes - Raytracer.HitWorld tests every entity of a leaf whose box the ray passes, so a ray
that lies in a face plane of an entity's own box (and fails that box) still meets the entity through the wider one.  Built at depth 32 no scene of the suite has a forced
leaf, and the two are the same bits: asserted below.

A float64 slab test, vectorised over the entities and widened so that it can only over-include, thins the entities out before the oracle's own box test decides
(needed for the meshes).  The module checks itself once per scene: with (0, +inf) its distance bits equal OracleScene.hit_world's on every test ray."""
import ctypes as C

import numpy as np

INF = np.float32(np.inf)

# interval families of the tests, per ray, from the ray's nearest distance d (0, +inf) and one uniform draw u in [0, 1)
FAMILIES = ["null", "tmax_below", "tmax_at", "tmax_above", "tmin_at", "tmin_above", "sub_near", "sub_far", "nan", "negative", "reversed"]
INVALID = ("nan", "negative", "reversed")


def interval_rays(tr, rt, scene, name, mesh_rays=300, mesh_axis_rays=60):
    """tests/test_gpu_trace_rays.py's (`tr`) generated + axis rays, moving scenes with every other ray at a random time; the mesh gets the first few hundred of each kind
    (the brute force is a loop over oracle calls): (pairs, times)"""
    pairs, times, generated = tr._test_rays(rt, scene, name, timed=True)
    if name == "mesh":
        keep = list(range(mesh_rays)) + list(range(generated, generated + mesh_axis_rays))
        pairs, times = [pairs[k] for k in keep], [times[k] for k in keep]
    return pairs, times


def up(x):
    return np.nextafter(np.float32(x), INF)


def down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def family_interval(family, d, u):
    """(tMin, tMax) as float32.  d: the ray's nearest distance under (0, +inf) (+inf on a miss: the families then probe the far end of the float range)."""
    d = np.float32(d)
    u = np.float32(u)
    far = d if np.isfinite(d) else np.float32(100.0)
    return {"null": (np.float32(0), INF),
            "tmax_below": (np.float32(0), down(d)), "tmax_at": (np.float32(0), d), "tmax_above": (np.float32(0), up(d)),
            "tmin_at": (d, INF), "tmin_above": (up(d), INF),
            "sub_near": (np.float32(far * u), np.float32(far * (u + np.float32(0.5)))),      # around the nearest hit or in front of it
            "sub_far": (np.float32(far * (1 + u)), np.float32(far * (1 + 4 * u))),           # behind it
            "nan": (np.float32(np.nan), INF) if u < 0.5 else (np.float32(0), np.float32(np.nan)),
            "negative": (np.float32(-(u + np.float32(2.0 ** -20))), INF),
            "reversed": (up(far), far)}[family]


def interval_is_traced(tmin, tmax):
    return bool(np.float32(0) <= tmin and tmin <= tmax)


class RayCandidates:
    """The entities whose gate box (the box of their reference leaf) the ray passes (the interval plays no part in that), ready for any number of intervals."""

    def __init__(self, ref, origin, direction, time, entities):
        self.ref, self.time, self.entities = ref, float(time), entities
        self.o, self.d = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_float * 3)(*[float(x) for x in direction])

    def query(self, tmin, tmax):
        """(distance as float32, the entities at that distance by bits, any-hit).  A miss: (+inf, empty, False).  An interval that is not traced: a miss.
        A distance that is not below +inf never counts (include/rtow.h)."""
        if not interval_is_traced(np.float32(tmin), np.float32(tmax)):
            return INF, frozenset(), False
        ref = self.ref
        out = (C.c_float * 9)()
        hits = []
        for e in self.entities:
            if ref.lib.oracle_kat_entity_hit(C.byref(ref.desc.entities[e]), ref.desc.triangles, ref.desc.triangleCount, self.o, self.d, self.time, float(tmin), float(tmax), out) == 1:
                t = np.float32(out[0])
                if t < INF:
                    hits.append((t, e))
        if not hits:
            return INF, frozenset(), False
        best = min(t for t, _ in hits)
        bits = best.view(np.uint32)
        return best, frozenset(e for t, e in hits if t.view(np.uint32) == bits), True


    def normal(self, entity, tmin, tmax):
        """HitRecord.Normal (world space) of Entity.Hit(ray, tMin, tMax) for one entity of the hit set, as three float32"""
        ref = self.ref
        out = (C.c_float * 9)()
        assert ref.lib.oracle_kat_entity_hit(C.byref(ref.desc.entities[entity]), ref.desc.triangles, ref.desc.triangleCount, self.o, self.d, self.time, float(tmin), float(tmax), out) == 1
        return np.asarray(out[4:7], np.float32)


def family_intervals(first, draws):
    """{family: (n, 2) float32} for n rays from their nearest distances under (0, +inf) and one draw each"""
    return {fam: np.asarray([family_interval(fam, d, u) for d, u in zip(first, draws)], np.float32).reshape(-1, 2) for fam in FAMILIES}


class IntervalReference:
    def __init__(self, oracle, desc):
        self.lib = oracle.load("strict")
        self.desc = desc
        self.osc = oracle.OracleScene(desc)
        n = desc.entityCount
        self.own_bounds = np.zeros((n, 6), np.float32)                                        # every entity's own box
        out = (C.c_float * 6)()
        for e in range(n):
            assert self.lib.oracle_kat_entity_bounds(C.byref(desc.entities[e]), desc.triangles, desc.triangleCount, out) == 0, e
            self.own_bounds[e] = out[:]
        self.bounds = np.zeros((n, 6), np.float32)                                            # the gate: the box of the reference leaf the entity sits in
        assert self.lib.oracle_kat_leaf_boxes(C.byref(desc), self.bounds.ctypes.data_as(C.POINTER(C.c_float))) == n
        if desc.maxBvhDepth in (0, 32):
            assert np.array_equal(self.bounds.view(np.uint32), self.own_bounds.view(np.uint32)), "a leaf forced at depth 32"
        self._lo, self._hi = self.bounds[:, :3].astype(np.float64), self.bounds[:, 3:].astype(np.float64)

    def close(self):
        self.osc.close()

    def _prefilter(self, origin, direction):
        """float64 slabs, every bound moved outwards by far more than binary32 rounding of the same expressions (2^-24 per operation): only over-includes"""
        o, d = np.asarray(origin, np.float64), np.asarray(direction, np.float64)
        keep = np.ones(len(self.bounds), bool)
        enter = np.zeros(len(self.bounds))
        leave = np.full(len(self.bounds), np.inf)
        for ax in range(3):
            lo, hi = self._lo[:, ax], self._hi[:, ax]
            scale = np.abs(lo) + np.abs(hi) + abs(o[ax]) + 1e-30
            if d[ax] == 0 or not np.isfinite(d[ax]) or not np.isfinite(o[ax]):
                if d[ax] == 0 and np.isfinite(o[ax]):
                    keep &= (o[ax] >= lo - 1e-5 * scale) & (o[ax] <= hi + 1e-5 * scale)       # (lo - o) * +-inf: passes only from inside the slab (or on its face: NaN)
                continue                                                                      # non-finite operands: the oracle decides
            inv = 1.0 / d[ax]
            t0, t1 = (lo - o[ax]) * inv, (hi - o[ax]) * inv
            pad = 1e-5 * (scale * abs(inv) + np.abs(t0) + np.abs(t1))
            enter = np.maximum(enter, np.minimum(t0, t1) - pad)
            leave = np.minimum(leave, np.maximum(t0, t1) + pad)
        keep &= ~(enter > leave)                                                              # NaN keeps
        return np.flatnonzero(keep)

    def ray(self, origin, direction, time=0.0):
        o, d = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_float * 3)(*[float(x) for x in direction])
        b = self.bounds
        passed = [int(e) for e in self._prefilter(origin, direction)
                  if self.lib.oracle_kat_aabb_hit(b[e, :3].ctypes.data_as(C.POINTER(C.c_float)), b[e, 3:].ctypes.data_as(C.POINTER(C.c_float)), o, d)]
        return RayCandidates(self, origin, direction, time, passed)

    def rays(self, pairs, times):
        """RayCandidates of every ray, and the self-check: with (0, +inf) the distance bits (and hit or miss) are OracleScene.hit_world's on every one of them."""
        out = []
        for (o, d), t in zip(pairs, times):
            rc = self.ray(o, d, t)
            dist, _, hit = rc.query(np.float32(0), INF)
            ref_hit, rec = self.osc.hit_world(o, d, t)
            assert hit == ref_hit, ("brute force and HitWorld disagree on hit or miss", o, d, t)
            if hit:
                assert dist.view(np.uint32) == np.float32(rec[0]).view(np.uint32), ("brute force and HitWorld disagree on the distance", o, d, t, dist, rec[0])
            rc.first = dist
            out.append(rc)
        return out
