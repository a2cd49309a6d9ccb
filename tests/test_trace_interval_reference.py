"""CPU: tests/trace_interval_reference.py - the brute-force reference of the interval ray queries - against the oracle itself: with (0, +inf) its distance bits are
Raytracer.HitWorld's on every test ray of every scene the GPU test uses (the module's own self-check), and the per-type boundary rules that include/rtow.h states - what
happens when tMin or tMax is exactly a hit distance or one of its two float neighbours - are what the oracle's Entity.Hit does: the expected values are the oracle's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_trace_rays as tr  # noqa: E402  (its ray generators)
import trace_interval_reference as ir  # noqa: E402

SCENES = ["cover", "moving", "mixed", "volumes", "mesh", "textured", "twins", "tiny", "coplanar"]
INF = ir.INF


@pytest.mark.parametrize("name", SCENES)
def test_with_no_bounds_the_brute_force_is_hit_world(rt, oracle, name):
    scene = tr._scene(rt, name)
    ref = ir.IntervalReference(oracle, scene.desc())
    pairs, times = ir.interval_rays(tr, rt, scene, name)
    if name != "mesh":
        pairs, times = pairs[::4] + pairs[-360:], times[::4] + times[-360:]          # a quarter of the generated rays, every axis ray
    try:
        cands = ref.rays(pairs, times)                                               # asserts hit or miss and the distance bits of every ray
    finally:
        ref.close()
    hits = sum(np.isfinite(rc.first) for rc in cands)
    assert len(cands) == len(pairs) and 0 < hits < len(cands), (name, hits)


def _one(rt, kind):
    S = rt.scenes
    s = S.Scene("one " + kind)
    m = S.lambertian((0.5, 0.5, 0.5))
    if kind == "sphere":
        s.add_sphere((0.1, -0.2, 0.3), 1.25, m)
    elif kind == "rect":
        s.add_rect((0.1, -0.2, 0.3), (3, 3), m)
    elif kind == "box":
        s.add_box((0.1, -0.2, 0.3), (1.5, 2.0, 2.5), m)
    else:
        s.add_triangle((-2, -2, 0.3), (2, -2, 0.3), (0, 2, 0.1), m)
    s.camera = {"position": [0.3, 0.4, 5.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    return s


@pytest.mark.parametrize("kind", ["sphere", "rect", "box", "triangle"])
def test_bounds_at_the_hit_distance_and_its_float_neighbours(rt, oracle, kind):
    scene = _one(rt, kind)
    desc = scene.desc()
    ref = ir.IntervalReference(oracle, desc)
    o = np.asarray([0.3, 0.4, 5.0], np.float32)
    d = np.asarray([-0.05, -0.11, -0.93], np.float32)                                # not normalised: distances are in units of it
    lib = oracle.load("strict")

    def entity_hit(tmin, tmax):
        out = (C.c_float * 9)()
        hit = lib.oracle_kat_entity_hit(C.byref(desc.entities[0]), desc.triangles, desc.triangleCount, (C.c_float * 3)(*o), (C.c_float * 3)(*d), 0.0, float(tmin), float(tmax), out)
        return hit == 1, np.float32(out[0])

    try:
        rc = ref.rays([(o, d)], [0.0])[0]
        t = rc.first
        assert np.isfinite(t) and t > 0, kind
        seen = {}
        for what, (tmin, tmax) in {"tmin-": (ir.down(t), INF), "tmin=": (t, INF), "tmin+": (ir.up(t), INF),
                                   "tmax-": (0, ir.down(t)), "tmax=": (0, t), "tmax+": (0, ir.up(t))}.items():
            want_hit, want_t = entity_hit(tmin, tmax)                                # the oracle's Entity.Hit is the expectation
            got_t, got_set, got_any = rc.query(np.float32(tmin), np.float32(tmax))
            assert got_any == want_hit and got_set == (frozenset([0]) if want_hit else frozenset()), (kind, what)
            assert got_t.view(np.uint32) == (want_t if want_hit else INF).view(np.uint32), (kind, what, got_t, want_t)
            seen[what] = (want_hit, want_t)
    finally:
        ref.close()
    print(kind, float(t), {k: (h, float(v)) for k, v in ((k, v[1]) for k, v in seen.items()) for h in [seen[k][0]]})
    same = lambda k: seen[k][0] and seen[k][1].view(np.uint32) == t.view(np.uint32)
    # include/rtow.h, "hit set" and "peeling", as statements about the oracle
    assert same("tmin-") and same("tmax+"), kind                                     # the interval that holds the distance strictly inside: every type
    assert not same("tmin+"), kind                                                   # the next float above excludes that hit for every type (what a peeling host passes)
    if kind == "sphere":
        assert not same("tmin=") and not same("tmax="), kind                         # both ends strict
        assert seen["tmin="][0] and seen["tmin="][1] > t                             # ... and the far root answers instead
        assert not seen["tmax="][0] and not seen["tmax-"][0]                         # a near root beyond tMax: the far root fails too
    else:
        assert same("tmax="), kind                                                   # rejected iff t > tMax
        assert not seen["tmax-"][0], kind
        if kind in ("rect", "triangle"):
            assert same("tmin="), kind                                               # rejected iff t < tMin: a hit at exactly tMin stays
            assert not seen["tmin+"][0], kind                                        # one-sided: nothing behind it
