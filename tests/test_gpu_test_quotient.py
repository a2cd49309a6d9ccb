"""The exact sphere test with the run's reciprocal (csrc/rtow_hit_tests.hip.h, sphere_hit_shared_rcp; TEST of the static- and the moving-sphere kernels) against the CPU
oracle, bit for bit, on scenes picked for the quotient.

Frames of 32 x 18 at 4 samples, seeds 1 .. 3, trace depth 8 and 16 (the 4- and 8-word kernels), through the plain launch, a chain of 3 and a group of 3 in both
contexts of tests/test_gpu_signed_walk.py (whose comparison helpers this reuses): colour, normal, albedo, weight and RayCount.  Each scene as it is (static spheres)
and with one sphere that moves (the moving-sphere kernels):
  inside   the camera inside a glass sphere: the first numerator of every camera ray is negative, the quotient is the second root's;
  shells   nested glass shells around a core: paths enter and leave sphere after sphere, both roots, origins on the surfaces;
  tangent  two internally tangent spheres and a ray through the point where they touch: both quotients are 3 / 1 exactly, the tie rule decides (t == best);
  ground   a radius-1000 ground with spheres of radius 0.01 resting on it, seen from 0.25 away;
  tiny     one sphere of radius 2^-66 at 3 x 2^-66: numerators below 2^-63, the range test fails and every quotient is the IEEE division.
The CPU test at the end shows with the oracle alone that each scene produces the case it is named for."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_signed_walk import KEYS, _download, _same, contexts  # noqa: F401

W, H, SPP = 32, 18, 4
TIE_PIXEL = (16, 9)
SCENES = ("inside", "shells", "tangent", "ground", "tiny")


def _grey(rt, s):
    return s.materials.append(rt.scenes.lambertian((0.6, 0.5, 0.4))) or len(s.materials) - 1


def build_scene(rt, name, moving):
    """(scene, make_params keywords, fix) - `fix(params)` adjusts the view where the scene needs one the look-at camera cannot give"""
    s = rt.scenes.Scene(name + ("_moving" if moving else ""))
    move = dict(moving=True, time_range=(0.0, 1.0)) if moving else {}
    kw, fix = {"focus": 1.0}, None
    if name == "inside":
        glass = s.materials.append(rt.scenes.dielectric(1.5)) or 0
        grey = _grey(rt, s)
        s.add_sphere((0.0, 0.0, 0.0), 2.0, glass)
        s.add_sphere((0.0, 0.0, -4.0), 1.0, grey)
        s.add_sphere((3.0, 0.5, -3.0), 0.7, rt.scenes.metal((0.8, 0.8, 0.8), 0.1), dest_offset=(0.0, 0.4, 0.0), **move)
        s.add_sphere((0.0, -1002.5, 0.0), 1000.0, grey)
        s.camera = {"position": [0.4, 0.3, 0.6], "target": [0.0, 0.0, -3.0], "up": [0.0, 1.0, 0.0], "vfov": 60.0, "aperture": 0.0}
    elif name == "shells":
        glass = s.materials.append(rt.scenes.dielectric(1.5)) or 0
        for radius in (1.0, 0.85, 0.6, 0.45):
            s.add_sphere((0.0, 0.0, -1.0), radius, glass)
        s.add_sphere((0.0, 0.0, -1.0), 0.2, rt.scenes.lambertian((0.8, 0.3, 0.3)), dest_offset=(0.1, 0.05, 0.0), **move)
        s.add_sphere((0.0, -101.0, -1.0), 100.0, _grey(rt, s))
        s.camera = {"position": [0.0, 0.3, 3.0], "target": [0.0, 0.0, -1.0], "up": [0.0, 1.0, 0.0], "vfov": 35.0, "aperture": 0.0}
    elif name == "tangent":
        # radius 2 about the origin and radius 1 about (0, 0, 1) touch at (0, 0, 2); from (0, 0, 5) straight down -z: b = -5, c = 21, sqrt(4), n0 = 3 and
        # b = -4, c = 15, sqrt(1), n0 = 3 - all exact.  No jitter, and the view's corner set so that the ray of TIE_PIXEL is (0, 0, -1) exactly (see fix)
        s.add_sphere((0.0, 0.0, 0.0), 2.0, rt.scenes.lambertian((0.2, 0.7, 0.3)))
        s.add_sphere((0.0, 0.0, 1.0), 1.0, rt.scenes.metal((0.9, 0.6, 0.2), 0.0))
        s.add_sphere((3.5, 0.0, 0.0), 1.0, rt.scenes.lambertian((0.3, 0.3, 0.8)), dest_offset=(0.0, 0.5, 0.0), **move)
        s.add_sphere((0.0, -102.0, 0.0), 100.0, _grey(rt, s))
        s.camera = {"position": [0.0, 0.0, 5.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 60.0, "aperture": 0.0}
        kw = {"focus": 1.0, "jitter": False}

        def fix(p):
            v = p.view
            assert v.horizontal.y == 0.0 and v.horizontal.z == 0.0 and v.vertical.x == 0.0 and v.vertical.z == 0.0 and v.lowerLeftCorner.z == -1.0
            u, w = pixel_centre(*TIE_PIXEL)
            v.lowerLeftCorner.x = -float(u * np.float32(v.horizontal.x))          # corner + u * horizontal + w * vertical: x and y cancel exactly, z is -1
            v.lowerLeftCorner.y = -float(w * np.float32(v.vertical.y))
    elif name == "ground":
        grey = _grey(rt, s)
        s.add_sphere((0.0, -1000.0, 0.0), 1000.0, grey)
        glass = s.materials.append(rt.scenes.dielectric(1.5)) or len(s.materials) - 1
        for i in range(25):
            x, z = 0.05 * (i % 5 - 2), 0.05 * (i // 5 - 2)
            y = float(np.sqrt(np.float64(1000.01) ** 2 - x * x - z * z) - 1000.0)      # resting on the ground: centres 1000.01 from the ground's centre
            s.add_sphere((x, y, z), 0.01, glass if i % 3 == 0 else grey, dest_offset=(0.0, 0.02, 0.0), **(move if i == 12 else {}))
        s.camera = {"position": [0.0, 0.05, 0.25], "target": [0.0, 0.01, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    else:
        unit = float(np.float32(2.0) ** -66)
        s.add_sphere((0.0, 0.0, -3.0 * unit), unit, rt.scenes.lambertian((0.7, 0.4, 0.2)), dest_offset=(0.25 * unit, 0.0, 0.0), **move)
        s.camera = {"position": [0.0, 0.0, 0.0], "target": [0.0, 0.0, -1.0], "up": [0.0, 1.0, 0.0], "vfov": 45.0, "aperture": 0.0}
    return s, kw, fix


def pixel_centre(cx, cy):
    """normalised coordinates of a pixel's centre, as the sample job forms them without jitter"""
    return (np.float32(cx) + np.float32(0.5)) / np.float32(W), (np.float32(cy) + np.float32(0.5)) / np.float32(H)


def make_params_list(rt, name, moving, depth):
    scene, kw, fix = build_scene(rt, name, moving)
    plist = [rt.scenes.make_params(scene, W, H, spp=SPP, trace_depth=depth, seed=seed, **kw) for seed in (1, 2, 3)]
    for p in plist:
        if fix:
            fix(p)
    return scene, plist


def _every_entry_point(rt, oracle, contexts, scene, plist, expect_image):  # noqa: F811
    """tests/test_gpu_signed_walk.py's _all_entry_points over a caller's parameter blocks: plain, chain of 3 and group of 3 in both contexts"""
    desc = scene.desc()
    n = W * H
    osc = oracle.OracleScene(desc)
    try:
        alone = [osc.sample_batch(p) for p in plist]
        chain = alone[0]
        for p in plist[1:]:
            chain = osc.sample_batch(p, {k: chain[k] for k, _ in KEYS})
    finally:
        osc.close()
    for name, ctx, log in contexts:
        del log[:]
        ctx.upload_scene(desc)
        said = [m for tag, m in log if tag == "scene"]
        assert len(said) == 1 and ("80-byte node image" in said[0]) == (name == "image80" and expect_image), (name, said)
        _same(rt.sample_batch_host(ctx, plist[0]), alone[0], (name, "plain"))
        bufs = [rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS]
        diags = [rt.DeviceBuffer(ctx, n * 4).zero() for _ in plist]
        rt.lib.check(rt.sample_batch_chain_device(ctx, plist, bufs, bufs, diags), "rtowSampleBatchChainDevice")
        ctx.synchronize()
        got = _download(bufs, n)
        got["diag"] = diags[2].download(np.float32, (n, 1))
        _same(got, chain, (name, "chain"))
        for b in bufs:
            b.zero()
        outs = [[rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS] for _ in plist]
        rt.lib.check(rt.sample_batch_group_device(ctx, plist, bufs, outs, diags), "rtowSampleBatchGroupDevice")
        ctx.synchronize()
        for k in range(3):
            got = _download(outs[k], n)
            got["diag"] = diags[k].download(np.float32, (n, 1))
            _same(got, alone[k], (name, "group", k))
        for b in bufs + diags + [x for o in outs for x in o]:
            b.free()
    return alone[0]


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
@pytest.mark.parametrize("name", SCENES)
def test_quotient_scenes_every_entry_point(rt, oracle, contexts, name, moving, depth):  # noqa: F811
    scene, plist = make_params_list(rt, name, moving, depth)
    ref = _every_entry_point(rt, oracle, contexts, scene, plist, expect_image=not moving)
    assert ref["diag"][:, 0].sum() >= W * H * SPP                 # every sample traced its camera ray
    if name in ("inside", "shells"):
        assert ref["diag"][:, 0].max() >= 4 * SPP, "input condition: paths go through the glass, sphere after sphere"


# ------------------------------------------------------------------------------------------------------------
# CPU: each scene produces the case it is named for - shown with the oracle alone
# ------------------------------------------------------------------------------------------------------------
def _camera_rays(oracle, p):
    """the oracle's camera ray (View.GetRay) through every pixel centre: origins (n, 3), directions (n, 3)"""
    lib = oracle.load("strict")
    rays = np.zeros((W * H, 8), np.float32)
    for cy in range(H):
        for cx in range(W):
            u, w = pixel_centre(cx, cy)
            state, out = C.c_uint32(1), (C.c_float * 8)()
            lib.oracle_kat_get_ray(C.byref(p.view), float(u), float(w), C.byref(state), out)
            rays[cy * W + cx] = list(out)
    return rays[:, 0:3], rays[:, 3:6]


def _entity_distance(rt, oracle, scene, index, origin, direction):
    """HitTests.Hit of one sphere of the scene by itself (tMin 0, tMax inf): (hit, distance)"""
    desc = scene.desc()
    out = (C.c_float * 9)()
    hit = oracle.load("strict").oracle_kat_entity_hit(C.byref(desc.entities[index]), None, 0, (C.c_float * 3)(*origin), (C.c_float * 3)(*direction), 0.0, 0.0, float("inf"), out)
    return hit == 1, np.float32(out[0])


@pytest.mark.parametrize("moving", [False, True], ids=["static", "moving"])
@pytest.mark.parametrize("name", SCENES)
def test_each_scene_produces_its_case(rt, oracle, name, moving):
    scene, plist = make_params_list(rt, name, moving, 8)
    p = plist[0]
    origins, dirs = _camera_rays(oracle, p)
    osc = oracle.OracleScene(scene.desc())
    try:
        found = [osc.nearest_hit(o, d, 0.0) for o, d in zip(origins, dirs)]
        _, counters = osc.sample_batch(p, want_counters=True)
    finally:
        osc.close()
    count = np.array([n for n, _ in found])
    dist = np.array([r[0] for _, r in found], np.float32)
    entity = np.array([int(r[7]) for _, r in found])
    print(name, moving, "rays", counters.rays, "candidates", counters.candidates, "hits", counters.hits, "max hits of a ray", counters.maxHits)
    assert counters.hits > 0 and counters.rays >= W * H * SPP
    if name == "inside":
        # the origin is inside the glass sphere (entity 0), so its first root lies behind every ray; the oracle's nearest hit of EVERY camera ray is that sphere
        # all the same: the second root
        assert np.linalg.norm(origins[0].astype(np.float64)) < 2.0 and np.all(origins == origins[0])
        assert np.all(count >= 1) and np.all(entity == 0) and np.all(dist > 0)
        assert counters.rays > 2 * W * H * SPP                       # and the paths go on from there
    elif name == "shells":
        # the ray through the shells' centre meets all four of them, and the core when it stands still; a ray finds at most one hit per sphere
        centre = int(np.argmax(count))
        assert count[centre] >= 4, count[centre]
        assert counters.maxHits >= 4
    elif name == "tangent":
        k = TIE_PIXEL[1] * W + TIE_PIXEL[0]
        assert dirs[k].tolist() == [0.0, 0.0, -1.0] and origins[k].tolist() == [0.0, 0.0, 5.0], (origins[k], dirs[k])
        hit0, t0 = _entity_distance(rt, oracle, scene, 0, origins[k], dirs[k])
        hit1, t1 = _entity_distance(rt, oracle, scene, 1, origins[k], dirs[k])
        assert hit0 and hit1 and t0 == np.float32(3.0) and t0.view(np.uint32) == t1.view(np.uint32), (t0, t1)
        assert count[k] == 2 and dist[k] == np.float32(3.0)            # both in the ray's hit list, at the nearest distance: t == best
    elif name == "ground":
        # most rays end on the ground (entity 0) a few tenths away, some on a sphere of radius 0.01
        assert np.any(entity[count > 0] == 0) and np.any(entity[count > 0] > 0)
        assert float(dist[count > 0].max()) < 100.0
    else:
        # camera rays have unit length (a = 1 within a few ulp), so t = n / a below 2^-64 means a numerator below 2^-63: outside the quotient's fast range
        hits = count > 0
        assert hits.sum() > W * H // 8
        assert np.all(dist[hits] > 0) and np.all(dist[hits] < np.float32(2.0) ** -64)
        a = np.sum(dirs.astype(np.float64) ** 2, axis=1)
        assert np.all(np.abs(a - 1.0) < 1e-6)
