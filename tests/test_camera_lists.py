"""CPU: what primary_candidates_kernel leaves off a pixel's camera-ray list (csrc/rtow_camera_lists.hip.h) held to its contract without a GPU.

A host shim (tests/native/camera_lists_shim.cpp) restates the kernel's beam and walk around the header's functions.  Soundness: for every pixel of the cover scene at
64 x 36, a strided set of its pixels at the 1920 x 1080 pixel size, and the small scenes of tests/camera_lists_support.py, camera rays drawn the way REGEN forms them
(corners of the pixel and the rim of the lens first) never have a dropped primitive as their nearest hit - by the oracle's HitWorld and by sphere_hit over all spheres -
and a primitive dropped as unreachable is not reported by sphere_hit at all.  Each scene must show the rule, or the "never drop" clause, it was picked for.
Margins: constructions on the unsafe side of each allowance, where the verdict must be "stays".  Degenerate inputs: nothing is dropped.
"""
import ctypes as C
import math

import numpy as np
import pytest

import camera_lists_support as S

U = 2.0 ** -24


def _check_pixels(oracle, name, w, h, pixels, rays_per_pixel, jitter=True, times=(0.0,)):
    sc = S.scene(name)
    cs = S.Compiled(sc)
    p = S.params(sc, jitter=jitter, w=w, h=h, name=name)
    osc = oracle.OracleScene(sc.desc())
    seen = {v: 0 for v in range(5)}
    covered = shorter = 0
    try:
        for cx, cy in pixels:
            listed, leaves, info = cs.pixel(p, cx, cy)
            full, _, _ = cs.pixel(p, cx, cy, prune=False)
            if listed is None:
                assert full is None
                continue
            assert [n for n in full if n in listed] == listed, "the remaining nodes keep their order"
            shorter += len(listed) < len(full)
            covered += info["covered"]
            for _, v in leaves:
                seen[v] += 1
            dropped = sorted({prim for prim, v in leaves if v in (S.UNREACHABLE, S.HIDDEN)})
            if not dropped:
                continue
            unreachable = [prim for prim, v in leaves if v == S.UNREACHABLE][:64]
            rays, nearest, hit = cs.rays(p, cx, cy, rays_per_pixel, 1, unreachable)
            assert not np.isin(nearest, dropped).any(), (name, cx, cy, "sphere_hit's nearest hit is a dropped primitive")
            assert not hit.any(), (name, cx, cy, "a primitive dropped as unreachable is reported as hit")
            for r in rays:
                for t in times:
                    got, o = osc.hit_world(r[0:3], r[3:6], t)
                    assert not (got and int(o[7]) in dropped), (name, cx, cy, int(o[7]), "the oracle's nearest hit is a dropped primitive")
    finally:
        osc.close()
    return seen, covered, shorter


def test_cover_scene_small_frame(oracle):
    seen, covered, shorter = _check_pixels(oracle, "cover", 64, 36, [(x, y) for y in range(36) for x in range(64)], 8)
    print("cover 64x36: verdicts", seen, "covered pixels", covered, "shorter lists", shorter)
    assert seen[S.UNREACHABLE] > 0 and seen[S.HIDDEN] > 0 and covered > 0 and shorter > 0


def test_cover_scene_full_size_pixels(oracle):
    seen, covered, shorter = _check_pixels(oracle, "cover", 1920, 1080, [(x, y) for y in range(7, 1080, 24) for x in range(5, 1920, 24)], 6)
    print("cover 1920x1080 strided: verdicts", seen, "covered pixels", covered, "shorter lists", shorter)
    assert seen[S.UNREACHABLE] > 0 and seen[S.HIDDEN] > 0 and shorter > 0


@pytest.mark.parametrize("name", S.SMALL_SCENES + ("moving",))
def test_small_scenes(oracle, name):
    jitter = name != "tangent"
    times = (0.0, 0.37, 1.0) if name == "moving" else (0.0,)
    seen, covered, shorter = _check_pixels(oracle, name, S.W, S.H, [(x, y) for y in range(S.H) for x in range(S.W)], 24 if name == "lens" else 12, jitter, times)
    print(name, "verdicts", seen, "covered pixels", covered, "shorter lists", shorter)
    sc = S.scene(name)
    cs = S.Compiled(sc)
    p = S.params(sc, jitter=jitter, name=name)
    if name == "one":
        assert seen[S.UNREACHABLE] > 0 and seen[S.STAYS] > 0 and seen[S.HIDDEN] == 0
    elif name == "stack":
        assert seen[S.HIDDEN] > 0
        for cx, cy in ((15, 8), (16, 9)):                      # centre pixels: the front sphere alone is left
            listed, leaves, _ = cs.pixel(p, cx, cy)
            assert len(listed) == 1 and sum(v == S.STAYS for _, v in leaves) == 1, (listed, leaves)
        # silhouette pixels (the front sphere's rim crosses them: it cannot cover) hide nothing and keep the front sphere's node
        rim = [(listed, leaves) for listed, leaves, info in (cs.pixel(p, cx, 9) for cx in range(S.W)) if not info["covered"] and dict(leaves).get(0) == S.STAYS]
        assert len(rim) >= 2 and all(len(listed) == 1 and S.HIDDEN not in [v for _, v in leaves] for listed, leaves in rim)
    elif name == "cluster":
        assert seen[S.HIDDEN] == 0 and covered == 0, "nothing covers a pixel"
        entries, no_list = S.list_lengths(cs, p, True)
        assert sum(entries[5:9]) > 0 and no_list > 0, "lists of 5 to 8 nodes survive, longer ones still fall back to the walk"
    elif name == "inside_glass":
        assert seen[S.HOLDS_ORIGIN] == S.W * S.H, "the sphere around the camera is in every beam and never dropped"
        assert seen[S.HIDDEN] > 0
    elif name == "tangent":
        _, leaves, info = cs.pixel(p, 16, 9)
        assert info["covered"] and dict(leaves)[0] == S.STAYS and dict(leaves)[1] == S.STAYS, "the tied partner stays"
    elif name == "horizon":
        ground = [dict(cs.pixel(p, cx, cy)[1]).get(0) for cy in (0, S.H - 1) for cx in range(S.W)]
        assert ground.count(S.UNREACHABLE) == S.W and ground.count(S.STAYS) == S.W, "the ground is dropped under the sky rows and kept in the bottom row"
        assert seen[S.STAYS] > S.W * S.H // 2
    elif name == "lens":
        assert p.view.lensRadius > 0 and seen[S.UNREACHABLE] > 0 and seen[S.HIDDEN] > 0
    elif name == "moving":
        assert seen[S.MOVING] > 0 and seen[S.UNREACHABLE] > 0


# ------------------------------------------------------------------ margins ------------------------------------------------------------------
DIR = np.array([0.36, 0.48, 0.8])                    # a unit direction without a zero component
SIDE = np.array([0.8, -0.6, 0.0])                    # perpendicular to it
SPREAD, GMIN = 2e-6, 1.0                              # the least spread the kernel ever has, no lens


def _beam(o=(0.0, 0.0, 0.0), d=DIR, R=0.0, spread=SPREAD, gmin=GMIN, ok=1):
    d32 = np.asarray(d, np.float32)
    return [float(x) for x in np.asarray(o, np.float32)] + [float(x) for x in d32] + [R, spread, gmin, ok]


def _seen(X, rho):
    E = 2.0 ** -19 * (X * X + rho * rho)
    return math.sqrt(rho * rho + E), E


@pytest.mark.parametrize("X", [1.0, 30.0, 1000.0])
@pytest.mark.parametrize("rho", [0.01, 0.2, 1000.0])
def test_grazing_rays_inside_the_allowance_keep_the_sphere(X, rho):
    lib = S.shim()
    seen, E = _seen(X, rho)
    # the centre at distance X from the origin, the centre ray passing it at miss distance m: inside what sphere_hit may see (the stated allowance), the sphere stays
    for m in (seen * (1.0 - 1e-9), rho, 0.5 * (rho + seen)):
        if m >= X:
            continue
        c = DIR * math.sqrt(X * X - m * m) + SIDE * m
        assert lib.cl_unreachable(*_beam(), float(c[0]), float(c[1]), float(c[2]), rho) == 0, (X, rho, m)
        assert lib.cl_unreachable(*_beam(), float(c[0]), float(c[1]), float(c[2]), -rho) == 0, "negative radii enter as |r|"
    if rho >= X:                                                   # the origin inside the sphere: never dropped, whatever the direction
        for c in (DIR * X, -DIR * X, SIDE * X):
            assert lib.cl_unreachable(*_beam(), float(c[0]), float(c[1]), float(c[2]), rho) == 0
        return
    # and the rule is alive: well outside it goes
    m = 2.0 * seen + 0.01 * X
    if m < X:
        c = DIR * math.sqrt(X * X - m * m) + SIDE * m
        assert lib.cl_unreachable(*_beam(), float(c[0]), float(c[1]), float(c[2]), rho) == 1, (X, rho, m)
    # the allowance covers what sphere_hit really reports: rays that pass outside the sphere and are reported all the same lie inside rhoSeen
    rng = np.random.default_rng(int(X * 7 + rho * 1000))
    worst = 0.0
    ro = np.zeros(3, np.float32)
    t = C.c_float()
    for _ in range(4000):
        a = rng.normal(size=3); a /= np.linalg.norm(a)
        b = np.cross(a, rng.normal(size=3)); b /= np.linalg.norm(b)
        m = rho + (seen - rho) * rng.uniform(0.0, 1.2) if seen - rho > 1e-7 * rho else rho * (1.0 + rng.uniform(0.0, 4e-7))
        c = (a * math.sqrt(X * X - m * m) + b * m).astype(np.float32)
        rd = a.astype(np.float32)
        rd = (rd * np.float32(1.0 / np.sqrt(np.dot(rd, rd), dtype=np.float32))).astype(np.float32)
        if lib.cl_sphere_hit(ro.ctypes.data, rd.ctypes.data, c.ctypes.data, rho, C.addressof(t)):
            c64, d64 = c.astype(np.float64), rd.astype(np.float64)
            true_m = np.linalg.norm(c64 - d64 * np.dot(c64, d64) / np.dot(d64, d64))
            worst = max(worst, true_m / seen)
            assert lib.cl_unreachable(*_beam(d=rd), float(c[0]), float(c[1]), float(c[2]), rho) == 0, "a sphere sphere_hit reports on the centre ray itself stays"
    print("X %g rho %g: rhoSeen %.6g, largest reported miss distance / rhoSeen %.4f" % (X, rho, seen, worst))
    assert worst <= 1.0


def test_a_sphere_the_centre_ray_just_fails_to_pass_inside_does_not_cover():
    lib = S.shim()
    tA = C.c_double()
    X, rho = 5.0, 1.0
    seen, E = _seen(X, rho)
    inner = math.sqrt(rho * rho - E)                                # what sphere_hit is certain to see
    width = (X * SPREAD) * 1.01 + 1e-5 * (1.0 + X)
    for m, covers in ((inner - width, 0), (inner - 0.5 * width, 0), (inner, 0), (rho, 0), (0.5 * rho, 1), (0.0, 1)):
        c = DIR * math.sqrt(X * X - m * m) + SIDE * m
        assert lib.cl_covers(*_beam(), float(c[0]), float(c[1]), float(c[2]), rho, C.byref(tA)) == covers, m
    # never: behind the origin, around the origin, too close to leave the reference's 0.001 room, a lens as wide as the gap
    for c, r in ((-DIR * 5.0, 1.0), (DIR * 0.5, 1.0), (DIR * 1.0005, 1.0)):
        assert lib.cl_covers(*_beam(), float(c[0]), float(c[1]), float(c[2]), r, C.byref(tA)) == 0
    c = DIR * 5.0
    assert lib.cl_covers(*_beam(R=0.2, gmin=1.0), float(c[0]), float(c[1]), float(c[2]), 1.0, C.byref(tA)) == 1
    assert lib.cl_covers(*_beam(R=0.2, gmin=1.0), float(c[0]), float(c[1]), float(c[2]), 0.2, C.byref(tA)) == 0      # the lens is as wide as the sphere


def test_a_sphere_entered_exactly_at_tA_stays():
    lib = S.shim()
    tA = C.c_double()
    cA = DIR * 5.0
    assert lib.cl_covers(*_beam(), float(cA[0]), float(cA[1]), float(cA[2]), 1.0, C.byref(tA)) == 1
    assert 5.0 < tA.value < 5.001, "closest approach plus the beam's spread there plus a relative allowance"
    rho = 0.5
    for entry, hidden in ((tA.value, 0), (tA.value * (1.0 + 2.0 ** -19) + 1e-6, 0), (tA.value - 0.3, 0), (4.0, 0), (tA.value + 0.5 + 0.01, 1), (tA.value + 3.0, 1)):
        # the TRUE sphere B is entered by the centre ray at `entry` (the grown one earlier): anything up to tA with its margin stays
        cB = (DIR * (entry + rho)).astype(np.float32)
        assert lib.cl_hidden(*_beam(), float(cB[0]), float(cB[1]), float(cB[2]), rho, tA.value) == hidden, entry
    # a sphere around the origin, or off to the side of the beam behind the coverer
    assert lib.cl_hidden(*_beam(), 0.1, 0.0, 0.0, 0.5, tA.value) == 0
    cB = DIR * 9.0 + SIDE * 3.0
    assert lib.cl_hidden(*_beam(), float(cB[0]), float(cB[1]), float(cB[2]), 0.5, tA.value) == 1
    assert lib.cl_hidden(*_beam(), float(cB[0]), float(cB[1]), float(cB[2]), 0.5, float("nan")) == 0
    assert lib.cl_hidden(*_beam(), float(cB[0]), float(cB[1]), float(cB[2]), 0.5, float("inf")) == 0


def test_degenerate_inputs_drop_nothing():
    lib = S.shim()
    tA = C.c_double()
    far = DIR * 9.0 + SIDE * 3.0                       # dropped by both rules in a sound pixel
    args = (float(far[0]), float(far[1]), float(far[2]), 0.5)
    assert lib.cl_unreachable(*_beam(), *args) == 1 and lib.cl_hidden(*_beam(), *args, 5.0) == 1 and lib.cl_beam_prunable(*_beam()) == 1
    nan, inf = float("nan"), float("inf")
    bad = [_beam(d=(0.0, 0.6, 0.8)), _beam(d=(0.6, 0.0, 0.8)), _beam(d=(0.6, 0.8, 0.0)),        # a zero direction component
           _beam(R=0.25, gmin=1.0), _beam(R=0.3, gmin=1.0),                                        # R >= gmin / 4
           _beam(ok=0), _beam(spread=nan), _beam(spread=inf), _beam(R=nan), _beam(gmin=nan), _beam(o=(nan, 0.0, 0.0)), _beam(o=(inf, 0.0, 0.0)),
           _beam(d=(nan, 0.48, 0.8)), _beam(d=(3.6, 4.8, 8.0)), _beam(R=-0.1), _beam(spread=-1e-3)]
    front = DIR * 5.0
    for b in bad:
        assert lib.cl_beam_prunable(*b) == 0, b
        assert lib.cl_unreachable(*b, *args) == 0 and lib.cl_hidden(*b, *args, 5.0) == 0, b
        assert lib.cl_covers(*b, float(front[0]), float(front[1]), float(front[2]), 1.0, C.byref(tA)) == 0, b
    for c in ((far[0], far[1], far[2], nan), (nan, far[1], far[2], 0.5), (far[0], inf, far[2], 0.5), (far[0], far[1], far[2], inf)):      # a NaN radius, a centre that is not finite
        c = [float(x) for x in c]
        assert lib.cl_unreachable(*_beam(), *c) == 0 and lib.cl_hidden(*_beam(), *c, 5.0) == 0
        assert lib.cl_covers(*_beam(), float(front[0]), float(front[1]), float(front[2]), c[3], C.byref(tA)) == (1 if c[3] == 0.5 else 0)
