"""Shared inputs of tests/test_query_edges_host.py (CPU: the host walk), tests/test_gpu_query_edges.py (the six ray queries on the device) and
tests/test_gpu_time_ranges.py (the moving-sphere sample kernels): the scenes, rays and ray times on which the queries ship code that the hand-built scenes of
tests/test_gpu_trace_rays.py never run, and the brute-force answers (tests/trace_interval_reference.py, oracle calls only), computed once per case and shared.

 * leaves forced at MaxBvhDepth: random scenes (tests/test_gpu_fuzz.py's generator, imported) at max_bvh_depth 32, 3 and 1, and `plane_scene` - axis-aligned entities at
   dyadic coordinates with rays lying exactly IN the planes of the entities' own boxes, which pass the union box of a forced leaf and not the own box;
 * SCENE_KIND_SPHERES_MOTION with one shared TimeRange other than (0, 1) (the hoisted clamp with commonT0 != 0, commonT1 != 1) and with mixed ranges, one of them
   reversed (commonTimeRange == 0: the clamp per sphere test); a general scene with the same ranges on a rect, a rotated box, a triangle and a sphere;
 * ray times below, at, inside, above the ranges, NaN, +inf and -inf;
 * one-entity scenes (the walk's root with one child).
A plain module, imported like trace_interval_reference.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_fuzz as fz  # noqa: E402  (its random-scene generator)
import test_gpu_trace_rays as tr  # noqa: E402  (its ray generators)
import trace_interval_reference as ir  # noqa: E402

NAN, INF = float("nan"), float("inf")
TIMES = (-0.5, 0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0, 1.5, NAN, INF, -INF)      # ray k of a time-range or one-entity scene gets TIMES[k % 12]
FUZZ_TIMES = (0.0, 0.3, 1.2, -0.2)                                               # random scenes (their movers have TimeRange (0, 1))
RANGES = ((0.25, 0.75), (0.9, 0.2), (-1.0, 3.0), (0.0, 1.0))                     # the second is reversed: t1 < t0
TWIN_TIMES = (0.1, 0.5, 0.9)                                                     # (0.25, 0.75) and (0.4, 0.6) clamp to the same end at 0.1 and 0.9, not at 0.5
FUZZ_SEEDS = tuple(range(12))
FUZZ_DEPTHS = (32, 3, 1)


def time_range_scene(rt, common, unit_ranges=False):
    """Sphere-only moving scene: a ground sphere, a 7 x 5 grid of radius-0.4 spheres of which two in three move, and two pairs of coincident twins (equal position and
    destinationOffset).  common: every TimeRange is (0.25, 0.75) - the scene compiler hoists the clamp; otherwise the ranges cycle through RANGES, one twin pair has
    identical ranges and the other (0.25, 0.75) and (0.4, 0.6): those two coincide bit for bit exactly when the ray time clamps both to the same end.
    unit_ranges: the same scene with every range (0, 1) (what the suite's other moving scenes have), for the input conditions."""
    S = rt.scenes
    s = S.Scene("time_ranges_%s" % ("common" if common else "mixed"))
    s.add_sphere((0, -100.5, 0), 100, S.lambertian((0.6, 0.6, 0.6)))
    mats = [S.lambertian((0.8, 0.2, 0.2)), S.metal((0.9, 0.9, 0.9), 0.0), S.dielectric(1.5), S.lambertian((0.1, 0.7, 0.2)), S.metal((0.8, 0.6, 0.2), 0.4),
            S.standard((0.1, 0.1, 0.1), 0.0, 0.0, emission=(2.0, 1.5, 1.0))]

    def rng_of(r):
        return (0.0, 1.0) if unit_ranges else r

    k = moved = 0
    for gx in range(-3, 4):
        for gz in range(-2, 3):
            mv = {}
            if k % 3:
                mv = dict(moving=True, dest_offset=(0.3 * (k % 3 - 1.5), 0.6, 0.2), time_range=rng_of(RANGES[0] if common else RANGES[moved % 4]))
                moved += 1
            s.add_sphere((gx * 1.1, 0.05 * (k % 4), gz * 1.1), 0.4, mats[k % len(mats)], **mv)
            k += 1
    twins = {}
    # the second pair flies through the frame from far outside it: at ray time 0.5 its members' clamped fractions are 0.5 and 0.49999993 ((0.5 - 0.4f) / (0.6f - 0.4f)),
    # and only a way of 128 units puts their centres 1e-5 apart there - enough to show in a hit distance of about 7 (ulp 5e-7), which a shorter way's difference is not
    for name, pos, dest, ranges in (("same", (-2.0, 1.75, 0.5), (0.3, 0.3, 0.1), (RANGES[0], RANGES[0])),
                                    ("different", (-64.0, 2.0, 0.0), (128.0, 0.0, 0.0), (RANGES[0], RANGES[0] if common else (0.4, 0.6)))):
        twins[name] = (s.entity_count, s.entity_count + 1)
        for c, r in enumerate(ranges):
            s.add_sphere(pos, 0.4, mats[c], moving=True, dest_offset=dest, time_range=rng_of(r))
    s.twins = twins
    s.camera = {"position": [0.5, 3.0, 7.0], "target": [0.0, 0.4, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    return s


TWIN_RAYS = 40


def twin_rays(scene):
    """TWIN_RAYS triples of rays from the camera at the different-range twin pair, ray 3 * j + i at ray time TWIN_TIMES[i] and aimed (with a spread of a third of the
    radius) at where the pair is at that time - the start, the middle and the end of its way: (pairs, times)"""
    rng = np.random.default_rng(17)
    cam = np.asarray(scene.camera["position"], np.float32)
    e = scene.twins["different"][0]
    pairs, times = [], []
    for _ in range(TWIN_RAYS):
        for t, f in zip(TWIN_TIMES, (0.0, 0.5, 1.0)):
            at = np.asarray(scene.positions[e], np.float64) + f * np.asarray(scene.dest_offsets[e], np.float64)
            pairs.append((cam, (at + rng.normal(size=3) * 0.12 - cam).astype(np.float32)))
            times.append(t)
    return pairs, times


def general_time_range_scene(rt, unit_ranges=False):
    """A moving rect, a moving rotated box, a moving triangle and a moving sphere with the four RANGES, and a static rect (the floor): SCENE_KIND_GENERAL"""
    S = rt.scenes
    s = S.Scene("time_ranges_general")
    r = [(0.0, 1.0)] * 4 if unit_ranges else RANGES
    s.add_rect((0, -1, 0), (10, 10), S.lambertian((0.6, 0.6, 0.6)), rotation=S.quat_axis_angle((1, 0, 0), -90))
    s.add_rect((-1.6, 0.1, -0.5), (1.8, 1.8), S.metal((0.9, 0.9, 0.9), 0.0), moving=True, dest_offset=(0.5, 0.7, 0.0), time_range=r[0])
    s.add_box((0.1, -0.3, 0.2), (1.1, 1.3, 1.1), S.lambertian((0.8, 0.3, 0.2)), rotation=S.quat_axis_angle((0, 1, 0), 25), moving=True, dest_offset=(0.4, 0.6, 0.3), time_range=r[1])
    s.add_triangle((-1.2, -1.0, 1.2), (-0.4, 0.6, 1.0), (0.4, -1.0, 1.4), S.lambertian((0.2, 0.3, 0.8)), moving=True, dest_offset=(0.0, 0.8, 0.4), time_range=r[2])
    s.add_sphere((1.8, -0.3, 0.3), 0.7, S.dielectric(1.5), moving=True, dest_offset=(-0.3, 0.7, 0.0), time_range=r[3])
    s.camera = {"position": [0.0, 1.0, 6.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    return s


ONE_ENTITY = ("sphere", "moving_sphere", "box", "triangle")


def one_entity_scene(rt, which):
    S = rt.scenes
    s = S.Scene("one_" + which)
    m = S.lambertian((0.7, 0.4, 0.3))
    if which == "sphere":
        s.add_sphere((0.2, 0.1, -0.3), 0.8, m)
    elif which == "moving_sphere":
        s.add_sphere((0.2, 0.1, -0.3), 0.8, m, moving=True, dest_offset=(0.5, 0.7, 0.2), time_range=RANGES[0])
    elif which == "box":
        s.add_box((0.1, -0.2, 0.0), (1.2, 0.9, 1.4), m, rotation=S.quat_axis_angle((1, 2, 0.5), 37))
    else:
        s.add_triangle((-1.0, -0.8, 0.2), (0.1, 1.1, -0.3), (1.2, -0.6, 0.4), m)
    s.camera = {"position": [0.5, 1.0, 5.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    return s


def plane_scene(rt):
    """Unrotated rects, boxes, a triangle and a sphere at dyadic coordinates (two boxes share a face, a rect lies in a face of one of them), so that a ray along an axis
    from a dyadic origin meets their surfaces, edges and box planes exactly."""
    S = rt.scenes
    s = S.Scene("planes")
    m = S.lambertian((0.7, 0.7, 0.7))
    s.add_rect((0.0, 0.0, -1.0), (2.0, 2.0), m)
    s.add_rect((-1.0, 0.0, 1.0), (1.0, 2.0), m)                                # in the z = 1 face of the two boxes below
    s.add_box((-1.5, 0.0, 0.5), (1.0, 1.0, 1.0), m)
    s.add_box((-0.5, 0.0, 0.5), (1.0, 1.0, 1.0), m)
    s.add_triangle((0.5, -1.0, 0.5), (1.5, -1.0, 0.5), (0.5, 1.0, 1.5), m)
    s.add_sphere((1.5, 0.5, -0.25), 0.5, m)
    s.camera = {"position": [0.0, 0.5, 6.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    return s


def plane_rays(own_boxes):
    """For every entity, every plane of its own box ((n, 6) float32: min.xyz, max.xyz) and both in-plane axes: rays that lie exactly in the plane (origin on it, that
    direction component exactly 0), run along one in-plane axis in both senses from two units outside the box, and pass through 0, 1/4, 1/2 and 1 of the box's extent
    on the other in-plane axis.  96 rays per entity."""
    pairs = []
    for b in np.asarray(own_boxes, np.float32):
        lo, hi = b[:3], b[3:]
        for axis in range(3):
            for plane in (lo[axis], hi[axis]):
                for run in range(3):
                    if run == axis:
                        continue
                    other = 3 - axis - run
                    for frac in (0.0, 0.25, 0.5, 1.0):
                        for sense in (1.0, -1.0):
                            o = np.zeros(3, np.float32)
                            d = np.zeros(3, np.float32)
                            o[axis] = plane
                            o[other] = np.float32(lo[other] + np.float32(frac) * np.float32(hi[other] - lo[other]))
                            o[run] = np.float32(lo[run] - 2.0) if sense > 0 else np.float32(hi[run] + 2.0)
                            d[run] = sense
                            pairs.append((o, d))
    return pairs


class Case:
    """One scene at one max_bvh_depth with its rays and ray times.  kind: "ranges" (the two sphere-only time-range scenes), "general", "one", "planes", "fuzz"."""

    def __init__(self, name, kind, build, depth=32, times=TIMES, rays=200):
        self.name, self.kind, self.build, self.depth, self.times, self.ray_count = name, kind, build, depth, times, rays
        self.forced = depth < 32

    def __repr__(self):
        return self.name


CASES = ([Case("ranges_common", "ranges", lambda rt: time_range_scene(rt, True), rays=300), Case("ranges_mixed", "ranges", lambda rt: time_range_scene(rt, False), rays=300),
          Case("ranges_general", "general", general_time_range_scene, rays=300)]
         + [Case("one_" + w, "one", lambda rt, w=w: one_entity_scene(rt, w), rays=150) for w in ONE_ENTITY]
         + [Case("planes_d%d" % d, "planes", plane_scene, depth=d, times=(0.0,)) for d in (32, 1)]
         + [Case("fuzz%d_d%d" % (s, d), "fuzz", lambda rt, s=s: fz._random_scene(rt, 1000 + s)[0], depth=d, times=FUZZ_TIMES) for s in FUZZ_SEEDS for d in FUZZ_DEPTHS])
BY_NAME = {c.name: c for c in CASES}
DEVICE_VARIANT_CASES = [c for c in CASES if c.forced or c.kind == "ranges"]          # also run under wide codes and with the tree in HBM


class Expected:
    """What the brute force says about one case: per ray the nearest distance under (0, +inf) (`first`), and per interval family and ray (distance, minimal set,
    any-hit, the normal where the set has one member).  `own_boxes`: the entities' own boxes (what plane_rays is made from)."""


_cache = {}


def case_rays(rt, case, scene, own_boxes):
    """(pairs, times) of a case; the mixed-range scene's twin rays come last"""
    if case.kind == "planes":
        pairs = plane_rays(own_boxes)
    else:
        pairs = list(tr._rays(scene, case.ray_count, 11)) + list(tr._axis_rays(scene, 12))
    times = [case.times[k % len(case.times)] for k in range(len(pairs))]
    if case.name == "ranges_mixed":
        p, t = twin_rays(scene)
        pairs, times = pairs + p, times + t
    return pairs, times


def expected(rt, oracle, case):
    """The Expected of a case, computed once per process (the reference's self-check against OracleScene.hit_world runs on every ray of it)"""
    if case.name in _cache:
        return _cache[case.name]
    x = Expected()
    x.scene = case.build(rt)
    x.desc = x.scene.desc(max_bvh_depth=case.depth)
    ref = ir.IntervalReference(oracle, x.desc)
    try:
        x.own_boxes = ref.own_bounds.copy()
        x.forced_entities = int((ref.bounds.view(np.uint32) != ref.own_bounds.view(np.uint32)).any(axis=1).sum())
        x.pairs, x.times = case_rays(rt, case, x.scene, x.own_boxes)
        cands = ref.rays(x.pairs, x.times)
        x.first = np.asarray([rc.first for rc in cands], np.float32)
        x.draws = np.random.default_rng(29).random(len(x.pairs)).astype(np.float32)
        x.families = ir.family_intervals(x.first, x.draws)
        x.want = {}
        for fam, iv in x.families.items():
            rows = []
            for k, rc in enumerate(cands):
                t, members, anyhit = rc.query(iv[k, 0], iv[k, 1])
                normal = rc.normal(next(iter(members)), iv[k, 0], iv[k, 1]) if len(members) == 1 else None
                rows.append((t, members, anyhit, normal))
            x.want[fam] = rows
    finally:
        ref.close()
    _cache[case.name] = x
    return x


def ray_array(rt, x):
    return tr._ray_array(rt, x.pairs, x.times)


# ---- input conditions, from the oracle alone ------------------------------------------------------------------------------------------------------------------------------
def hit_world_answers(oracle, desc, pairs, times):
    """(n,) uint64: OracleScene.hit_world's hit bit and distance bits of every ray, one time for all rays if `times` is a number"""
    osc = oracle.OracleScene(desc)
    try:
        out = np.zeros(len(pairs), np.uint64)
        for k, (o, d) in enumerate(pairs):
            hit, rec = osc.hit_world(o, d, times if np.isscalar(times) else times[k])
            out[k] = (int(np.float32(rec[0]).view(np.uint32)) | (1 << 32)) if hit else 0
        return out
    finally:
        osc.close()


def rays_that_differ_from_the_range_start(oracle, x, time):
    """how many rays of a time-range case answer differently at ray time `time` than at 0.25, the start of RANGES[0]"""
    return int((hit_world_answers(oracle, x.desc, x.pairs, time) != hit_world_answers(oracle, x.desc, x.pairs, 0.25)).sum())


def twin_set_sizes(x, pair):
    """per twin ray j (x's last rays): the sizes of the brute force's minimal set under (0, +inf) at the three TWIN_TIMES, counting only sets made of the pair's members"""
    n = len(x.pairs)
    base = n - 3 * TWIN_RAYS
    sizes = []
    for j in range(TWIN_RAYS):
        row = []
        for i in range(3):
            _, members, _, _ = x.want["null"][base + 3 * j + i]
            row.append(len(members) if members and members <= frozenset(pair) else 0)
        sizes.append(tuple(row))
    return sizes


# ---- the sample path on the time-range scenes (tests/test_gpu_time_ranges.py) ----------------------------------------------------------------------------------------------
FRAME = (64, 36, 4, 6)                                                           # width, height, samples per pixel, trace depth
FRAME_SCENES = {"ranges_common": lambda rt, unit=False: time_range_scene(rt, True, unit), "ranges_mixed": lambda rt, unit=False: time_range_scene(rt, False, unit),
                "ranges_general": lambda rt, unit=False: general_time_range_scene(rt, unit)}
_frames = {}


def frame_params(rt, scene, policy, seed=1):
    w, h, spp, depth = FRAME
    return rt.scenes.make_params(scene, w, h, spp=spp, trace_depth=depth, seed=seed, rng_policy=policy)


def oracle_frames(rt, oracle, name, policy, unit_ranges=False):
    """(scene, desc, [first batch, second batch on top of it]) of OracleScene.sample_batch with seeds 1 and 2, computed once per process"""
    key = (name, policy, unit_ranges)
    if key not in _frames:
        scene = FRAME_SCENES[name](rt, unit_ranges)
        desc = scene.desc()
        osc = oracle.OracleScene(desc)
        try:
            first = osc.sample_batch(frame_params(rt, scene, policy, 1))
            second = osc.sample_batch(frame_params(rt, scene, policy, 2), {k: first[k] for k in ("color", "normal", "albedo", "scw")})
        finally:
            osc.close()
        _frames[key] = (scene, desc, [first, second])
    return _frames[key]


def share_of_pixels_the_ranges_change(rt, oracle, name, policy):
    """of the first batch's pixels, the share whose colour differs from the same scene's with every TimeRange set to (0, 1)"""
    a, b = oracle_frames(rt, oracle, name, policy)[2][0]["color"], oracle_frames(rt, oracle, name, policy, unit_ranges=True)[2][0]["color"]
    return float((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).mean())
