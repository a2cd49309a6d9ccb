"""GPU: rtowTraceRaysDevice / rtowTraceViewDevice - batched nearest-hit queries on the device - against the host probe (rtowProbeNearestHit, every ray), against the
oracle's Raytracer.HitWorld (distance, normal and entity bit for bit), the view form against its formula and against the sample path's first hit, partial outputs with
guard words, odd counts, stream order behind a chain of sample batches, wide codes and HBM-resident trees.  One GPU context at a time."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCENES = ["cover", "moving", "mixed", "volumes", "mesh", "textured", "twins", "tiny", "coplanar", "stress"]
MOVING = ("moving", "twins")
TIE_CAP = {"twins": 0.35, "coplanar": 0.35}      # share of hitting rays whose entity HitWorld and the job's sorted hit list name differently (bit-identical distances); 1 % elsewhere


def _scene(rt, name):
    S = rt.scenes
    return {"cover": S.cover_scene, "moving": S.moving_scene, "mixed": S.mixed_scene, "volumes": S.volume_scene, "mesh": lambda: S.mesh_scene(3), "textured": S.textured_scene,
            "twins": lambda: S.twin_spheres_scene(True), "tiny": S.tiny_scene, "stress": lambda: S.stress_scene(count=3000, max_tentatives=12000), "coplanar": S.coplanar_scene}[name]()


def _rays(scene, count, seed):
    """tests/test_gpu_probe.py's ray generator"""
    rng = np.random.default_rng(seed)
    cam = np.asarray(scene.camera["position"], dtype=np.float32)
    target = np.asarray(scene.camera["target"], dtype=np.float32)
    yield cam, (target - cam).astype(np.float32)                                   # the view axis itself, unnormalised
    for k in range(count):
        o = cam if k % 2 == 0 else (cam + rng.normal(size=3) * 2.0).astype(np.float32)
        d = (target - o + rng.normal(size=3) * (0.05 if k % 4 == 0 else 1.5)).astype(np.float32)
        if k % 3 == 0: d = (d / np.linalg.norm(d)).astype(np.float32)
        if k % 17 == 0: d = -d                                                     # mostly misses
        yield o, d


def _axis_rays(scene, seed):
    """rays with one or two direction components exactly zero (+0 and -0), from the camera, from the target and from points around it"""
    rng = np.random.default_rng(seed)
    cam = np.asarray(scene.camera["position"], dtype=np.float32)
    target = np.asarray(scene.camera["target"], dtype=np.float32)
    origins = [cam, target] + [(target + rng.normal(size=3) * 3.0).astype(np.float32) for _ in range(10)]
    for o in origins:
        for axis in range(3):
            for sign in (1.0, -1.0):
                d = np.zeros(3, np.float32)
                d[axis] = sign
                yield o, d
                d = d.copy()
                d[(axis + 1) % 3] = np.float32(-0.0)
                yield o, d
                d = d.copy()
                d[(axis + 2) % 3] = np.float32(rng.normal())                      # one exact zero left
                yield o, d


def _ray_array(rt, pairs, times):
    a = np.zeros(len(pairs), dtype=np.dtype(rt.abi.RAY_DTYPE))
    a["origin"] = np.asarray([o for o, _ in pairs], np.float32)
    a["direction"] = np.asarray([d for _, d in pairs], np.float32)
    a["time"] = np.asarray(times, np.float32)
    a["pad"] = np.float32(np.nan)                                                  # ignored by the library
    return a


def _test_rays(rt, scene, name, timed):
    gen = list(_rays(scene, 2000, 11))
    pairs = gen + list(_axis_rays(scene, 12))
    rng = np.random.default_rng(3)
    draws = rng.random(len(pairs)).astype(np.float32)
    draws = np.clip(draws, np.float32(2.0 ** -20), np.float32(1.0 - 2.0 ** -20))
    times = [float(draws[k]) if (timed and name in MOVING and k % 2) else 0.0 for k in range(len(pairs))]
    return pairs, times, len(gen)


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _check_against_probe(rt, ctx, name, scene):
    pairs, times, _ = _test_rays(rt, scene, name, timed=True)
    got = ctx.trace_rays(_ray_array(rt, pairs, times))
    dist = np.zeros(len(pairs), np.float32)
    ent = np.zeros(len(pairs), np.int32)
    for k, ((o, d), t) in enumerate(zip(pairs, times)):
        _, dist[k], ent[k] = ctx.hit_world(o, d, t)
    assert np.array_equal(_u32(got["distance"]), _u32(dist)), (name, np.flatnonzero(_u32(got["distance"]) != _u32(dist))[:8])
    assert np.array_equal(got["entityIndex"], ent), (name, np.flatnonzero(got["entityIndex"] != ent)[:8])
    miss = ent < 0
    assert miss.any() and (~miss).any(), name
    assert np.all(np.isposinf(got["distance"][miss])) and np.all(got["entityIndex"][miss] == -1)
    assert np.all(_u32(got["normal"][miss]) == 0), name                           # (+0, +0, +0)
    assert np.all(np.isfinite(got["distance"][~miss])), name


@pytest.mark.parametrize("name", SCENES)
def test_every_ray_equals_the_host_probe(rt, name):
    """1. distance (as uint32) and entityIndex of EVERY ray, hits and misses, equal rtowProbeNearestHit's; misses give +inf, -1 and a zero normal."""
    scene = _scene(rt, name)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        _check_against_probe(rt, ctx, name, scene)


@pytest.mark.parametrize("name", SCENES)
def test_hits_equal_the_oracles_hit_world(rt, oracle, name):
    """2. hit or miss and the distance bits for every ray; entity and the three normal words bit for bit wherever HitWorld and the job's sorted hit list name the same
    entity (tests/test_gpu_probe.py's rule for ties); the share of hitting rays that rule leaves out is capped: 1 % (35 % in twins and coplanar)."""
    scene = _scene(rt, name)
    desc = scene.desc()
    pairs, times, generated = _test_rays(rt, scene, name, timed=False)            # ray time 0: the setting the caps were counted at
    with rt.Context(0) as ctx:
        ctx.upload_scene(desc)
        got = ctx.trace_rays(_ray_array(rt, pairs, times))
    osc = oracle.OracleScene(desc)
    hits = misses = tied = 0
    try:
        for k, ((o, d), t) in enumerate(zip(pairs, times)):
            ref_hit, ref = osc.hit_world(o, d, t)
            counted = k < generated                                               # the axis rays are compared too, but the caps are about the generator's rays
            assert (got["entityIndex"][k] >= 0) == ref_hit, (name, k)
            if not ref_hit:
                misses += counted
                assert np.isposinf(got["distance"][k]) and got["entityIndex"][k] == -1 and np.all(_u32(got["normal"][k]) == 0), (name, k)
                continue
            hits += counted
            assert _u32(got["distance"][k]) == _u32(ref[0]), (name, k, got["distance"][k], ref[0])
            _, job = osc.nearest_hit(o, d, t)
            if int(ref[7]) != int(job[7]):
                tied += counted
                continue
            assert got["entityIndex"][k] == int(ref[7]), (name, k)
            assert np.array_equal(_u32(got["normal"][k]), _u32(ref[4:7])), (name, k, got["normal"][k], ref[4:7])
    finally:
        osc.close()
    print("%s: %d hits, %d misses, %d tied of the generator's %d rays" % (name, hits, misses, tied, generated))
    assert hits > 1000 and misses > 20, (name, hits, misses)
    assert tied <= TIE_CAP.get(name, 0.01) * hits, (name, tied, hits)


def _view_params(rt, scene, w, h, **kw):
    p = rt.scenes.make_params(scene, w, h, spp=1, trace_depth=1, jitter=False, noise_color=rt.abi.NOISE_WHITE, **kw)
    p.view.lensRadius = 0.0
    return p


def _expected_directions(view, w, h):
    f = lambda v: np.asarray([np.float32(v.x), np.float32(v.y), np.float32(v.z)], np.float64)
    col, row = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u, v = ((col + 0.5) / w).reshape(-1, 1), ((row + 0.5) / h).reshape(-1, 1)
    d = f(view.lowerLeftCorner) + u * f(view.horizontal) + v * f(view.vertical)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@pytest.mark.parametrize("name", ["cover", "mixed", "mesh"])
@pytest.mark.parametrize("size", [(96, 54), (101, 37)])
def test_view_rays_follow_the_formula_and_feed_back(rt, name, size):
    """3a. outRays: origin bits = view.origin, time = the parameter, every direction component within 1e-6 of the float64 value of the formula, relative to the
    direction's length (1): a float32 dot, rsqrt-or-sqrt and multiply are a handful of half-ulp roundings, 2^-20 is the margin.  (Relative to the component itself
    the bound would mean nothing: lowerLeftCorner + u * horizontal cancels towards the image centre - `mixed` at 101 columns has u = 1/2 exactly in the middle
    column, where the float64 x component is the rounding residue of the view's own float32 fields and the float32 sum is 0 - so no float32 evaluation of the
    formula, the sample kernel's included, keeps a component-relative bound there.)  The same rays through trace_rays return the same three buffers bit for bit."""
    w, h = size
    scene = _scene(rt, name)
    view = _view_params(rt, scene, w, h).view
    t = 0.25
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        got = ctx.trace_view(view, w, h, time=t, want_rays=True)
        again = ctx.trace_rays(got["rays"])
    rays = got["rays"]
    assert rays.shape == (w * h,)
    assert np.all(_u32(rays["origin"]) == _u32([view.origin.x, view.origin.y, view.origin.z]))
    assert np.all(_u32(rays["time"]) == _u32(t))
    want = _expected_directions(view, w, h)
    err = np.abs(rays["direction"].astype(np.float64) - want)
    print("%s %dx%d: largest direction error per component, relative to the direction's length: %.3g" % (name, w, h, err.max()))
    assert np.all(err <= 1e-6), (name, err.max())
    for k in ("distance", "entityIndex", "normal"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(again[k]).view(np.uint32)), (name, k)
    assert (got["entityIndex"] >= 0).sum() > w * h // 4, name


@pytest.mark.parametrize("name", ["cover", "mixed"])
def test_view_normal_is_the_sample_paths_first_hit_normal(rt, name):
    """3b. rtowSampleBatchDevice from zeroed accumulators with 1 sample, jitter off, lensRadius 0, traceDepth 1, white noise: normal[p] equals hits.normal[p] bit for
    bit at every pixel with a hit (JOBS/SampleBatchJob.cs:313-314: sampleNormal = rec.Normal at depth 0).

    Two properties of the reference, neither a tolerance:
     * the accumulator holds 0 + N: a component of N that is -0 is stored as +0, so the query's normal is compared after the same `0 + x`;
     * the sample path draws every ray's Ray.Time at random (JOBS/SampleBatchJob.cs:134), the query takes one time for all.  `mixed` has two moving entities (a box and
       a sphere): pixels that see one of them see it at another time in the sample path.  Those pixels are left out by the query itself - a pixel is compared when the
       view query names the same non-moving entity at ray times 0, 1/4, 1/2, 3/4 and 1 - and they are few: the two entities are small in a room that fills the frame,
       so at least half of the frame's hit pixels must remain.  `cover` has no moving entity: every hit pixel is compared."""
    w, h = 96, 54
    scene = _scene(rt, name)
    p = _view_params(rt, scene, w, h)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        sample = rt.sample_batch_host(ctx, p)
        views = [ctx.trace_view(p.view, w, h, time=t) for t in (0.0, 0.25, 0.5, 0.75, 1.0)]
    ent = views[0]["entityIndex"]
    hit = ent >= 0
    moving = np.asarray(scene.moving, bool)
    keep = hit.copy()
    if moving.any():
        for v in views[1:]:
            keep &= v["entityIndex"] == ent
        keep &= ~moving[np.maximum(ent, 0)]
    else:
        for v in views[1:]:
            assert np.array_equal(v["entityIndex"], ent) and np.array_equal(_u32(v["normal"]), _u32(views[0]["normal"])), name
    print("%s: %d of %d hit pixels compared" % (name, keep.sum(), hit.sum()))
    assert keep.sum() >= (hit.sum() if not moving.any() else hit.sum() // 2) and hit.sum() > w * h // 4
    accumulated = np.zeros((w * h, 3), np.float32) + views[0]["normal"]
    assert np.array_equal(_u32(sample["normal"][keep]), _u32(accumulated[keep])), (name, np.flatnonzero((_u32(sample["normal"]) != _u32(accumulated)).any(axis=1) & keep)[:8])
    assert np.any(sample["normal"][keep] != 0)


GUARD = 0x5ca1ab1e


def test_partial_outputs_guard_words_counts_and_validation(rt):
    """4. each hit pointer NULL in turn: the others unchanged bit for bit, memory next to every buffer untouched; counts 1, 63, 64, 65, 1000; argument validation with a
    real context; RTOW_ERROR_NO_SCENE before the upload."""
    a = rt.abi
    lib = rt.lib.load()
    scene = _scene(rt, "mixed")
    pairs, times, _ = _test_rays(rt, scene, "mixed", timed=True)
    rays = _ray_array(rt, pairs, times)
    with rt.Context(0) as ctx:
        one = rt.DeviceBuffer(ctx, 4096).zero()
        hb = a.HitBuffers(one.handle.value, None, None)
        vp = a.TraceViewParams(8, 8, a.View(), 0.0, 0)
        assert lib.rtowTraceRaysDevice(ctx.handle, 1, one.handle, C.byref(hb), None) == a.RTOW_ERROR_NO_SCENE
        assert lib.rtowTraceViewDevice(ctx.handle, C.byref(vp), C.byref(hb), None, None) == a.RTOW_ERROR_NO_SCENE
        ctx.upload_scene(scene.desc())
        bad = a.RTOW_ERROR_INVALID_VALUE
        none = a.HitBuffers(None, None, None)
        assert lib.rtowTraceRaysDevice(ctx.handle, 1, None, C.byref(hb), None) == bad
        assert lib.rtowTraceRaysDevice(ctx.handle, 1, one.handle, None, None) == bad
        assert lib.rtowTraceRaysDevice(ctx.handle, 1, one.handle, C.byref(none), None) == bad
        assert lib.rtowTraceRaysDevice(ctx.handle, -1, one.handle, C.byref(hb), None) == bad
        assert lib.rtowTraceRaysDevice(ctx.handle, 0, one.handle, C.byref(hb), None) == 0
        assert lib.rtowTraceViewDevice(ctx.handle, None, C.byref(hb), None, None) == bad
        assert lib.rtowTraceViewDevice(ctx.handle, C.byref(vp), None, None, None) == bad
        assert lib.rtowTraceViewDevice(ctx.handle, C.byref(vp), C.byref(none), None, None) == bad
        for p in (a.TraceViewParams(0, 8, a.View(), 0.0, 0), a.TraceViewParams(8, 0, a.View(), 0.0, 0), a.TraceViewParams(65536, 32768, a.View(), 0.0, 0),
                  a.TraceViewParams(8, 8, a.View(), 0.0, 7)):
            assert lib.rtowTraceViewDevice(ctx.handle, C.byref(p), C.byref(hb), None, None) == bad
        ctx.synchronize()
        assert not one.download(np.uint32, (1024,)).any()                          # nothing was enqueued by any refused call (or by count == 0)
        one.free()

        full = ctx.trace_rays(rays)
        for count in (1, 63, 64, 65, 1000, len(rays)):
            for absent in (None, "distance", "entityIndex", "normal"):
                words = {"distance": count, "entityIndex": count, "normal": 3 * count}
                bufs = {}
                for k, n in words.items():
                    if k != absent:
                        bufs[k] = rt.DeviceBuffer(ctx, (n + 32) * 4).upload(np.full(n + 32, GUARD, np.uint32))
                dev = rt.DeviceBuffer(ctx, count * 32).upload(rays[:count])
                hits = a.HitBuffers(*[(bufs[k].handle.value + 64) if k in bufs else None for k in ("distance", "entityIndex", "normal")])
                rt.lib.check(lib.rtowTraceRaysDevice(ctx.handle, count, dev.handle, C.byref(hits), None), "rtowTraceRaysDevice")
                ctx.synchronize()
                for k, n in words.items():
                    if k == absent:
                        continue
                    raw = bufs[k].download(np.uint32, (n + 32,))
                    assert np.all(raw[:16] == GUARD) and np.all(raw[16 + n:] == GUARD), (count, absent, k)
                    assert np.array_equal(raw[16:16 + n], np.ascontiguousarray(full[k][:count]).reshape(-1).view(np.uint32)), (count, absent, k)
                for b in list(bufs.values()) + [dev]:
                    b.free()


def test_a_query_behind_a_chain_of_sample_batches_returns_the_idle_hits(rt):
    """4. (order) a view query and a ray query enqueued on the context's stream directly after a chain of sample batches return the hits of an idle device"""
    a = rt.abi
    lib = rt.lib.load()
    scene = _scene(rt, "cover")
    w, h = 160, 90
    n = w * h
    view = _view_params(rt, scene, w, h).view
    plist = [rt.scenes.make_params(scene, w, h, spp=8, trace_depth=8, seed=s) for s in (1, 2, 3)]
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        idle = ctx.trace_view(view, w, h, time=0.0, want_rays=True)
        acc = [rt.DeviceBuffer(ctx, n * c * 4).zero() for c in (4, 3, 3, 1)]
        out = {k: rt.DeviceBuffer(ctx, n * c * 4).zero() for k, c in (("distance", 1), ("entityIndex", 1), ("normal", 3))}
        out2 = {k: rt.DeviceBuffer(ctx, n * c * 4).zero() for k, c in (("distance", 1), ("entityIndex", 1), ("normal", 3))}
        rays = rt.DeviceBuffer(ctx, n * 32).upload(idle["rays"])
        vp = a.TraceViewParams(w, h, view, 0.0, 0)
        hv = a.HitBuffers(out["distance"].handle.value, out["entityIndex"].handle.value, out["normal"].handle.value)
        hr = a.HitBuffers(out2["distance"].handle.value, out2["entityIndex"].handle.value, out2["normal"].handle.value)
        rt.lib.check(rt.sample_batch_chain_device(ctx, plist, acc, acc), "rtowSampleBatchChainDevice")
        rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(vp), C.byref(hv), None, None), "rtowTraceViewDevice")
        rt.lib.check(lib.rtowTraceRaysDevice(ctx.handle, n, rays.handle, C.byref(hr), None), "rtowTraceRaysDevice")
        ctx.synchronize()
        for o in (out, out2):
            assert np.array_equal(o["distance"].download(np.uint32, (n,)), _u32(idle["distance"]))
            assert np.array_equal(o["entityIndex"].download(np.int32, (n,)), idle["entityIndex"])
            assert np.array_equal(o["normal"].download(np.uint32, (n, 3)), _u32(idle["normal"]))
        assert acc[0].download(np.float32, (n, 4))[:, 3].min() > 0                 # the chain ran


@pytest.mark.parametrize("how", ["wide", "hbm"])
def test_wide_codes_and_hbm_resident_trees_do_not_matter(rt, how):
    """5. check 1 on mesh(3) under RTOW_CONTEXT_FORCE_WIDE_CODES, and with an LDS scene budget so small that the sample kernels read the tree from HBM"""
    scene = _scene(rt, "mesh")
    kw = {"flags": rt.abi.CONTEXT_FORCE_WIDE_CODES} if how == "wide" else {"lds_scene_budget": 1024}
    with rt.Context(0, **kw) as ctx:
        ctx.upload_scene(scene.desc())
        info = ctx.scene_info()
        assert (info.wideCodes == 1) if how == "wide" else (info.sceneInLds == 0), (how, info.wideCodes, info.sceneInLds)
        _check_against_probe(rt, ctx, "mesh", scene)
