"""GPU: rtowTraceRaysIntervalDevice / rtowTraceOcclusionDevice - ray queries with a parameter interval - against rtowTraceRaysDevice (NULL intervals: bit for bit), the
host probe rtowProbeNearestHitInterval (every ray, every interval family), each other (occlusion = the nearest form names an entity) and the brute-force reference of
tests/trace_interval_reference.py (oracle calls only); peeling, intervals that are not traced, odd counts, odd addresses, partial outputs with guard words, count == 0
and the argument validation with a real context.  One GPU context at a time."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_trace_rays as tr  # noqa: E402  (its scenes and ray generators)
import trace_interval_reference as ir  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = ["cover", "moving", "mixed", "volumes", "mesh", "textured", "twins", "tiny", "coplanar"]
GUARD = 0x5ca1ab1e
_u32 = tr._u32


def _rays_and_draws(rt, scene, name, thinned=False):
    if thinned:
        pairs, times = ir.interval_rays(tr, rt, scene, name)
    else:
        pairs, times, _ = tr._test_rays(rt, scene, name, timed=True)
    draws = np.random.default_rng(29).random(len(pairs)).astype(np.float32)
    return pairs, times, draws


def _check_against_trace_rays_probe_and_occlusion(rt, ctx, name, scene):
    """properties 1, 2, 3 and 6 on one resident scene"""
    pairs, times, draws = _rays_and_draws(rt, scene, name)
    rays = tr._ray_array(rt, pairs, times)
    plain = ctx.trace_rays(rays)
    null = ctx.trace_rays_interval(rays)                                            # 1. NULL intervals: rtowTraceRaysDevice bit for bit
    for k in ("distance", "entityIndex", "normal"):
        assert np.array_equal(np.ascontiguousarray(null[k]).view(np.uint32), np.ascontiguousarray(plain[k]).view(np.uint32)), (name, k)
    assert np.array_equal(ctx.trace_occlusion(rays), (plain["entityIndex"] >= 0).astype(np.uint8)), name
    hit = plain["entityIndex"] >= 0
    assert hit.any() and (~hit).any(), name
    later = np.zeros(len(pairs), bool)
    occluded_seen = clear_seen = 0
    for fam, iv in ir.family_intervals(plain["distance"], draws).items():
        got = ctx.trace_rays_interval(rays, iv)
        dist = np.zeros(len(pairs), np.float32)
        ent = np.zeros(len(pairs), np.int32)
        for k, ((o, d), t) in enumerate(zip(pairs, times)):                         # 2. every ray equals the host probe
            _, dist[k], ent[k] = ctx.hit_world_interval(o, d, t, iv[k, 0], iv[k, 1])
        assert np.array_equal(_u32(got["distance"]), _u32(dist)), (name, fam, np.flatnonzero(_u32(got["distance"]) != _u32(dist))[:8])
        assert np.array_equal(got["entityIndex"], ent), (name, fam, np.flatnonzero(got["entityIndex"] != ent)[:8])
        miss = ent < 0
        assert np.all(np.isposinf(got["distance"][miss])) and np.all(_u32(got["normal"][miss]) == 0), (name, fam)
        assert np.all(np.isfinite(got["distance"][~miss])), (name, fam)
        occ = ctx.trace_occlusion(rays, iv)                                         # 3. occlusion = the nearest form names an entity
        assert occ.dtype == np.uint8 and np.array_equal(occ, (~miss).astype(np.uint8)), (name, fam, np.flatnonzero(occ != (~miss))[:8])
        if fam in ir.INVALID:                                                       # 6. intervals that are not traced
            assert miss.all() and not occ.any(), (name, fam)
        elif fam == "null":
            assert np.array_equal(_u32(got["distance"]), _u32(plain["distance"])) and np.array_equal(_u32(got["normal"]), _u32(plain["normal"])), name
        else:
            occluded_seen += int((~miss).sum())
            clear_seen += int(miss.sum())
            later |= ~miss & hit & (got["distance"] > plain["distance"]) & (iv[:, 0] >= plain["distance"])
    print("%s: %d rays, %d hit; over the valid families %d occluded, %d clear; %d rays with a later hit behind an excluded nearest one" %
          (name, len(pairs), hit.sum(), occluded_seen, clear_seen, later.sum()))
    assert occluded_seen > 0 and clear_seen > 0 and later.any(), name


@pytest.mark.parametrize("name", SCENES)
def test_null_intervals_the_host_probe_and_occlusion_agree_on_every_ray(rt, name):
    """1. NULL intervals: distance, entity and normal of rtowTraceRaysDevice bit for bit.  2. every ray under every interval family: distance bits and entity of
    rtowProbeNearestHitInterval.  3. rtowTraceOcclusionDevice = (entityIndex >= 0) of the nearest form on the same rays and intervals.  6. the three kinds of interval
    that are not traced give a miss / 0."""
    scene = tr._scene(rt, name)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        _check_against_trace_rays_probe_and_occlusion(rt, ctx, name, scene)


def test_stress_scene_with_its_tree_in_hbm(rt):
    """11. 3000 spheres: properties 1 - 3 only"""
    scene = tr._scene(rt, "stress")
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        _check_against_trace_rays_probe_and_occlusion(rt, ctx, "stress", scene)


@pytest.mark.parametrize("name", SCENES)
def test_every_ray_equals_the_brute_force_reference(rt, oracle, name):
    """4. distance bits and any-hit of every ray under every family equal the brute force over the oracle's Entity.Hit; the entity is in its minimal set; where that set
    has one member, the normal is that Entity.Hit's HitRecord.Normal (a sphere's far root and a box's exit face included) bit for bit after `0 + x` on both sides: a
    component that is -0 is compared as +0.  That is a property of the normal rtowTraceRaysDevice already returns, which NULL intervals must reproduce bit for bit: the
    sphere kinds skip the rotation by the identity quaternion, through which the reference's -0 becomes +0 (v + q.w * t + cross(q.xyz, t) with t = 0) - the tiny scene's
    negative-radius shell hit along an axis shows it; tests/test_gpu_trace_rays.py compares the sample path's accumulated normal the same way.  The mesh: the thinned
    ray set."""
    scene = tr._scene(rt, name)
    desc = scene.desc()
    pairs, times, draws = _rays_and_draws(rt, scene, name, thinned=True)
    rays = tr._ray_array(rt, pairs, times)
    ref = ir.IntervalReference(oracle, desc)
    try:
        cands = ref.rays(pairs, times)
        first = np.asarray([rc.first for rc in cands], np.float32)
        families = ir.family_intervals(first, draws)
        with rt.Context(0) as ctx:
            ctx.upload_scene(desc)
            got = {fam: (ctx.trace_rays_interval(rays, iv), ctx.trace_occlusion(rays, iv)) for fam, iv in families.items()}
        normals = 0
        zero = np.zeros(3, np.float32)
        for fam, iv in families.items():
            g, occ = got[fam]
            for k, rc in enumerate(cands):
                want_t, want_set, want_any = rc.query(iv[k, 0], iv[k, 1])
                assert _u32(g["distance"][k]) == _u32(want_t), (name, fam, k, g["distance"][k], want_t)
                assert bool(occ[k]) == want_any, (name, fam, k)
                e = int(g["entityIndex"][k])
                assert (e in want_set) if want_any else e == -1, (name, fam, k, e, sorted(want_set))
                if len(want_set) == 1:
                    normals += 1
                    assert np.array_equal(_u32(g["normal"][k] + zero), _u32(rc.normal(e, iv[k, 0], iv[k, 1]) + zero)), (name, fam, k)
    finally:
        ref.close()
    assert normals >= 100, (name, normals)


def test_peeling_on_the_cover_scene(rt, oracle):
    """5. tMin = the next float above each ray's first distance: a miss or strictly farther, and the reference's answer; a second peel likewise"""
    scene = tr._scene(rt, "cover")
    desc = scene.desc()
    pairs, times, _ = _rays_and_draws(rt, scene, "cover")
    pairs, times = pairs[::3], times[::3]
    rays = tr._ray_array(rt, pairs, times)
    ref = ir.IntervalReference(oracle, desc)
    try:
        cands = [ref.ray(o, d, t) for (o, d), t in zip(pairs, times)]
        with rt.Context(0) as ctx:
            ctx.upload_scene(desc)
            layer = ctx.trace_rays(rays)
            peeled = 0
            for depth in range(2):
                iv = np.stack([np.nextafter(layer["distance"], np.float32(np.inf)), np.full(len(pairs), np.inf, np.float32)], axis=1).astype(np.float32)
                nxt = ctx.trace_rays_interval(rays, iv)
                had = layer["entityIndex"] >= 0
                assert np.all(nxt["entityIndex"][~had] == -1), depth                # behind a miss (tMin = +inf) there is nothing
                hit = nxt["entityIndex"] >= 0
                assert np.all(nxt["distance"][hit] > layer["distance"][hit]), depth
                for k, rc in enumerate(cands):
                    want_t, want_set, want_any = rc.query(iv[k, 0], iv[k, 1])
                    assert _u32(nxt["distance"][k]) == _u32(want_t) and ((int(nxt["entityIndex"][k]) in want_set) if want_any else nxt["entityIndex"][k] == -1), (depth, k)
                peeled += int(hit.sum())
                layer = nxt
    finally:
        ref.close()
    assert peeled > 200, peeled


def test_counts_odd_addresses_partial_outputs_guard_words_and_validation(rt):
    """7. counts 1, 63, 65, 257.  8. rays and intervals at a 4-byte offset, `occluded` at an odd byte address.  9. outputs not asked for, and guard words around every
    output, are untouched.  10. count == 0 launches nothing; the validation of include/rtow.h with a real context; RTOW_ERROR_NO_SCENE before the upload."""
    a = rt.abi
    lib = rt.lib.load()
    scene = tr._scene(rt, "mixed")
    pairs, times, draws = _rays_and_draws(rt, scene, "mixed")
    rays = tr._ray_array(rt, pairs, times)
    with rt.Context(0) as ctx:
        one = rt.DeviceBuffer(ctx, 4096).zero()
        hb = a.HitBuffers(one.handle.value, None, None)
        o3, d3 = a.Float3(0, 0, 5), a.Float3(0, 0, -1)
        assert lib.rtowTraceRaysIntervalDevice(ctx.handle, 1, one.handle, None, C.byref(hb), None) == a.RTOW_ERROR_NO_SCENE
        assert lib.rtowTraceOcclusionDevice(ctx.handle, 1, one.handle, None, one.handle, None) == a.RTOW_ERROR_NO_SCENE
        assert lib.rtowProbeNearestHitInterval(ctx.handle, C.byref(o3), C.byref(d3), 0.0, 0.0, 1.0, None, None) == a.RTOW_ERROR_NO_SCENE
        ctx.upload_scene(scene.desc())
        bad = a.RTOW_ERROR_INVALID_VALUE
        none = a.HitBuffers(None, None, None)
        assert lib.rtowTraceRaysIntervalDevice(ctx.handle, 1, None, None, C.byref(hb), None) == bad
        assert lib.rtowTraceRaysIntervalDevice(ctx.handle, 1, one.handle, None, None, None) == bad
        assert lib.rtowTraceRaysIntervalDevice(ctx.handle, 1, one.handle, None, C.byref(none), None) == bad
        assert lib.rtowTraceRaysIntervalDevice(ctx.handle, -1, one.handle, None, C.byref(hb), None) == bad
        assert lib.rtowTraceRaysIntervalDevice(ctx.handle, 0, one.handle, None, C.byref(hb), None) == 0
        assert lib.rtowTraceOcclusionDevice(ctx.handle, 1, None, None, one.handle, None) == bad
        assert lib.rtowTraceOcclusionDevice(ctx.handle, 1, one.handle, None, None, None) == bad
        assert lib.rtowTraceOcclusionDevice(ctx.handle, -1, one.handle, None, one.handle, None) == bad
        assert lib.rtowTraceOcclusionDevice(ctx.handle, 0, one.handle, None, one.handle, None) == 0
        assert lib.rtowProbeNearestHitInterval(ctx.handle, None, C.byref(d3), 0.0, 0.0, 1.0, None, None) == bad
        assert lib.rtowProbeNearestHitInterval(ctx.handle, C.byref(o3), C.byref(d3), 0.0, 0.0, 1.0, None, None) == 0
        ctx.synchronize()
        assert not one.download(np.uint32, (1024,)).any()                          # nothing was enqueued by any refused call (or by count == 0)
        one.free()

        first = ctx.trace_rays(rays, want=("distance",))["distance"]
        iv = ir.family_intervals(first, draws)["sub_near"]
        full = ctx.trace_rays_interval(rays, iv)
        full_occ = ctx.trace_occlusion(rays, iv)
        assert 0 < int(full_occ.sum()) < len(rays)
        for count in (1, 63, 65, 257):
            for absent in (None, "distance", "entityIndex", "normal"):
                words = {"distance": count, "entityIndex": count, "normal": 3 * count}
                bufs = {k: rt.DeviceBuffer(ctx, (n + 32) * 4).upload(np.full(n + 32, GUARD, np.uint32)) for k, n in words.items() if k != absent}
                # rays and intervals one float into their allocations; `occluded` 16 guard words and one byte in
                dev = rt.DeviceBuffer(ctx, count * 32 + 4).upload(np.concatenate([np.zeros(1, np.float32), rays[:count].view(np.float32).reshape(-1)]))
                div = rt.DeviceBuffer(ctx, count * 8 + 4).upload(np.concatenate([np.zeros(1, np.float32), iv[:count].reshape(-1)]))
                occ_words = (count + 1 + 3) // 4 + 32
                docc = rt.DeviceBuffer(ctx, occ_words * 4).upload(np.full(occ_words, GUARD, np.uint32))
                hits = a.HitBuffers(*[(bufs[k].handle.value + 64) if k in bufs else None for k in ("distance", "entityIndex", "normal")])
                rt.lib.check(lib.rtowTraceRaysIntervalDevice(ctx.handle, count, dev.handle.value + 4, div.handle.value + 4, C.byref(hits), None), "rtowTraceRaysIntervalDevice")
                rt.lib.check(lib.rtowTraceOcclusionDevice(ctx.handle, count, dev.handle.value + 4, div.handle.value + 4, docc.handle.value + 65, None), "rtowTraceOcclusionDevice")
                ctx.synchronize()
                for k, n in words.items():
                    if k == absent:
                        continue
                    raw = bufs[k].download(np.uint32, (n + 32,))
                    assert np.all(raw[:16] == GUARD) and np.all(raw[16 + n:] == GUARD), (count, absent, k)
                    assert np.array_equal(raw[16:16 + n], np.ascontiguousarray(full[k][:count]).reshape(-1).view(np.uint32)), (count, absent, k)
                raw = docc.download(np.uint8, (occ_words * 4,))
                want = np.full(occ_words, GUARD, np.uint32).view(np.uint8).copy()
                want[65:65 + count] = full_occ[:count]
                assert np.array_equal(raw, want), (count, absent)
                for b in list(bufs.values()) + [dev, div, docc]:
                    b.free()
