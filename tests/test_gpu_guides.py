"""GPU: rtowTraceGuideRaysDevice / rtowTraceGuideViewDevice - the end of every ray's specular chain - against tests/guides_reference.py (the numpy restatement of
include/rtow.h's specification, anchored without a GPU by tests/test_guides_reference.py): every output of every ray bit for bit on eight scenes, the view form end to end
against the sample kernel's own albedo and normal AOVs with no reference in the loop, the degenerate forms against rtowTraceRaysDevice, the edges of the launch with guard
words and odd offsets, stream order across a re-upload, the argument validation, and what the chain's guides are worth to the denoiser.  One GPU context at a time."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guides_reference as ref  # noqa: E402
from guides_quality import guide_quality  # noqa: E402
import shade_hits_reference as shade  # noqa: E402
import test_gpu_trace_rays as tr  # noqa: E402  (its ray generators)
from test_gpu_shade_hits import _Guarded, GUARD  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
# (scene, rays taken from the generators (None: all), context flags)
RUNS = [("cover", None, 0), ("tiny", None, 0), ("mixed", None, 0), ("twin_row", None, 0), ("textured", None, 0), ("textured_mirror", None, 0), ("volumes", None, 0),
        ("cover", None, "wide"), ("mesh", 300, 0)]


def _scene(rt, name):
    S = rt.scenes
    return {"cover": S.cover_scene, "tiny": S.tiny_scene, "mixed": S.mixed_scene, "twin_row": S.twin_row_scene, "textured": S.textured_scene, "volumes": S.volume_scene,
            "mesh": lambda: S.mesh_scene(3), "mirrors": lambda: ref.mirror_scene(rt), "textured_mirror": lambda: ref.textured_mirror_scene(rt)}[name]()


def _test_rays(rt, scene, name, take=None):
    """about 1 500 generated rays and the axis rays of tests/test_gpu_trace_rays.py; `mixed` (moving entities): every other ray at a random time"""
    pairs = list(tr._rays(scene, 1500, 11)) + list(tr._axis_rays(scene, 12))
    draws = np.random.default_rng(3).random(len(pairs)).astype(F)
    times = [float(draws[k]) if (name == "mixed" and k % 2) else 0.0 for k in range(len(pairs))]
    return tr._ray_array(rt, pairs, times)[:take]


def _assert_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].dtype, want[k].shape)
        if k == "rays":
            g, w = got[k].view(F).reshape(-1, 8), want[k].view(F).reshape(-1, 8)
        else:
            g, w = got[k], want[k]
        bad = ~shade.same_bits(g, w) if g.dtype == F else (g != w)
        assert not bad.any(), (what, k, np.argwhere(bad)[:6].tolist(), g[bad][:6], w[bad][:6])


@pytest.mark.parametrize("name,take,flags", RUNS, ids=["%s%s" % (n, "-wide" if f else "") for n, _, f in RUNS])
def test_every_output_of_every_ray_equals_the_restatement(rt, oracle, name, take, flags):
    """1. hits, rays, throughput, pathDistance, bounces and end of about 1 600 rays (mesh: 300, the restatement is a loop) at maxBounces 8: uint32 words equal the
    restatement's.  Not vacuous: chains that end in the sky, on a surface, and chains that followed a surface all occur; on `tiny` (a hollow glass ball) a dielectric
    reflects totally; on `textured_mirror` (the textured scene plus a mirror with an Image albedo) the throughput takes the values of many texels."""
    scene = _scene(rt, name)
    desc = scene.desc()
    rays = _test_rays(rt, scene, name, take)
    with rt.Context(0, **({"flags": rt.abi.CONTEXT_FORCE_WIDE_CODES} if flags else {})) as ctx:
        ctx.upload_scene(desc)
        if flags:
            assert ctx.scene_info().wideCodes == 1
        got = ctx.trace_guide_rays(rays, 8)
    want, reflections = ref.guides(oracle, scene, desc, rays, 8)
    print("%s: end %s, bounces %s, dielectric reflections %d" % (name, np.bincount(want["end"], minlength=3).tolist(), np.bincount(want["bounces"]).tolist(), reflections))
    assert (want["end"] == ref.END_SKY).any() and (want["end"] == ref.END_SURFACE).any() and (want["bounces"] >= 1).any(), name
    if name == "tiny":
        assert reflections >= 1
    if name == "textured_mirror":                                                  # the tint comes from many different texels of the mirror's image
        followed = want["throughput"][want["bounces"] >= 1]
        assert len(np.unique(followed.view(np.uint32), axis=0)) > 20 and np.any(followed[:, 0] != followed[:, 1]), len(followed)
    _assert_equal(got, want, name)


def _mirror_frame(rt, ctx, w, h, max_bounces):
    scene = ref.mirror_scene(rt)
    p = ref.mirror_params(rt, scene, w, h)
    ctx.upload_scene(scene.desc())
    return scene, p, ctx.trace_guide_view(p.view, w, h, max_bounces)


def test_view_form_end_to_end_against_the_sample_kernel(rt):
    """2. the mirror scene at 61 x 37 (not a multiple of the 8 x 8 tile), no reference in the loop: rtowTraceGuideViewDevice(maxBounces 8) -> rtowShadeHitsDevice on its rays
    and entityIndex, against rtowSampleBatchDevice's albedo and normal AOVs (1 spp, jitter off, lens 0, white noise, traceDepth 9, zeroed accumulators) on every pixel, as
    uint32 words; no chain of this frame is cut at 8.  At maxBounces 1 the cut pixels are exactly those whose chain is longer than 1, and they report the second mirror."""
    w, h = 61, 37
    with rt.Context(0) as ctx:
        scene, p, got = _mirror_frame(rt, ctx, w, h, 8)
        surface = ctx.shade_hits(got["rays"], got["entityIndex"], p.environment, outputs=("albedo", "emission"))
        sample = rt.sample_batch_host(ctx, p, want_diag=False)
        cut = ctx.trace_guide_view(p.view, w, h, 1)
        second = ctx.trace_rays(cut["rays"])
    assert not (got["end"] == ref.END_CUT).any(), np.bincount(got["end"]).tolist()
    print("bounces:", np.bincount(got["bounces"]).tolist(), "end:", np.bincount(got["end"]).tolist())
    assert got["bounces"].max() >= 3 and (got["bounces"] >= 1).sum() > w * h // 10 and (got["end"] == ref.END_SKY).any()
    albedo, normal = ref.expected_aovs(scene, p.environment, got["rays"], got["entityIndex"], got["normal"], surface)
    have_albedo, have_normal = (F(0) + sample["albedo"]).astype(F), (F(0) + sample["normal"]).astype(F)
    bad = ~(shade.same_bits(have_albedo, albedo).all(axis=1) & shade.same_bits(have_normal, normal).all(axis=1))
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8], have_albedo[bad][:3], albedo[bad][:3], have_normal[bad][:3], normal[bad][:3])
    longer = got["bounces"] > 1
    assert longer.sum() > 10 and np.array_equal((cut["bounces"] == 1) & (cut["end"] == ref.END_CUT), longer)
    assert np.all(cut["end"][~longer] == got["end"][~longer]) and np.all(cut["bounces"][~longer] == got["bounces"][~longer])
    specular = np.asarray([shade.is_perfect_specular(m) for m in scene.materials])[np.asarray(scene.material_index)]
    assert np.all(specular[cut["entityIndex"][longer]])                            # the surface the cut chain stands on is the second mirror ...
    for k in ("distance", "entityIndex", "normal"):                                # ... as rtowTraceRaysDevice reports it for the chain's last ray
        assert np.array_equal(np.ascontiguousarray(cut[k]).view(np.uint32), np.ascontiguousarray(second[k]).view(np.uint32)), k


def _assert_is_the_plain_trace(rt, ctx, rays, max_bounces, what):
    plain = ctx.trace_rays(rays)
    got = ctx.trace_guide_rays(rays, max_bounces)
    for k in ("distance", "entityIndex", "normal"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(plain[k]).view(np.uint32)), (what, k)
    want_rays = rays.copy()
    want_rays["pad"] = 0
    assert np.array_equal(got["rays"].view(np.uint32), want_rays.view(np.uint32)), what
    assert np.all(got["throughput"] == 1) and not got["bounces"].any(), what
    hit = plain["entityIndex"] >= 0
    assert hit.sum() > 100 and (~hit).sum() > 20, what
    assert np.array_equal(got["pathDistance"][hit].view(np.uint32), plain["distance"][hit].view(np.uint32)) and not got["pathDistance"][~hit].view(np.uint32).any(), what
    return got, hit


@pytest.mark.parametrize("name", ["cover", "mixed"])
def test_max_bounces_zero_is_the_plain_trace(rt, name):
    """3a. maxBounces 0: hits bit for bit rtowTraceRaysDevice's, rays out == in with pad 0, throughput 1, bounces 0, pathDistance = the distance (+0 on a miss);
    end = 2 exactly on the perfectly specular first hits."""
    scene = _scene(rt, name)
    rays = _test_rays(rt, scene, name)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        got, hit = _assert_is_the_plain_trace(rt, ctx, rays, 0, name)
        info = ctx.shade_hits(rays, got["entityIndex"], outputs=("materialInfo",))["materialInfo"]
    specular = hit & ((info & rt.abi.MATERIAL_INFO_PERFECT_SPECULAR) != 0)
    assert specular.any() and np.array_equal(got["end"], np.where(hit, np.where(specular, 2, 1), 0).astype(np.uint8)), name


def test_a_scene_without_specular_materials_is_the_plain_trace_at_any_depth(rt):
    """3b. lambert spheres only, maxBounces 64"""
    S = rt.scenes
    scene = S.Scene("lambert")
    rng = np.random.default_rng(8)
    scene.add_sphere((0, -1000, 0), 1000, S.lambertian((0.5, 0.5, 0.5)))
    for _ in range(40):
        scene.add_sphere((rng.uniform(-4, 4), rng.uniform(0.2, 2), rng.uniform(-4, 4)), rng.uniform(0.2, 0.6), S.lambertian(tuple(rng.uniform(0.1, 0.9, 3))))
    scene.camera = {"position": [3.0, 2.0, 9.0], "target": [0.0, 0.5, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    rays = _test_rays(rt, scene, "lambert")
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        got, hit = _assert_is_the_plain_trace(rt, ctx, rays, 64, "lambert")
    assert np.array_equal(got["end"], hit.astype(np.uint8))


@pytest.mark.parametrize("size", [(9, 7), (61, 37)])
def test_view_form_equals_the_ray_form_on_the_views_rays(rt, size):
    """3c. rtowTraceGuideViewDevice == rtowTraceGuideRaysDevice fed with rtowTraceViewDevice's outRays, every output"""
    w, h = size
    scene = _scene(rt, "cover")
    view = rt.scenes.make_view(scene, w, h)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        first = ctx.trace_view(view, w, h, time=0.25, want_rays=True, want=("entityIndex",))
        by_view = ctx.trace_guide_view(view, w, h, 8, time=0.25)
        by_rays = ctx.trace_guide_rays(first["rays"], 8)
    assert (by_view["bounces"] >= 1).any()
    _assert_equal(by_view, by_rays, size)


def _outputs(a, count):
    """words of every output for `count` elements (`end`: bytes, rounded up to words for the guard)"""
    return {k: (count * np.dtype(d).itemsize * wd + 3) // 4 for k, (d, wd) in a.GUIDE_OUTPUTS.items()}


def _as_bytes(x):
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def test_edges_of_the_launch(rt):
    """4. counts 0, 1, 255, 256, 257; each output alone with the others NULL, and all at once; guard words before and after every buffer; rays and outputs at odd 4-byte
    offsets, `end` at an odd address; the input rays aliasing out->rays; NaN / inf / zero directions end as rtowTraceRaysDevice ends them and write nothing else."""
    a = rt.abi
    lib = rt.lib.load()
    scene = _scene(rt, "tiny")
    rays = _test_rays(rt, scene, "tiny")[:257].copy()
    nan, inf = F(np.nan), F(np.inf)
    odd = [(nan, 0, -1), (0, nan, -1), (nan, nan, nan), (inf, 0, 0), (0, -inf, 0), (inf, -inf, inf), (0, 0, 0), (-0.0, 0, -0.0)]
    rays["direction"][100:100 + len(odd)] = np.asarray(odd, F)
    params = a.GuideParams(8, 0, 0)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        full = ctx.trace_guide_rays(rays, 8)
        plain = ctx.trace_rays(rays)
        assert (full["bounces"] >= 1).any() and (full["end"] == 0).any() and (full["end"] == 1).any()
        strange = slice(100, 100 + len(odd))
        assert (plain["entityIndex"][strange] < 0).all() and not full["end"][strange].any() and not full["bounces"][strange].any()
        for name in ("distance", "entityIndex", "normal"):
            assert np.array_equal(_as_bytes(full[name][strange]), _as_bytes(plain[name][strange])), name
        for count in (0, 1, 255, 256, 257):
            m = max(count, 1)
            for only in list(a.GUIDE_OUTPUTS) + [None, "alias"]:                  # None: all at once; "alias": all at once, out->rays = the input
                names = list(a.GUIDE_OUTPUTS) if only in (None, "alias") else [only]
                d_rays = _Guarded(rt, ctx, 8 * m, rays[:m].view(np.uint32))
                outs = {k: _Guarded(rt, ctx, _outputs(a, m)[k] + (1 if k == "end" else 0)) for k in names if not (only == "alias" and k == "rays")}
                at = {k: g.ptr + (1 if k == "end" else 0) for k, g in outs.items()}            # `end` at an odd address
                if only == "alias":
                    at["rays"] = d_rays.ptr
                buffers = a.guide_buffers(at)
                rt.lib.check(lib.rtowTraceGuideRaysDevice(ctx.handle, C.byref(params), count, d_rays.ptr, C.byref(buffers), None), "rtowTraceGuideRaysDevice")
                ctx.synchronize()
                for k, g in outs.items():
                    if count == 0:
                        g.check(None)
                    else:
                        pattern = np.tile(np.frombuffer(np.uint32(GUARD).tobytes(), np.uint8), g.words)
                        lead = 1 if k == "end" else 0
                        want = _as_bytes(full[k][:count])
                        pattern[lead:lead + want.size] = want                      # the elements, and the guard pattern in every other byte of the allocation's body
                        assert np.array_equal(g.check(True).view(np.uint8), pattern), (count, only, k)
                    g.buf.free()
                body = d_rays.check(True)
                if only == "alias" and count:
                    assert np.array_equal(body[:8 * count].view(np.uint8), _as_bytes(full["rays"][:count])), count
                else:
                    assert np.array_equal(body, rays[:m].view(np.uint32).reshape(-1)), (count, only)
                d_rays.buf.free()


def test_stream_order_across_a_reupload(rt, oracle):
    """5. on a caller's stream: rtowTraceGuideViewDevice and rtowShadeHitsDevice back to back with no synchronisation between them, a re-upload of another scene, the same
    pair again: each result matches its own scene's restatement."""
    a = rt.abi
    lib = rt.lib.load()
    w, h = 24, 16
    n = w * h
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    shape = lambda k: (np.dtype(a.GUIDE_OUTPUTS[k][0]), (n, a.GUIDE_OUTPUTS[k][1]) if a.GUIDE_OUTPUTS[k][1] > 1 else (n,))
    with rt.Context(0) as ctx:
        side = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(side)) == 0
        try:
            results = []
            for name in ("tiny", "mirrors"):
                scene = _scene(rt, name)
                desc = scene.desc()
                ctx.upload_scene(desc)
                view = rt.scenes.make_view(scene, w, h)
                env = a.Environment(a.SKY_GRADIENT, a.Float3(*scene.sky_bottom), a.Float3(*scene.sky_top))
                outs = {k: rt.DeviceBuffer(ctx, n * shape(k)[0].itemsize * a.GUIDE_OUTPUTS[k][1]).zero() for k in a.GUIDE_OUTPUTS}
                albedo = rt.DeviceBuffer(ctx, n * 12).zero()
                ctx.synchronize()
                gp = a.GuideParams(8, 0, 0)
                vp = a.TraceViewParams(w, h, view, 0.0, 0)
                buffers = a.guide_buffers({k: b.ptr for k, b in outs.items()})
                rt.lib.check(lib.rtowTraceGuideViewDevice(ctx.handle, C.byref(gp), C.byref(vp), C.byref(buffers), side), "rtowTraceGuideViewDevice")
                job = rt.ShadeHitsJob(ctx, n, env)
                job.Rays, job.EntityIndex, job.Albedo = outs["rays"], outs["entityIndex"], albedo
                assert job.Schedule(side).Complete() == 0
                results.append((name, scene, desc, env, view, outs, albedo))
            assert hip.hipStreamSynchronize(side) == 0
            for name, scene, desc, env, view, outs, albedo in results:
                got = {k: outs[k].download(*shape(k)) for k in outs}
                want, _ = ref.guides(oracle, scene, desc, shade.view_rays(view, w, h), 8)
                assert (want["bounces"] >= 1).sum() > n // 50, name
                _assert_equal(got, want, name)
                surface = shade.surface(oracle, scene, desc, want["rays"], want["entityIndex"], env)
                assert shade.same_bits(albedo.download(F, (n, 3)), surface["albedo"]).all(), name
                for b in list(outs.values()) + [albedo]:
                    b.free()
        finally:
            hip.hipStreamDestroy(side)


def test_validation_leaves_the_outputs_untouched(rt):
    """6. RTOW_ERROR_NO_SCENE before the first upload; every RTOW_ERROR_INVALID_VALUE case of both calls with a real context; none of them writes a word of the guarded
    outputs; count == 0 succeeds and writes nothing."""
    a = rt.abi
    lib = rt.lib.load()
    bad = a.RTOW_ERROR_INVALID_VALUE
    scene = _scene(rt, "tiny")
    rays = _test_rays(rt, scene, "tiny")[:64]
    with rt.Context(0) as ctx:
        outs = {k: _Guarded(rt, ctx, _outputs(a, 64)[k]) for k in a.GUIDE_OUTPUTS}
        out = a.guide_buffers({k: g.ptr for k, g in outs.items()})
        none = a.guide_buffers({})
        d_rays = rt.DeviceBuffer(ctx, 64 * 32).upload(rays)
        ok = a.GuideParams(8, 0, 0)
        view = a.TraceViewParams(8, 8, rt.scenes.make_view(scene, 8, 8), 0.0, 0)
        ref_ = lambda x: C.byref(x) if x is not None else None
        by_rays = lambda p=ok, count=64, r=d_rays.handle, o=out, c=ctx.handle: lib.rtowTraceGuideRaysDevice(c, ref_(p), count, r, ref_(o), None)
        by_view = lambda p=ok, v=view, o=out, c=ctx.handle: lib.rtowTraceGuideViewDevice(c, ref_(p), ref_(v), ref_(o), None)
        assert by_rays() == a.RTOW_ERROR_NO_SCENE and by_rays(count=0) == a.RTOW_ERROR_NO_SCENE and by_view() == a.RTOW_ERROR_NO_SCENE
        ctx.upload_scene(scene.desc())
        for call in (by_rays, by_view):
            assert call(c=None) == bad and call(p=None) == bad and call(o=None) == bad and call(o=none) == bad
            for p in (a.GuideParams(-1, 0, 0), a.GuideParams(65, 0, 0), a.GuideParams(-2**31, 0, 0), a.GuideParams(8, 1, 0), a.GuideParams(8, 0, 1), a.GuideParams(8, -1, 0)):
                assert call(p=p) == bad, (p.maxBounces, p.flags, p.reserved)
        assert by_rays(r=None) == bad and by_rays(count=-1) == bad and by_rays(count=-2**31) == bad
        assert by_view(v=None) == bad
        for v in (a.TraceViewParams(0, 8, view.view, 0.0, 0), a.TraceViewParams(8, -1, view.view, 0.0, 0), a.TraceViewParams(65536, 32768, view.view, 0.0, 0),
                  a.TraceViewParams(8, 8, view.view, 0.0, 1)):
            assert by_view(v=v) == bad
        assert by_rays(count=0) == 0
        ctx.synchronize()
        for g in outs.values():
            g.check(None)
        assert by_rays(p=a.GuideParams(64, 0, 0)) == 0 and by_view(p=a.GuideParams(0, 0, 0)) == 0                # and the valid calls, at both ends of maxBounces, do write
        ctx.synchronize()
        assert not np.all(outs["bounces"].check(True) == GUARD)


def test_chain_guides_denoise_no_worse_than_first_hit_guides(rt):
    """7. the quality run at the size tests/test_gpu_denoise.py uses (192 x 108): the chain-guided whole-frame error is at most 1.05 x the first-hit-guided error of the
    same frame.  The margin is for the seed-to-seed spread of the ratio (profiles/r11_guides.json records it over three seeds)."""
    with rt.Context(0) as ctx:
        q = guide_quality(rt, ctx, 192, 108, 1)
    print("denoised / noisy, whole frame and on specular first hits:", {k: q[k] for k in ("combine_guides", "first_hit_guides", "chain_guides")})
    assert q["perfect_specular_first_hit_share"] > 0.1 and q["mean_bounces"] > 0.1
    assert q["chain_guides"]["whole_frame_over_noisy"] <= 1.05 * q["first_hit_guides"]["whole_frame_over_noisy"], q
