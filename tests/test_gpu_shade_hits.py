"""GPU: rtowShadeHitsDevice - the material of every first hit - against tests/shade_hits_reference.py (the numpy restatement of include/rtow.h's specification, anchored
without a GPU by tests/test_shade_hits_reference.py): every output of every element bit for bit on ten scenes and three skies, the view form against the sample path's
albedo AOV, the edges of the launch with guard words and odd offsets, defined results for inputs no trace call produces, stream order across a re-upload, and the
argument validation.  One GPU context at a time."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_hits_reference as ref  # noqa: E402
import test_gpu_trace_rays as tr  # noqa: E402  (its ray generators)

pytestmark = pytest.mark.gpu

GUARD = 0x5ca1ab1e
SCENES = ["cover", "moving", "mixed", "volumes", "textured", "textured_triangles", "mesh", "textured_mesh", "textured_volumes", "tiny"]
# the sky of each run: every scene under its own gradient, one under a non-square half-float cubemap, one without a sky
RUNS = [(name, "gradient", 0) for name in SCENES] + [("cover", "cubemap", 0), ("tiny", "none", 0), ("textured", "gradient", "wide")]


def _scene(rt, name):
    S = rt.scenes
    return {"cover": S.cover_scene, "moving": S.moving_scene, "mixed": S.mixed_scene, "volumes": S.volume_scene, "textured": S.textured_scene,
            "textured_triangles": lambda: S.textured_scene(triangles_only=True), "mesh": lambda: S.mesh_scene(1), "textured_mesh": lambda: S.textured_mesh_scene(1),
            "textured_volumes": S.textured_volume_scene, "tiny": S.tiny_scene}[name]()


def _environment(rt, scene, sky):
    a = rt.abi
    kind = {"gradient": a.SKY_GRADIENT, "cubemap": a.SKY_CUBEMAP, "none": a.SKY_NONE}[sky]
    return a.Environment(kind, a.Float3(*scene.sky_bottom), a.Float3(*scene.sky_top))


def _test_rays(rt, scene):
    pairs = list(tr._rays(scene, 2000, 11)) + list(tr._axis_rays(scene, 12))
    return tr._ray_array(rt, pairs, [0.0] * len(pairs))


def _assert_equal(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        bad = ~ref.same_bits(got[k], want[k])
        assert not bad.any(), (what, k, np.argwhere(bad)[:6].tolist(), got[k][bad][:6], want[k][bad][:6])


@pytest.mark.parametrize("name,sky,flags", RUNS, ids=["%s-%s%s" % (n, s, "-wide" if f else "") for n, s, f in RUNS])
def test_every_output_of_every_element_equals_the_restatement(rt, oracle, name, sky, flags):
    """1. albedo, emission, texCoord, metallicGlossiness, materialIndex and materialInfo of about 2 000 rays and the axis rays, entityIndex from rtowTraceRaysDevice:
    uint32 words equal the restatement's.  `mesh` and `textured_mesh` number their entities in leaf order (the entity -> primitive map is not the identity)."""
    scene = _scene(rt, name)
    desc = scene.desc()
    rays = _test_rays(rt, scene)
    env = _environment(rt, scene, sky)
    cubemap = rt.scenes.SkyCubemap.from_values(5, 3, 4, half=True, seed=503) if sky == "cubemap" else None
    with rt.Context(0, **({"flags": rt.abi.CONTEXT_FORCE_WIDE_CODES} if flags else {})) as ctx:
        ctx.upload_scene(desc)
        if cubemap is not None:
            ctx.upload_sky_cubemap(cubemap.desc())
        if flags:
            assert ctx.scene_info().wideCodes == 1
        ent = ctx.trace_rays(rays, want=("entityIndex",))["entityIndex"]
        got = ctx.shade_hits(rays, ent, env)
    hit = ent >= 0
    assert hit.sum() > 100 and (~hit).sum() > 20, (name, int(hit.sum()), int((~hit).sum()))
    want = ref.surface(oracle, scene, desc, rays, ent, env, cubemap)
    _assert_equal(got, want, (name, sky))
    assert np.all(got["materialIndex"][~hit] == -1) and np.all(got["materialInfo"][~hit] == 0xFFFFFFFF)
    for k in ("emission", "texCoord", "metallicGlossiness"):
        assert not got[k][~hit].view(np.uint32).any(), (name, k)                  # +0 on a miss
    assert np.array_equal(got["materialIndex"][hit], np.asarray(scene.material_index, np.int32)[ent[hit]])
    if sky == "cubemap" or (sky == "gradient" and tuple(scene.sky_bottom) != tuple(scene.sky_top)):
        assert len(np.unique(got["albedo"][~hit], axis=0)) > 10, name             # the sky varies with the direction
    elif sky == "none":
        assert not got["albedo"][~hit].view(np.uint32).any()
    if name.startswith("textured"):
        assert np.any(got["texCoord"][hit] != 0), name


@pytest.mark.parametrize("name", ["cover", "textured"])
def test_view_form_against_the_sample_paths_albedo(rt, oracle, name):
    """2. a 61 x 37 frame (not a multiple of the 8 x 8 tile): rtowTraceViewDevice -> rtowShadeHitsDevice against rtowSampleBatchDevice's albedo AOV (1 sample, jitter off,
    lens radius 0, white noise, trace depth 1, zeroed accumulators) on the comparable pixels of tests/test_shade_hits_reference.py, with its cap: emission + albedo at
    hits, the sky albedo on sky pixels, as uint32 words."""
    w, h = 61, 37
    scene = {"cover": rt.scenes.cover_scene, "textured": rt.scenes.textured_scene}[name]()
    p = rt.scenes.make_params(scene, w, h, spp=1, trace_depth=1, jitter=False, noise_color=rt.abi.NOISE_WHITE)
    p.view.lensRadius = 0.0
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        view = ctx.trace_view(p.view, w, h, want_rays=True, want=("entityIndex",))
        got = ctx.shade_hits(view["rays"], view["entityIndex"], p.environment)
        sample = rt.sample_batch_host(ctx, p, want_diag=False)
    ent = view["entityIndex"]
    keep = ref.comparable(scene, ent)
    print("%s: %d of %d pixels comparable, %d of them sky" % (name, keep.sum(), w * h, (keep & (ent < 0)).sum()))
    assert 2 * int((~keep).sum()) <= w * h, (name, int(keep.sum()))
    assert (keep & (ent >= 0)).sum() > w * h // 8 and (ent < 0).sum() > w * h // 16, name
    want = ref.expected_albedo_aov(got, ent)
    have = (np.float32(0) + sample["albedo"]).astype(np.float32)
    bad = ~ref.same_bits(have, want).all(axis=1) & keep
    assert not bad.any(), (name, np.flatnonzero(bad)[:8], have[bad][:4], want[bad][:4])


class _Guarded:
    """`words` uint32 words at an odd 4-byte offset inside an allocation filled with guard words"""
    LEAD, TAIL = 17, 15

    def __init__(self, rt, ctx, words, fill=None):
        self.words = words
        raw = np.full(self.LEAD + words + self.TAIL, GUARD, np.uint32)
        if fill is not None:
            raw[self.LEAD:self.LEAD + words] = np.ascontiguousarray(fill).reshape(-1).view(np.uint32)
        self.buf = rt.DeviceBuffer(ctx, raw.nbytes).upload(raw)
        self.ptr = self.buf.ptr + 4 * self.LEAD

    def check(self, expected=None):
        raw = self.buf.download(np.uint32, (self.LEAD + self.words + self.TAIL,))
        assert np.all(raw[:self.LEAD] == GUARD) and np.all(raw[self.LEAD + self.words:] == GUARD), "guard words overwritten"
        body = raw[self.LEAD:self.LEAD + self.words]
        if expected is None:
            assert np.all(body == GUARD), "written although nothing should be"
        return body


def test_edges_of_the_launch(rt, oracle):
    """3. counts 1, 255, 256, 257 and 0; each output on its own with the other five NULL; guard words before and after every buffer stay; rays, entityIndex and every output
    start at odd 4-byte offsets inside their allocations."""
    a = rt.abi
    lib = rt.lib.load()
    scene = _scene(rt, "textured")
    rays = _test_rays(rt, scene)[:257]
    env = _environment(rt, scene, "gradient")
    params = a.ShadeHitsParams(env, 0, 0)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        ent = ctx.trace_rays(rays, want=("entityIndex",))["entityIndex"]
        full = ctx.shade_hits(rays, ent, env)
        assert (ent >= 0).any() and (ent < 0).any()
        for count in (1, 255, 256, 257, 0):
            d_rays = _Guarded(rt, ctx, 8 * max(count, 1), rays[:max(count, 1)].view(np.uint32))
            d_ent = _Guarded(rt, ctx, max(count, 1), ent[:max(count, 1)])
            for only in list(a.SURFACE_OUTPUTS) + [None]:                          # None: all six at once
                names = list(a.SURFACE_OUTPUTS) if only is None else [only]
                outs = {k: _Guarded(rt, ctx, max(count, 1) * a.SURFACE_OUTPUTS[k][1]) for k in names}
                surface = a.SurfaceBuffers(*[outs[k].ptr if k in outs else None for k in a.SURFACE_OUTPUTS])
                rt.lib.check(lib.rtowShadeHitsDevice(ctx.handle, C.byref(params), count, d_rays.ptr, d_ent.ptr, C.byref(surface), None), "rtowShadeHitsDevice")
                ctx.synchronize()
                for k, g in outs.items():
                    if count == 0:
                        g.check(None)
                    else:
                        want = np.ascontiguousarray(full[k][:count]).reshape(-1).view(np.uint32)
                        assert np.array_equal(g.check(True), want), (count, only, k)
                    g.buf.free()
            d_rays.check(True)
            d_ent.check(True)
            d_rays.buf.free()
            d_ent.buf.free()
    _assert_equal(full, ref.surface(oracle, scene, scene.desc(), rays, ent, env), "textured, first 257 rays")


def _odd_scene(rt):
    """the textured scene plus a quad of the floor's image material whose texture coordinates run far outside [0, 1): the texel clamp applies"""
    s = rt.scenes.textured_scene()
    s.name = "textured + wide uv"
    rt.scenes._quad(s, (-2.6, 2.2, 1.0), (-1.0, 2.2, 1.0), (-1.0, 3.4, 1.0), (-2.6, 3.4, 1.0), 0, uv0=(-2.0, -1.5), uv1=(3.0, 2.5))
    return s


def test_defined_results_for_inputs_a_trace_would_not_produce(rt, oracle):
    """4. entityIndex -1, -2, entityCount, INT32_MAX, INT32_MIN (misses); a ray that misses the triangle it names (TexCoords (0, 0), that triangle's material at (0, 0));
    NaN, infinite and zero directions, as misses and naming a triangle; a material with a null image; texture coordinates far outside [0, 1).  All bit-exact."""
    scene = _odd_scene(rt)
    desc = scene.desc()
    n_ent = scene.entity_count
    tri = [e for e in range(n_ent) if scene.types[e] == rt.abi.ENTITY_TRIANGLE]
    wide_uv = tri[-2:]                                                             # the quad added last
    null_image = [e for e in tri if scene.materials[scene.material_index[e]].albedo.imageIndex < 0 and scene.materials[scene.material_index[e]].albedo.type == rt.abi.TEXTURE_IMAGE]
    assert len(wide_uv) == 2 and null_image
    cam = np.asarray(scene.camera["position"], np.float32)
    rng = np.random.default_rng(41)
    pairs = []
    for k in range(300):                                                           # towards the wide-uv quad, the null-image quad and the floor
        target = [(-2.6 + 1.6 * rng.random(), 2.2 + 1.2 * rng.random(), 1.0), (-2.2 + 1.2 * rng.random(), 0.01, 0.5 + 1.2 * rng.random()),
                  (-3 + 6 * rng.random(), 0.0, -3 + 6 * rng.random())][k % 3]
        pairs.append((cam, (np.asarray(target, np.float32) - cam).astype(np.float32)))
    traced_rays = tr._ray_array(rt, pairs, [0.0] * len(pairs))
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    odd_dirs = [(nan, 0, -1), (0, nan, -1), (nan, nan, nan), (inf, 0, 0), (0, inf, 0), (0, -inf, 0), (inf, -inf, inf), (0, 0, 0), (-0.0, 0, -0.0), (1e38, -1e38, 1e38)]
    with rt.Context(0) as ctx:
        ctx.upload_scene(desc)
        traced_ent = ctx.trace_rays(traced_rays, want=("entityIndex",))["entityIndex"]
        assert np.isin(wide_uv, traced_ent).all() and np.isin(null_image, traced_ent).any() and (traced_ent == 0).any() | (traced_ent == 1).any()
        # misnamed: every traced ray names the NEXT triangle instead of the one it hits, or an index that is no entity
        rays = [traced_rays, traced_rays.copy(), traced_rays[:50].copy()]
        ents = [traced_ent, np.asarray([tri[(tri.index(e) + 1) % len(tri)] if e in tri else tri[0] for e in traced_ent], np.int32),
                np.resize(np.asarray([-1, -2, n_ent, 2**31 - 1, -2**31, n_ent + 1, 65536, -65536], np.int64), 50).astype(np.int32)]
        for as_entity in (-1, tri[0], wide_uv[0], null_image[0]):
            r = tr._ray_array(rt, [(cam, np.asarray(d, np.float32)) for d in odd_dirs], [0.0] * len(odd_dirs))
            rays.append(r)
            ents.append(np.full(len(odd_dirs), as_entity, np.int32))
        rays, ents = np.concatenate(rays), np.concatenate(ents)
        env = _environment(rt, scene, "gradient")
        got = ctx.shade_hits(rays, ents, env)
    want = ref.surface(oracle, scene, desc, rays, ents, env)
    _assert_equal(got, want, "odd inputs")
    n = len(traced_rays)
    uv = got["texCoord"][:n][np.isin(traced_ent, wide_uv)]
    assert (uv.max() > 2.0) and (uv.min() < -1.0), (uv.min(), uv.max())           # far outside [0, 1): texels come from the image's border rows and columns
    assert not got["albedo"][:n][np.isin(traced_ent, null_image)].view(np.uint32).any()           # null image: 0
    misnamed = slice(n, 2 * n)
    zero_uv = ~got["texCoord"][misnamed].view(np.uint32).any(axis=1)              # (a few rays do meet the triangle they name instead: one behind the surface they hit)
    assert zero_uv.sum() > n // 2, int(zero_uv.sum())
    assert np.array_equal(got["materialIndex"][misnamed], np.asarray(scene.material_index, np.int32)[ents[misnamed]])
    assert np.all(got["materialIndex"][2 * n:2 * n + 50] == -1)


def test_stream_order_across_a_reupload(rt, oracle):
    """5. on a caller's stream: rtowTraceViewDevice and rtowShadeHitsDevice back to back with no synchronisation between them, a re-upload of another scene, the same
    pair again: each result matches its own scene's restatement."""
    a = rt.abi
    lib = rt.lib.load()
    w, h = 24, 16
    n = w * h
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    with rt.Context(0) as ctx:
        side = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(side)) == 0
        try:
            results = []
            for name in ("textured", "mixed"):
                scene = _scene(rt, name)
                desc = scene.desc()
                ctx.upload_scene(desc)
                view = rt.scenes.make_view(scene, w, h)
                env = _environment(rt, scene, "gradient")
                d_rays, d_ent = rt.DeviceBuffer(ctx, n * 32).zero(), rt.DeviceBuffer(ctx, n * 4).zero()
                outs = {k: rt.DeviceBuffer(ctx, n * 4 * a.SURFACE_OUTPUTS[k][1]).zero() for k in a.SURFACE_OUTPUTS}
                ctx.synchronize()
                vp = a.TraceViewParams(w, h, view, 0.0, 0)
                hits = a.HitBuffers(None, d_ent.ptr, None)
                rt.lib.check(lib.rtowTraceViewDevice(ctx.handle, C.byref(vp), C.byref(hits), d_rays.handle, side), "rtowTraceViewDevice")
                job = rt.ShadeHitsJob(ctx, n, env)
                job.Rays, job.EntityIndex = d_rays, d_ent
                job.Albedo, job.Emission, job.TexCoord, job.MetallicGlossiness, job.MaterialIndex, job.MaterialInfo = [outs[k] for k in a.SURFACE_OUTPUTS]
                assert job.Schedule(side).Complete() == 0
                results.append((name, scene, desc, env, d_rays, d_ent, outs))
            assert hip.hipStreamSynchronize(side) == 0
            for name, scene, desc, env, d_rays, d_ent, outs in results:
                rays = d_rays.download(np.dtype(a.RAY_DTYPE), (n,))
                ent = d_ent.download(np.int32, (n,))
                got = {k: outs[k].download(np.dtype(a.SURFACE_OUTPUTS[k][0]), (n, a.SURFACE_OUTPUTS[k][1]) if a.SURFACE_OUTPUTS[k][1] > 1 else (n,)) for k in outs}
                assert (ent >= 0).sum() > n // 4, name
                _assert_equal(got, ref.surface(oracle, scene, desc, rays, ent, env), name)
                for b in [d_rays, d_ent] + list(outs.values()):
                    b.free()
        finally:
            hip.hipStreamDestroy(side)


def test_validation_leaves_the_outputs_untouched(rt):
    """6. RTOW_ERROR_NO_SCENE before the first upload; every RTOW_ERROR_INVALID_VALUE case with a real context; none of them writes a word of the guarded outputs."""
    a = rt.abi
    lib = rt.lib.load()
    bad = a.RTOW_ERROR_INVALID_VALUE
    scene = _scene(rt, "tiny")
    rays = _test_rays(rt, scene)[:64]
    with rt.Context(0) as ctx:
        outs = {k: _Guarded(rt, ctx, 64 * a.SURFACE_OUTPUTS[k][1]) for k in a.SURFACE_OUTPUTS}
        surface = a.SurfaceBuffers(*[outs[k].ptr for k in a.SURFACE_OUTPUTS])
        none = a.SurfaceBuffers(None, None, None, None, None, None)
        d_rays = rt.DeviceBuffer(ctx, 64 * 32).upload(rays)
        d_ent = rt.DeviceBuffer(ctx, 64 * 4).zero()
        env = _environment(rt, scene, "gradient")
        ok = a.ShadeHitsParams(env, 0, 0)
        call = lambda p=ok, count=64, r=d_rays.handle, e=d_ent.handle, s=surface, c=ctx.handle: \
            lib.rtowShadeHitsDevice(c, C.byref(p) if p is not None else None, count, r, e, C.byref(s) if s is not None else None, None)
        assert call() == a.RTOW_ERROR_NO_SCENE
        assert call(count=0) == a.RTOW_ERROR_NO_SCENE
        ctx.upload_scene(scene.desc())
        assert call(c=None) == bad and call(p=None) == bad and call(r=None) == bad and call(e=None) == bad and call(s=None) == bad
        assert call(s=none) == bad
        assert call(count=-1) == bad and call(count=-2**31) == bad
        assert call(p=a.ShadeHitsParams(env, 1, 0)) == bad and call(p=a.ShadeHitsParams(env, 0, 1)) == bad and call(p=a.ShadeHitsParams(env, -1, 0)) == bad
        for sky in (3, -1, 255):
            assert call(p=a.ShadeHitsParams(a.Environment(sky, a.Float3(1, 1, 1), a.Float3(0, 0, 1)), 0, 0)) == bad, sky
        assert call(count=0) == 0
        ctx.synchronize()
        for g in outs.values():
            g.check(None)
        assert call() == 0                                                        # and the valid call does write
        ctx.synchronize()
        assert not np.all(outs["materialIndex"].check(True) == GUARD)
