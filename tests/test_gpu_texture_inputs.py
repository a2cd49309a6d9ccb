"""GPU: the data a host hands over through rtowUploadSkyCubemap, rtowUploadBlueNoise and rtowUploadStbNoise, at the layouts and values that the helpers of
scenes.py never produce - faces that are not square, every kind of pixel stride, all 65 536 half bit patterns, sky directions on the exact ties between two and
three axes and on the face border, noise sets whose row stride is no power of two and whose texels sit on the ends of their domain - against the oracle bit for
bit and, for the cubemap, against the whole-array numpy evaluation of tests/cubemap_numpy.py (pinned to the oracle on the CPU by tests/test_cubemap_oracle.py).

The cubemap tests make a frame a table of sky lookups: the camera sits at (1000, 0, 0), the only entity is a sphere of radius 1e-3 at the world origin (no ray of
the views below passes within 1/128 rad of it: every pixel is a miss), traceDepth 1, one sample, jitter off, lensRadius 0, white noise, zeroed accumulators.  Then
color.xyz of a pixel is 0 + Cubemap.Sample(its direction) and color.w is 1.  The views are written straight into RtowView with dyadic values, so that every
component of lowerLeftCorner + u * horizontal + v * vertical is exact and components that are equal before normalize() stay equal after it (the same factor):
  face views  128 x 128: component `axis` is +-1, the other two are -1 + 2u and -1 + 2v: one whole face, no ties;
  tie views     8 x 8:   component `axis` is +-5/8, the other two take +-1/8, +-3/8, +-5/8, +-7/8: rows and columns at +-5/8 tie with the constant axis, the four
                         corners are triple ties, and every tied pixel has u or v at exactly +-1, where min(coords, faceSizeMinusOne) clamps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cubemap_numpy as cn  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("color", "normal", "albedo", "scw")
FACE_VIEW, TIE_VIEW = 128, 8


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _lookup_scene(rt):
    S = rt.scenes
    sc = S.Scene("sky lookups")
    sc.add_sphere((0, 0, 0), 1e-3, S.lambertian((0.5, 0.5, 0.5)))
    sc.camera = {"position": [1000, 0, 0], "target": [0, 0, 0], "up": [0, 1, 0], "vfov": 60.0, "aperture": 0.0}
    return sc


def _params(rt, scene, axis, sign, constant, size, seed=1):
    a = rt.abi
    p = rt.scenes.make_params(scene, size, size, spp=1, trace_depth=1, seed=seed, jitter=False, focus=1.0, sky_type=a.SKY_CUBEMAP, noise_color=a.NOISE_WHITE)
    free = [k for k in range(3) if k != axis]
    llc, hor, ver = [-1.0] * 3, [0.0] * 3, [0.0] * 3
    llc[axis] = sign * constant
    hor[free[0]], ver[free[1]] = 2.0, 2.0
    p.view = a.View(a.Float3(1000, 0, 0), a.Float3(*llc), a.Float3(*hor), a.Float3(*ver), a.Float3(0, 0, 1), a.Float3(0, 1, 0), a.Float3(1, 0, 0), 0.0)
    return p


class _Harness:
    """The lookup scene on the device and in the oracle, the twelve views, and the ray directions of each (rtowTraceViewDevice's outRays), computed once."""

    def __init__(self, rt, oracle, ctx):
        self.rt, self.ctx = rt, ctx
        self.scene = _lookup_scene(rt)
        self.desc = self.scene.desc()
        self.osc = oracle.OracleScene(self.desc)
        ctx.upload_scene(self.desc)
        self.views = []                                        # (kind, face, params, directions)
        for kind, constant, size in (("face", 1.0, FACE_VIEW), ("tie", 0.625, TIE_VIEW)):
            for axis in range(3):
                for sign in (1.0, -1.0):
                    p = _params(rt, self.scene, axis, sign, constant, size)
                    got = ctx.trace_view(p.view, size, size, want_rays=True)
                    assert np.all(got["entityIndex"] == -1), (kind, axis, sign)
                    self.views.append((kind, axis * 2 + (0 if sign > 0 else 1), p, got["rays"]["direction"].copy()))

    def set_cubemap(self, desc):
        self.ctx.upload_sky_cubemap(desc)
        self.osc.set_cubemap(desc)

    def both(self, p):
        """One batch from zeroed accumulators on the device and in the oracle: equal bit for bit (NaN for NaN), every pixel one ray that missed."""
        gpu, ref = self.rt.sample_batch_host(self.ctx, p), self.osc.sample_batch(p)
        assert np.all(ref["color"][:, 3] == 1) and np.all(ref["diag"][:, 0] == 1)          # a hit at traceDepth 1 is a failed sample: w == 0
        _equal(gpu, ref)
        return gpu, ref


def _equal(gpu, ref):
    for k in KEYS:
        g, r = gpu[k].reshape(-1), ref[k].reshape(-1)
        nan = np.isnan(r)
        assert np.all(np.isnan(g[nan])), k
        bad = np.flatnonzero((_u32(g) != _u32(r)) & ~nan)
        assert bad.size == 0, (k, bad[:8], g[bad[:8]], r[bad[:8]])
    assert np.array_equal(gpu["diag"][:, 0], ref["diag"][:, 0]), "RayCount differs"


@pytest.fixture(scope="module")
def lookups(rt, oracle, gpu_context):
    h = _Harness(rt, oracle, gpu_context)
    yield h
    gpu_context.upload_sky_cubemap(None)
    h.osc.close()


def _check_views(h, sky, kinds=("face", "tie")):
    """Every view of `kinds` under the cubemap that is set: device == oracle, the sample path's directions are the view form's, color.xyz == 0 + the texel that the
    numpy evaluation names for that direction; returns which texels the face views and the tie views read."""
    _, fh, fw, _ = sky.faces.shape
    reached = {"face": np.zeros((6, fh, fw), bool), "tie": np.zeros((6, fh, fw), bool)}
    for kind, face_of_view, p, dirs in h.views:
        if kind not in kinds:
            continue
        gpu, ref = h.both(p)
        # sampleNormal = -ray.Direction of a miss: the sample path normalises the direction that rtowTraceViewDevice wrote out
        assert np.array_equal(_u32(ref["normal"]), _u32(np.float32(0) + -dirs)), (kind, face_of_view)
        face, cx, cy = cn.lookup(dirs, fw, fh)
        if kind == "face":
            assert np.all(face == face_of_view)
        reached[kind][face, cy, cx] = True
        with np.errstate(invalid="ignore"):                                                 # signalling NaN texels
            want = np.float32(0) + cn.decode(sky.faces, face, cx, cy)
        nan = np.isnan(want)
        for got in (gpu["color"][:, :3], gpu["albedo"]):                                   # the sky colour is also the albedo of a pixel that met nothing
            assert np.all(np.isnan(got[nan])) and np.array_equal(_u32(got)[~nan], _u32(want)[~nan]), (kind, face_of_view)
        assert np.all(gpu["color"][:, 3] == 1)
    return reached


@pytest.mark.parametrize("layout", cn.LAYOUTS, ids=cn.layout_id)
def test_cubemap_layouts(lookups, layout):
    """Faces that are not square at pixel strides 6, 8 and 16 (halves) and 3, 4 and 5 (bytes), the channels after b holding values that no r, g or b holds, under
    the six face views and the six tie views.

    Coverage.  A face view reads every texel of its face that a direction off the face's border can address: columns 0 .. 2 * (W / 2) - 1, that is all of them for an
    even W.  Column W - 1 of an odd W is (int)((u + 1) * (W / 2)) == W - 1, u == 1 exactly (likewise the rows, and the only texel of a width of 1 is read by
    everything).  u == +-1 is a tie of two axes, which the first axis wins: the +-X faces have such columns and rows, the +-Y faces such rows (|z| == |y|), and no
    direction at all reads column W - 1 of an odd-width +-Y or +-Z face or row H - 1 of an odd-height +-Z face.  The tie views read what can be read there."""
    h = lookups
    w, fh, _, _ = layout
    sky = cn.layout_sky(layout)
    h.ctx.upload_scene(h.desc)
    h.set_cubemap(sky.desc())
    reached = _check_views(h, sky)
    assert reached["face"][:, :max(fh // 2 * 2, 1), :max(w // 2 * 2, 1)].all()
    tie = reached["tie"]
    for face in (0, 1):
        assert tie[face, :, w - 1].any() and tie[face, fh - 1, :].any() and tie[face, fh - 1, w - 1]    # u == 1, v == 1, and both in the triple-tie corner
    for face in (2, 3):
        assert tie[face, fh - 1, :].any()


def test_every_half_bit_pattern_through_the_cubemap(lookups):
    """All 65 536 half bit patterns - zeros, subnormals, infinities and NaNs of both signs included - as r, g and b texels of eight 32 x 16 cubemaps (9 216 values
    each), every texel read by the six face views.  Where the oracle's value is NaN the device's is NaN (sign and payload free), everywhere else the bits are
    equal; the same against numpy's own half -> float conversion of the texel each direction addresses.  (A NaN texel reaches color, albedo and nothing else:
    SampleBatchJob has no NaN handling of its own, and color.w stays 1.)"""
    h = lookups
    rng = np.random.default_rng(65536)
    count = 8 * 6 * 16 * 32 * 3
    bits = np.concatenate([np.arange(65536), rng.integers(0, 65536, count - 65536)]).astype(np.uint16)
    bits = bits[rng.permutation(count)].reshape(8, 6, 16, 32, 3)
    assert np.unique(bits).size == 65536
    h.ctx.upload_scene(h.desc)
    for k in range(8):
        faces = np.full((6, 16, 32, 4), 0x3c00, np.uint16)                                 # alpha 1
        faces[..., :3] = bits[k]
        sky = h.rt.scenes.SkyCubemap(faces.view(np.float16), h.rt.abi.CUBEMAP_SIGNED_HALF)
        h.set_cubemap(sky.desc())
        assert _check_views(h, sky, kinds=("face",))["face"].all()


def test_cubemap_replaced_by_another_layout(rt, oracle, lookups):
    """One context through a large half cubemap, a small byte one with stride 5 in the allocation the first left behind (one batch, and three chained in one
    launch), and none: every frame is the oracle's with the same cubemap, and after the drop the sky is black."""
    h = lookups
    big = rt.scenes.synthetic_sky(size=64, half=True)
    small = cn.layout_sky((5, 3, False, 5))
    osc = h.osc
    with rt.Context(0) as ctx:
        ctx.upload_scene(h.desc)
        for sky in (big, small, None, small):
            desc = sky.desc() if sky is not None else None
            ctx.upload_sky_cubemap(desc)
            osc.set_cubemap(desc)
            for kind, face_of_view, p, dirs in h.views:
                n = int(p.size.x) * int(p.size.y)
                gpu, ref = rt.sample_batch_host(ctx, p), osc.sample_batch(p)
                _equal(gpu, ref)
                want = np.zeros((n, 3), np.float32) if sky is None else np.float32(0) + cn.sample(sky, dirs)
                assert np.array_equal(_u32(gpu["color"][:, :3]), _u32(want)) and np.all(gpu["color"][:, 3] == 1), (kind, face_of_view)
                if sky is not small:
                    continue
                plist = [_copy_with_seed(rt, p, seed) for seed in (1, 2, 3)]
                bufs = [rt.DeviceBuffer(ctx, n * c * 4).zero() for c in (4, 3, 3, 1)]
                try:
                    rt.lib.check(rt.sample_batch_chain_device(ctx, plist, bufs, bufs), "rtowSampleBatchChainDevice")
                    ctx.synchronize()
                    chained = {k: b.download(np.float32, (n, c) if c > 1 else (n,)) for k, b, c in zip(KEYS, bufs, (4, 3, 3, 1))}
                finally:
                    for b in bufs:
                        b.free()
                acc = None
                for q in plist:
                    acc = osc.sample_batch(q, None if acc is None else {k: acc[k] for k in KEYS})
                for k in KEYS:
                    assert np.array_equal(_u32(chained[k]).reshape(-1), _u32(acc[k]).reshape(-1)), (kind, face_of_view, k)
                assert np.all(chained["color"][:, 3] == 3)
    osc.set_cubemap(None)


def _copy_with_seed(rt, p, seed):
    q = rt.abi.SampleParams.from_buffer_copy(p)
    q.seed = seed
    return q


@pytest.mark.parametrize("noise_color", ["blue", "stbn"])
@pytest.mark.parametrize("row_stride", [1, 5, 12])
def test_noise_sets_at_odd_strides_and_domain_ends(rt, oracle, gpu_context, row_stride, noise_color):
    """Noise sets of three textures whose row stride is no power of two (`% rowStride` is no mask, and the STBN sections start at all, 4 all, 8 all and 11 all
    bytes with all = 3 * stride^2), read from the last texture, with the texel values of textures made from 8-bit data planted among the random ones: blue +0, 1,
    the smallest and largest subnormal half, the smallest normal and the half below 1 in .x and .y, STBN bytes 0 and 255 in every channel of the five sets (see
    NoiseTextures(planted=True): each in 1/8 of the texels; a stride of 1 is one texel a texture, read by every draw).  Sphere, moving + lens and volume scenes, and
    the tiny scene once more behind a wide lens, so that every draw kind - jitter, lens disk, time, cosine hemisphere, sphere direction, scalar - meets them."""
    ctx, S, a = gpu_context, rt.scenes, rt.abi
    color = a.NOISE_BLUE if noise_color == "blue" else a.NOISE_SPATIOTEMPORAL_BLUE
    noise = S.NoiseTextures(row_stride=row_stride, count=3, planted=True)
    ctx.upload_blue_noise(noise.blue_desc())
    ctx.upload_stb_noise(noise.stb_desc())
    try:
        for scene, lens in ((S.cover_scene(60, 600), None), (S.tiny_scene(), None), (S.volume_scene(), None), (S.tiny_scene(), 0.5)):
            desc = scene.desc()
            p = S.make_params(scene, 40, 36, spp=3, trace_depth=8, seed=5, jitter=True, noise_color=color, noise_texture_index=2)
            if lens is not None:
                p.view.lensRadius = lens
            ctx.upload_scene(desc)
            gpu = rt.sample_batch_host(ctx, p)
            osc = oracle.OracleScene(desc)
            osc.set_blue_noise(noise.blue_desc())
            osc.set_stb_noise(noise.stb_desc())
            ref = osc.sample_batch(p)
            osc.close()
            for k in KEYS:
                assert np.array_equal(_u32(gpu[k]), _u32(ref[k])), (scene.name, lens, k)
            assert np.array_equal(gpu["diag"][:, 0], ref["diag"][:, 0]), (scene.name, lens)
            assert gpu["color"][:, 3].sum() > 0
    finally:
        ctx.upload_blue_noise(None)
        ctx.upload_stb_noise(None)
