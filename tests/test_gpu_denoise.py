"""GPU tests of rtowDenoiseDevice (include/rtow.h): the a-trous kernel bit for bit against the numpy restatement of its specification
(tests/denoise_reference.py), the combine -> denoise -> finalize chain on a caller's stream against the oracle, exact edges, denoising quality on the cover
scene, refusals and determinism.  All in the session context, no subprocesses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
# (flags, normalSharpness, colorSigma, albedoSigma): demodulation on and off, each sigma at 0, both at 0
CONFIGS = [(1, 4, 0.5, 0.5), (0, 7, 0.5, 0.1), (1, 0, 0.0, 0.3), (0, 3, 0.25, 0.0), (1, 8, 0.0, 0.0)]
SIZES = [(1, 1), (1, 37), (37, 1), (41, 29), (96, 54), (257, 3)]


class Frame:
    """float3 device buffers at a byte offset into their allocations (4: views that are only 4-byte aligned)"""

    def __init__(self, rt, ctx, n, offset=0):
        self.rt, self.ctx, self.n, self.offset = rt, ctx, n, offset
        self.buf = rt.DeviceBuffer(ctx, n * 12 + offset + 4)

    @property
    def ptr(self):
        return self.buf.ptr + self.offset

    def upload(self, a):
        a = np.ascontiguousarray(a, F)
        assert a.nbytes == self.n * 12
        self.rt.lib.check(self.rt.lib.load().rtowDeviceCopy(self.ctx.handle, a.ctypes.data, self.ptr, a.nbytes, self.rt.abi.MEMCPY_HOST_TO_DEVICE), "rtowDeviceCopy")
        return self

    def download(self):
        out = np.empty((self.n, 3), F)
        self.rt.lib.check(self.rt.lib.load().rtowDeviceCopy(self.ctx.handle, self.ptr, out.ctypes.data, out.nbytes, self.rt.abi.MEMCPY_DEVICE_TO_HOST), "rtowDeviceCopy")
        return out

    def free(self):
        self.buf.free()


def _inputs(w, h, seed):
    """random guided frame with the awkward values the specification names: NaN and +-inf colours, exactly-zero normals (blocks of them, so sky sits
    beside sky and beside surface), zero, tiny and threshold albedo, negative and zero normal dot products"""
    rng = np.random.default_rng(seed)
    n = w * h
    c = rng.uniform(0, 3, (n, 3)).astype(F)
    c[rng.random(n) < 0.02] *= F(40)                                   # fireflies
    for val in (np.nan, np.inf, -np.inf):
        idx = rng.integers(0, n, max(1, n // 97))
        c[idx, rng.integers(0, 3, idx.size)] = val
    nrm = rng.normal(size=(n, 3)).astype(F)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(F)
    nrm[(rng.random(n) < 0.5)] = nrm[0]                                # large areas with one normal, so some weights survive sharpness 8
    img = nrm.reshape(h, w, 3)
    img[: h // 3, : w // 2] = 0                                        # a block of sky
    nrm[rng.random(n) < 0.03] = 0
    a = rng.uniform(0, 1, (n, 3)).astype(F)
    a[rng.random(n) < 0.05] = 0
    a[rng.random(n) < 0.05] = F(2.0 ** -10)
    a[rng.random(n) < 0.05] = F(2.0 ** -11)
    return c, nrm, a


def _run(rt, ctx, w, h, frames, params, out, scratch_ptr, stream=None):
    p = rt.abi.DenoiseParams(w, h, *params)
    return rt.lib.load().rtowDenoiseDevice(ctx.handle, C.byref(p), frames[0].ptr, frames[1].ptr, frames[2].ptr, scratch_ptr, out.ptr, stream)


def _check_all_levels(rt, ctx, w, h, c, nrm, a, cfg, offset):
    flags, sharp, cs, asg = cfg
    levels = dr.denoise_levels(w, h, c, nrm, a, 8, sharp, cs, asg, flags)
    n = w * h
    ins = [Frame(rt, ctx, n, offset).upload(x) for x in (c, nrm, a)]
    out, scratch = Frame(rt, ctx, n, offset), Frame(rt, ctx, n, offset)
    try:
        for it in range(1, 9):
            rc = _run(rt, ctx, w, h, ins, (it, sharp, cs, asg, flags, 0), out, scratch.ptr if it > 1 else None)
            assert rc == rt.abi.RTOW_SUCCESS, rc
            ctx.synchronize()
            want = dr.finish(levels[it - 1], a, flags)
            got = out.download()
            bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
            assert bad.size == 0, ((w, h), cfg, it, offset, bad[:5], got[bad[:3]], want[bad[:3]])
    finally:
        for f in ins + [out, scratch]:
            f.free()


@pytest.mark.parametrize("w,h", SIZES)
def test_bit_exact_against_the_restatement(rt, gpu_context, w, h):
    for k, cfg in enumerate(CONFIGS):
        c, nrm, a = _inputs(w, h, 100 * w + h + k)
        _check_all_levels(rt, gpu_context, w, h, c, nrm, a, cfg, offset=4 if k % 2 else 0)


def test_bit_exact_at_1080p(rt, gpu_context):
    w, h = 1920, 1080
    c, nrm, a = _inputs(w, h, 7)
    _check_all_levels(rt, gpu_context, w, h, c, nrm, a, CONFIGS[0], offset=4)


def _render(rt, ctx, scene, w, h, spp, seed):
    return rt.sample_batch_host(ctx, rt.scenes.make_params(scene, w, h, spp=spp, trace_depth=8, seed=seed), want_diag=False)


def test_combine_denoise_finalize_chain_on_a_caller_stream(rt, oracle, gpu_context):
    """rtowCombineDevice -> rtowDenoiseDevice -> rtowFinalizeDevice enqueued back to back on a caller-owned stream with no synchronisation in between:
    the RGBA32 bytes equal oracle.finalize(denoise_reference(oracle.combine(...)))."""
    ctx = gpu_context
    scene = rt.scenes.cover_scene()
    ctx.upload_scene(scene.desc())
    w, h = 96, 54
    n = w * h
    acc = _render(rt, ctx, scene, w, h, 4, 3)
    ins = [rt.DeviceBuffer(ctx).upload(acc[k]) for k in ("color", "normal", "albedo")]
    comb = [rt.DeviceBuffer(ctx, n * 12) for _ in range(3)]
    den, scratch = rt.DeviceBuffer(ctx, n * 12), rt.DeviceBuffer(ctx, rt.abi.denoise_scratch_bytes(w, h))
    r8 = [rt.DeviceBuffer(ctx, n * 4) for _ in range(3)]
    hip = C.CDLL("libamdhip64.so")
    side = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(side)) == 0
    try:
        cj = rt.CombineJob(ctx, (w, h))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = ins
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = comb
        assert cj.Schedule(side).Complete() == 0
        dj = rt.DenoiseJob(ctx, w, h)
        dj.InputColor, dj.InputNormal, dj.InputAlbedo, dj.Scratch, dj.OutputColor = comb[0], comb[1], comb[2], scratch, den
        assert dj.Schedule(side).Complete() == 0
        fj = rt.FinalizeTexturesJob(ctx, n)
        fj.InputColor, fj.InputNormal, fj.InputAlbedo = den, comb[1], comb[2]
        fj.OutputColor, fj.OutputNormal, fj.OutputAlbedo = r8
        assert fj.Schedule(side).Complete() == 0
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        assert hip.hipStreamSynchronize(side) == 0
        oc, on, oa = oracle.combine(w, h, acc["color"], acc["normal"], acc["albedo"])
        a = rt.abi
        dref = dr.denoise_reference(w, h, oc, on, oa, a.DENOISE_DEFAULT_ITERATIONS, a.DENOISE_DEFAULT_NORMAL_SHARPNESS, a.DENOISE_DEFAULT_COLOR_SIGMA,
                                    a.DENOISE_DEFAULT_ALBEDO_SIGMA, a.DENOISE_DEFAULT_FLAGS)
        assert np.array_equal(den.download(F, (n, 3)).view(np.uint32), dref.view(np.uint32))
        want = oracle.finalize(dref, on, oa)
        for got, wv in zip(r8, want):
            assert np.array_equal(got.download(np.uint8, (n, 4)), wv)
        assert not np.array_equal(want[0], oracle.finalize(oc, on, oa)[0])        # the denoise pass changed the picture
    finally:
        for b in ins + comb + [den, scratch] + r8:
            b.free()
        hip.hipStreamDestroy.argtypes = [C.c_void_p]
        hip.hipStreamDestroy(side)


def _denoise_host(rt, ctx, w, h, c, nrm, a, params):
    n = w * h
    ins = [Frame(rt, ctx, n).upload(x) for x in (c, nrm, a)]
    out, scratch = Frame(rt, ctx, n), Frame(rt, ctx, n)
    try:
        assert _run(rt, ctx, w, h, ins, params, out, scratch.ptr) == rt.abi.RTOW_SUCCESS
        ctx.synchronize()
        return out.download()
    finally:
        for f in ins + [out, scratch]:
            f.free()


def test_edges_hold_exactly(rt, gpu_context):
    """Two planes with perpendicular normals, and a sky / surface silhouette (exactly-zero normals beside non-zero ones): changing every colour right of
    the edge leaves every output pixel left of it bit-identical, at every level count."""
    rng = np.random.default_rng(11)
    w, h, edge = 150, 40, 61
    n = w * h
    c = rng.uniform(0, 2, (n, 3)).astype(F)
    c2 = c.reshape(h, w, 3).copy()
    c2[:, edge:] = rng.uniform(0, 100, (h, w - edge, 3))
    c2 = c2.reshape(-1, 3)
    a = rng.uniform(0.1, 1, (n, 3)).astype(F)
    planes = np.zeros((h, w, 3), F)
    planes[:, :edge] = (1, 0, 0)
    planes[:, edge:] = (0, 0, 1)
    sky = np.zeros((h, w, 3), F)
    sky[:, edge:] = (0, 0.6, 0.8)
    for nrm in (planes.reshape(-1, 3), sky.reshape(-1, 3)):
        for it in (1, 5, 8):
            params = (it, 0, 0.0, 0.0, 1, 0)                           # no colour / albedo terms: only the normals can stop the blur
            x = _denoise_host(rt, gpu_context, w, h, c, nrm, a, params).reshape(h, w, 3)
            y = _denoise_host(rt, gpu_context, w, h, c2, nrm, a, params).reshape(h, w, 3)
            assert np.array_equal(x[:, :edge].view(np.uint32), y[:, :edge].view(np.uint32)), it
            assert not np.array_equal(x[:, edge:], y[:, edge:])


def test_quality_on_the_cover_scene(rt, gpu_context):
    """192 x 108, 4 spp (seed 1) against 1024 spp (seed 2), both combined on the device: with the recommended parameters the denoised frame's mean squared
    error against the 1024-spp frame is at most half the noisy frame's (measured 0.43)."""
    ctx = gpu_context
    scene = rt.scenes.cover_scene()
    ctx.upload_scene(scene.desc())
    w, h = 192, 108
    n = w * h
    combined = []
    for spp, seed in ((4, 1), (1024, 2)):
        acc = _render(rt, ctx, scene, w, h, spp, seed)
        ins = [rt.DeviceBuffer(ctx).upload(acc[k]) for k in ("color", "normal", "albedo")]
        outs = [rt.DeviceBuffer(ctx, n * 12) for _ in range(3)]
        cj = rt.CombineJob(ctx, (w, h))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = ins
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = outs
        assert cj.Schedule().Complete() == 0
        ctx.synchronize()
        combined.append([o.download(F, (n, 3)) for o in outs])
        for b in ins + outs:
            b.free()
    (c4, n4, a4), (ref, _, _) = combined
    a = rt.abi
    den = _denoise_host(rt, ctx, w, h, c4, n4, a4, (a.DENOISE_DEFAULT_ITERATIONS, a.DENOISE_DEFAULT_NORMAL_SHARPNESS, a.DENOISE_DEFAULT_COLOR_SIGMA,
                                                    a.DENOISE_DEFAULT_ALBEDO_SIGMA, a.DENOISE_DEFAULT_FLAGS, 0))
    noisy = float(np.mean((c4.astype(np.float64) - ref) ** 2))
    ratio = float(np.mean((den.astype(np.float64) - ref) ** 2)) / noisy
    print("denoise quality: noisy MSE %.6g, denoised / noisy %.4f" % (noisy, ratio))
    assert np.isfinite(den).all() and ratio <= 0.5, ratio


def test_refusals(rt, gpu_context):
    ctx = gpu_context
    lib = rt.lib.load()
    bad = rt.abi.RTOW_ERROR_INVALID_VALUE
    w, h = 16, 8
    n = w * h
    c, nrm, a = _inputs(w, h, 5)
    ins = [Frame(rt, ctx, n).upload(x) for x in (c, nrm, a)]
    out, scratch = Frame(rt, ctx, n), Frame(rt, ctx, n)
    sentinel = np.full((n, 3), 7.0, F)
    out.upload(sentinel)
    P = rt.abi.DenoiseParams
    good = (3, 4, 0.5, 0.5, 1, 0)
    try:
        def call(params=good, cp=None, npp=None, ap=None, sp=-1, op=None, size=(w, h)):
            p = P(size[0], size[1], *params)
            return lib.rtowDenoiseDevice(ctx.handle, C.byref(p), cp or ins[0].ptr, npp or ins[1].ptr, ap or ins[2].ptr,
                                         scratch.ptr if sp == -1 else sp, op or out.ptr, None)
        # aliasing: the output or the scratch on an input, the output on the scratch, a partial overlap
        assert call(op=ins[0].ptr) == bad and call(op=ins[1].ptr) == bad and call(op=ins[2].ptr) == bad
        assert call(sp=ins[0].ptr) == bad and call(sp=out.ptr) == bad and call(op=scratch.ptr + 12) == bad
        # NULL scratch with more than one level (one level needs none), NULL inputs
        assert call(sp=None) == bad
        assert lib.rtowDenoiseDevice(ctx.handle, C.byref(P(w, h, *good)), None, ins[1].ptr, ins[2].ptr, scratch.ptr, out.ptr, None) == bad
        assert lib.rtowDenoiseDevice(ctx.handle, C.byref(P(w, h, *good)), ins[0].ptr, ins[1].ptr, ins[2].ptr, scratch.ptr, None, None) == bad
        # parameters
        for params in ((0, 4, 0.5, 0.5, 1, 0), (9, 4, 0.5, 0.5, 1, 0), (3, -1, 0.5, 0.5, 1, 0), (3, 9, 0.5, 0.5, 1, 0), (3, 4, -0.5, 0.5, 1, 0),
                       (3, 4, 0.5, -1e-30, 1, 0), (3, 4, float("nan"), 0.5, 1, 0), (3, 4, 0.5, float("inf"), 1, 0), (3, 4, 0.5, 0.5, 3, 0),
                       (3, 4, 0.5, 0.5, -1, 0), (3, 4, 0.5, 0.5, 1, 1), (3, 4, 0.5, 0.5, 1, -7)):
            assert call(params) == bad, params
        for size in ((0, h), (w, 0), (-1, h), (65536, 32768)):
            assert call(size=size) == bad, size
        ctx.synchronize()
        assert np.array_equal(out.download(), sentinel)                # nothing was enqueued
        assert call((1, 4, 0.5, 0.5, 1, 0), sp=None) == rt.abi.RTOW_SUCCESS
        ctx.synchronize()
        assert np.array_equal(out.download().view(np.uint32), dr.denoise_reference(w, h, c, nrm, a, 1, 4, 0.5, 0.5, 1).view(np.uint32))
    finally:
        for f in ins + [out, scratch]:
            f.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    w, h = 320, 180
    c, nrm, a = _inputs(w, h, 9)
    x = _denoise_host(rt, gpu_context, w, h, c, nrm, a, (8, 4, 0.5, 0.5, 1, 0))
    y = _denoise_host(rt, gpu_context, w, h, c, nrm, a, (8, 4, 0.5, 0.5, 1, 0))
    assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
