"""GPU tests of rtowAccumulateMomentsDevice and rtowDenoiseVarianceDevice (include/rtow.h): both kernels bit for bit against the numpy restatement of their
specification (tests/denoise_variance_reference.py), what follows from the specification (no colour term = rtowDenoiseDevice at colorSigma 0), the behaviour at
a luminance step, the group -> moments -> fold -> combine -> denoise -> finalize chain on a caller's stream against the oracle, refusals, determinism, and the
denoising quality on two cover-scene frames of very different noise.  All in the session context, no subprocesses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402
import denoise_variance_reference as dv  # noqa: E402
from test_gpu_denoise import SIZES, _inputs  # noqa: E402  (the sizes and the awkward guided frames of the plain filter's tests)

pytestmark = pytest.mark.gpu

F = np.float32
# (flags, normalSharpness, colorSigma, albedoSigma): demodulation on and off, each sigma at 0, both at 0
CONFIGS = [(1, 4, 4.0, 0.5), (0, 7, 2.0, 0.1), (1, 0, 0.0, 0.3), (0, 3, 8.0, 0.0), (1, 8, 0.0, 0.0)]


class View:
    """`nbytes` of device memory at a byte offset into its allocation (4: a view that is only 4-byte aligned)"""

    def __init__(self, rt, ctx, nbytes, offset=0):
        self.rt, self.ctx, self.nbytes, self.offset = rt, ctx, nbytes, offset
        self.buf = rt.DeviceBuffer(ctx, nbytes + offset + 4)

    @property
    def ptr(self):
        return self.buf.ptr + self.offset

    def upload(self, a):
        a = np.ascontiguousarray(a, F)
        assert a.nbytes == self.nbytes, (a.nbytes, self.nbytes)
        self.rt.lib.check(self.rt.lib.load().rtowDeviceCopy(self.ctx.handle, a.ctypes.data, self.ptr, a.nbytes, self.rt.abi.MEMCPY_HOST_TO_DEVICE), "rtowDeviceCopy")
        return self

    def download(self, shape):
        out = np.empty(shape, F)
        assert out.nbytes == self.nbytes
        self.rt.lib.check(self.rt.lib.load().rtowDeviceCopy(self.ctx.handle, self.ptr, out.ctypes.data, out.nbytes, self.rt.abi.MEMCPY_DEVICE_TO_HOST), "rtowDeviceCopy")
        return out

    def free(self):
        self.buf.free()


def _same_bits(got, want):
    return np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


# ---------------------------------------------------------------- moments

def _batch_colors(n, count, seed):
    """per-batch accumulator colours (rgb sums, w = successful samples) with what the specification names: w = 0, negative and NaN w, inf / NaN channels"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        w = rng.integers(1, 5, n).astype(F)
        c = np.concatenate([rng.uniform(0, 3, (n, 3)).astype(F) * w[:, None], w[:, None]], axis=1).astype(F)
        c[rng.random(n) < 0.1, 3] = 0
        c[rng.random(n) < 0.05, 3] = -2
        c[rng.random(n) < 0.05, 3] = np.nan
        for val in (np.inf, -np.inf, np.nan, 3e38):
            idx = rng.integers(0, n, max(1, n // 23))
            c[idx, rng.integers(0, 3, idx.size)] = val
        out.append(c)
    return out


def _moments(rt, ctx, n, color_views, in_ptr, out_ptr, stream=None):
    arr = (C.c_void_p * len(color_views))(*[v.ptr for v in color_views])
    return rt.lib.load().rtowAccumulateMomentsDevice(ctx.handle, n, len(color_views), arr, in_ptr, out_ptr, stream)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 41 * 29])
def test_moments_bit_exact_against_the_restatement(rt, gpu_context, n):
    ctx = gpu_context
    for count in (1, 4, 16):
        offset = 4 if count != 4 else 0
        colors = _batch_colors(n, count, 1000 * n + count)
        more = _batch_colors(n, count, 1000 * n + count + 500)
        views = [View(rt, ctx, n * 16, offset).upload(c) for c in colors]
        m = View(rt, ctx, n * 12, offset).upload(np.full((n, 3), 9.0, F))
        other = View(rt, ctx, n * 12, offset)
        try:
            assert _moments(rt, ctx, n, views, None, m.ptr) == rt.abi.RTOW_SUCCESS              # from a NULL input: zeros
            ctx.synchronize()
            first = dv.accumulate_moments(colors)
            got = m.download((n, 3))
            assert _same_bits(got, first), (n, count, np.flatnonzero((got != first).any(1))[:5])
            assert (first[:, 2] < count).any() or n < 8                                         # some batches were skipped
            for v, c in zip(views, more):
                v.upload(c)
            assert _moments(rt, ctx, n, views, m.ptr, m.ptr) == rt.abi.RTOW_SUCCESS             # in place: the next kick of the frame
            ctx.synchronize()
            second = dv.accumulate_moments(more, first)
            assert _same_bits(m.download((n, 3)), second), (n, count)
            assert _moments(rt, ctx, n, views, m.ptr, other.ptr) == rt.abi.RTOW_SUCCESS         # out of place, from given moments
            ctx.synchronize()
            assert _same_bits(other.download((n, 3)), dv.accumulate_moments(more, second)), (n, count)
            assert _same_bits(m.download((n, 3)), second)                                       # the input stayed as it was
        finally:
            for v in views + [m, other]:
                v.free()


# ---------------------------------------------------------------- the filter

def _moment_inputs(n, seed):
    """moments with n in {0, 1, 2, 7}, plausible sums, cancellation (s2 < s1^2 / n), huge and NaN entries"""
    rng = np.random.default_rng(seed)
    cnt = rng.choice(np.array([0, 1, 2, 7], F), n, p=[0.1, 0.1, 0.3, 0.5])
    mean = rng.uniform(0, 2, n).astype(F)
    spread = rng.uniform(0, 1, n).astype(F)
    s1 = (cnt * mean).astype(F)
    s2 = (cnt * (mean * mean + spread * spread)).astype(F)
    m = np.stack([s1, s2, cnt], axis=1).astype(F)
    k = rng.random(n)
    m[k < 0.08, 1] *= F(0.5)                                              # s2 < s1^2 / n: the difference cancels below zero
    m[(k >= 0.08) & (k < 0.12), 1] = (m[(k >= 0.08) & (k < 0.12), 0] ** 2 / np.maximum(m[(k >= 0.08) & (k < 0.12), 2], 1)).astype(F)   # exactly no spread, up to rounding
    for col, val in ((0, 3e38), (1, 3e38), (1, 1e30), (1, np.inf), (0, np.nan), (1, np.nan), (2, np.nan), (2, np.inf), (1, 1e-30)):
        idx = rng.integers(0, n, max(1, n // (600 if val == 3e38 else 61)))      # a huge variance spreads to every pixel whose taps reach it: keep those few
        m[idx, col] = val
    return m


def _run(rt, ctx, w, h, ins, moments, params, out, scratch, var_ptr, stream=None):
    p = rt.abi.DenoiseParams(w, h, *params)
    return rt.lib.load().rtowDenoiseVarianceDevice(ctx.handle, C.byref(p), ins[0].ptr, ins[1].ptr, ins[2].ptr, moments.ptr, scratch.ptr, out.ptr, var_ptr, stream)


def _check_all_levels(rt, ctx, w, h, c, nrm, a, m, cfg, offset, null_variance_at):
    flags, sharp, cs, asg = cfg
    levels = dv.denoise_variance_levels(w, h, c, nrm, a, m, 8, sharp, cs, asg, flags)
    n = w * h
    ins = [View(rt, ctx, n * 12, offset).upload(x) for x in (c, nrm, a)]
    mom = View(rt, ctx, n * 12, offset).upload(m)
    out, var = View(rt, ctx, n * 12, offset), View(rt, ctx, n * 4, offset)
    scratch = View(rt, ctx, rt.abi.denoise_variance_scratch_bytes(w, h), offset)
    try:
        for it in range(1, 9):
            want_c, want_v = dv.finish(levels[it - 1], a, flags)
            var.upload(np.full(n, 5.0, F))
            rc = _run(rt, ctx, w, h, ins, mom, (it, sharp, cs, asg, flags, 0), out, scratch, var.ptr)
            assert rc == rt.abi.RTOW_SUCCESS, rc
            ctx.synchronize()
            got, got_v = out.download((n, 3)), var.download((n,))
            bad = np.flatnonzero((got.view(np.uint32) != want_c.view(np.uint32)).any(1))
            assert bad.size == 0, ((w, h), cfg, it, offset, bad[:5], got[bad[:3]], want_c[bad[:3]])
            bad = np.flatnonzero(got_v.view(np.uint32) != want_v.view(np.uint32))
            assert bad.size == 0, ((w, h), cfg, it, offset, bad[:5], got_v[bad[:3]], want_v[bad[:3]])
            assert not np.isnan(got_v).any()
            if it == null_variance_at:                                     # without outVariance: the same colour, and nothing written there
                var.upload(np.full(n, 5.0, F))
                out.upload(np.zeros((n, 3), F))
                assert _run(rt, ctx, w, h, ins, mom, (it, sharp, cs, asg, flags, 0), out, scratch, None) == rt.abi.RTOW_SUCCESS
                ctx.synchronize()
                assert _same_bits(out.download((n, 3)), want_c) and (var.download((n,)) == 5.0).all()
    finally:
        for f in ins + [mom, out, var, scratch]:
            f.free()


@pytest.mark.parametrize("w,h", SIZES)
def test_filter_bit_exact_against_the_restatement(rt, gpu_context, w, h):
    for k, cfg in enumerate(CONFIGS):
        c, nrm, a = _inputs(w, h, 100 * w + h + k)
        m = _moment_inputs(w * h, 7 * w + h + k)
        _check_all_levels(rt, gpu_context, w, h, c, nrm, a, m, cfg, offset=4 if k % 2 else 0, null_variance_at=1 + (k + w) % 8)


def _device_outputs(rt, ctx, w, h, c, nrm, a, m, params, plain=False):
    """outColor (and outVariance) of one call; plain: rtowDenoiseDevice on the same frame"""
    n = w * h
    ins = [View(rt, ctx, n * 12).upload(x) for x in (c, nrm, a)]
    mom = View(rt, ctx, n * 12).upload(m)
    out, var, scratch = View(rt, ctx, n * 12), View(rt, ctx, n * 4), View(rt, ctx, rt.abi.denoise_variance_scratch_bytes(w, h))
    try:
        if plain:
            p = rt.abi.DenoiseParams(w, h, *params)
            rc = rt.lib.load().rtowDenoiseDevice(ctx.handle, C.byref(p), ins[0].ptr, ins[1].ptr, ins[2].ptr, scratch.ptr, out.ptr, None)
        else:
            rc = _run(rt, ctx, w, h, ins, mom, params, out, scratch, var.ptr)
        assert rc == rt.abi.RTOW_SUCCESS, rc
        ctx.synchronize()
        return out.download((n, 3)), (None if plain else var.download((n,)))
    finally:
        for f in ins + [mom, out, var, scratch]:
            f.free()


def test_without_a_colour_term_the_colour_is_the_plain_filters(rt, gpu_context):
    """colorSigma == 0: outColor is rtowDenoiseDevice's at colorSigma 0 on the same inputs, bit for bit, for any moments; with every n < 2 no pixel has a
    variance, and the same holds for colorSigma > 0."""
    w, h = 96, 54
    c, nrm, a = _inputs(w, h, 21)
    m = _moment_inputs(w * h, 22)
    few = m.copy()
    few[:, 2] = np.random.default_rng(23).integers(0, 2, w * h)
    for flags, sharp, asg, it in ((1, 4, 0.5, 5), (0, 2, 0.0, 8), (1, 0, 0.2, 1)):
        plain, _ = _device_outputs(rt, gpu_context, w, h, c, nrm, a, m, (it, sharp, 0.0, asg, flags, 0), plain=True)
        got, _ = _device_outputs(rt, gpu_context, w, h, c, nrm, a, m, (it, sharp, 0.0, asg, flags, 0))
        assert _same_bits(got, plain), (flags, sharp, asg, it)
        got, var = _device_outputs(rt, gpu_context, w, h, c, nrm, a, few, (it, sharp, 4.0, asg, flags, 0))
        assert _same_bits(got, plain), (flags, sharp, asg, it)
        assert (var == -1).all()
    on, _ = _device_outputs(rt, gpu_context, w, h, c, nrm, a, m, (5, 4, 4.0, 0.5, 1, 0))
    assert not _same_bits(on, _device_outputs(rt, gpu_context, w, h, c, nrm, a, m, (5, 4, 0.0, 0.5, 1, 0))[0])         # the colour term does something


def test_the_moments_decide_whether_a_luminance_step_survives(rt, gpu_context):
    """Two flat regions of luminance 0.2 and 1.0 with equal guides, three levels.  Moments that say "no variance" (four equal batch means) make the colour term's
    denominator 2^-20: a tap across the step weighs 1 / (1 + 0.64 * 2^20), and the columns at the step change by less than 1e-4.  Moments that say "variance 100"
    make it 1 / (1 + 0.64 / 1600): the step is blurred like a flat area, and the column next to it moves by more than 0.2 (level 0 alone puts 5/16 of the weight
    across: 0.25)."""
    w, h, edge = 64, 16, 32
    n = w * h
    img = np.empty((h, w, 3), F)
    img[:, :edge] = 0.2
    img[:, edge:] = 1.0
    c = img.reshape(-1, 3)
    nrm = np.tile(np.array([0, 1, 0], F), (n, 1))
    a = np.full((n, 3), 0.5, F)
    l = dv.lum(c)
    params = (3, 4, 4.0, 0.5, 0, 0)

    def change(m):
        out, var = _device_outputs(rt, gpu_context, w, h, c, nrm, a, m, params)
        d = np.abs(out - c).reshape(h, w, 3)[:, edge - 1:edge + 1]
        return float(d.mean()), var

    calm = np.stack([F(4) * l, F(4) * (l * l), np.full(n, 4, F)], axis=1).astype(F)
    noisy = np.stack([F(4) * l, F(4) * (l * l) + F(1200), np.full(n, 4, F)], axis=1).astype(F)      # d = 1200, v = 1200 / 12 = 100
    kept, v_calm = change(calm)
    blurred, v_noisy = change(noisy)
    print("luminance step: mean absolute change at the step %.3g with no variance, %.3g with variance 100" % (kept, blurred))
    assert kept < 1e-4, kept
    assert blurred > 0.2, blurred
    assert (v_calm >= 0).all() and v_calm.max() < 1e-6 and (v_noisy > 0).all() and v_noisy.max() < 100         # filtering reduces the variance


# ---------------------------------------------------------------- end to end

KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))


def _group(rt, ctx, scene, w, h, batches, spp, seed0, stream=None):
    """`batches` independent batches of `spp` samples from zeroed inputs (rtowSampleBatchGroupDevice): the per-batch output buffers, enqueued, not waited for"""
    n = w * h
    zero = [rt.DeviceBuffer(ctx, n * k * 4).zero() for _, k in KEYS]
    outs = [[rt.DeviceBuffer(ctx, n * k * 4).zero() for _, k in KEYS] for _ in range(batches)]
    plist = [rt.scenes.make_params(scene, w, h, spp=spp, trace_depth=8, seed=seed0 + b) for b in range(batches)]
    ctx.synchronize()                                                      # the zero fills, before anything goes to another stream
    assert rt.sample_batch_group_device(ctx, plist, zero, outs, None, stream) == 0
    return zero, outs


def _fold(rt, ctx, n, acc, outs, stream=None):
    lib = rt.lib.load()
    dst = rt.abi.AccumBuffers(*[b.ptr for b in acc])
    for o in outs:
        src = rt.abi.AccumBuffers(*[b.ptr for b in o])
        assert lib.rtowAddAccumDevice(ctx.handle, n, C.byref(dst), C.byref(src), stream) == 0


def test_group_moments_fold_combine_denoise_finalize_chain_on_a_caller_stream(rt, oracle, gpu_context):
    """4 batches of 1 spp as a group -> rtowAccumulateMomentsDevice -> rtowAddAccumDevice folds -> rtowCombineDevice -> rtowDenoiseVarianceDevice ->
    rtowFinalizeDevice, enqueued back to back on a caller-owned stream with no synchronisation in between: the RGBA32 bytes equal oracle combine / finalize
    around the restatement, fed from the downloaded per-batch buffers."""
    ctx = gpu_context
    scene = rt.scenes.cover_scene()
    ctx.upload_scene(scene.desc())
    w, h = 96, 54
    n = w * h
    a = rt.abi
    hip = C.CDLL("libamdhip64.so")
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipStreamDestroy.argtypes = [C.c_void_p]
    side = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(side)) == 0
    bufs = []
    try:
        acc = [rt.DeviceBuffer(ctx, n * k * 4).zero() for _, k in KEYS]
        mom = rt.DeviceBuffer(ctx, a.moments_bytes(n))
        comb = [rt.DeviceBuffer(ctx, n * 12) for _ in range(3)]
        den, var = rt.DeviceBuffer(ctx, n * 12), rt.DeviceBuffer(ctx, n * 4)
        scratch = rt.DeviceBuffer(ctx, a.denoise_variance_scratch_bytes(w, h))
        r8 = [rt.DeviceBuffer(ctx, n * 4) for _ in range(3)]
        bufs = acc + [mom] + comb + [den, var, scratch] + r8
        zero, outs = _group(rt, ctx, scene, w, h, 4, 1, 1, side)
        bufs += zero + [b for o in outs for b in o]
        mj = rt.MomentsJob(ctx, n)
        mj.Colors, mj.OutputMoments = [o[0] for o in outs], mom
        assert mj.Schedule(side).Complete() == 0
        _fold(rt, ctx, n, acc, outs, side)
        cj = rt.CombineJob(ctx, (w, h))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = acc[:3]
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = comb
        assert cj.Schedule(side).Complete() == 0
        dj = rt.DenoiseVarianceJob(ctx, w, h)
        dj.InputColor, dj.InputNormal, dj.InputAlbedo, dj.Moments, dj.Scratch, dj.OutputColor, dj.OutputVariance = comb[0], comb[1], comb[2], mom, scratch, den, var
        assert dj.Schedule(side).Complete() == 0
        fj = rt.FinalizeTexturesJob(ctx, n)
        fj.InputColor, fj.InputNormal, fj.InputAlbedo = den, comb[1], comb[2]
        fj.OutputColor, fj.OutputNormal, fj.OutputAlbedo = r8
        assert fj.Schedule(side).Complete() == 0
        assert hip.hipStreamSynchronize(side) == 0
        per_batch = [[b.download(F, (n, k)) for b, (_, k) in zip(o, KEYS)] for o in outs]
        folded = [np.zeros((n, k), F) for _, k in KEYS]
        for pb in per_batch:
            folded = [f + x for f, x in zip(folded, pb)]                   # rtowAddAccumDevice: dst += src, in batch order
        m_ref = dv.accumulate_moments([pb[0] for pb in per_batch])
        assert _same_bits(mom.download(F, (n, 3)), m_ref)
        assert (m_ref[:, 2] >= 2).mean() > 0.5                            # most pixels have a variance estimate (a batch whose one sample failed is skipped)
        oc, on, oa = oracle.combine(w, h, folded[0], folded[1], folded[2])
        dref, vref = dv.denoise_variance_reference(w, h, oc, on, oa, m_ref, a.DENOISE_VARIANCE_DEFAULT_ITERATIONS, a.DENOISE_VARIANCE_DEFAULT_NORMAL_SHARPNESS,
                                                   a.DENOISE_VARIANCE_DEFAULT_COLOR_SIGMA, a.DENOISE_VARIANCE_DEFAULT_ALBEDO_SIGMA, a.DENOISE_VARIANCE_DEFAULT_FLAGS)
        assert _same_bits(den.download(F, (n, 3)), dref)
        assert _same_bits(var.download(F, (n,)), vref)
        want = oracle.finalize(dref, on, oa)
        for got, wv in zip(r8, want):
            assert np.array_equal(got.download(np.uint8, (n, 4)), wv)
        assert not np.array_equal(want[0], oracle.finalize(oc, on, oa)[0])        # the denoise pass changed the picture
    finally:
        hip.hipStreamSynchronize(side)
        for b in bufs:
            b.free()
        hip.hipStreamDestroy(side)


# ---------------------------------------------------------------- refusals, determinism

def test_refusals(rt, gpu_context):
    ctx = gpu_context
    lib = rt.lib.load()
    bad = rt.abi.RTOW_ERROR_INVALID_VALUE
    w, h = 16, 8
    n = w * h
    c, nrm, a = _inputs(w, h, 5)
    m = _moment_inputs(n, 6)
    ins = [View(rt, ctx, n * 12).upload(x) for x in (c, nrm, a)]
    mom = View(rt, ctx, n * 12).upload(m)
    out, var = View(rt, ctx, n * 12), View(rt, ctx, n * 4)
    scratch = View(rt, ctx, rt.abi.denoise_variance_scratch_bytes(w, h))
    colors = [View(rt, ctx, n * 16).upload(x) for x in _batch_colors(n, 16, 8)]
    sentinel, sentinel_v = np.full((n, 3), 7.0, F), np.full(n, 7.0, F)
    out.upload(sentinel)
    var.upload(sentinel_v)
    P = rt.abi.DenoiseParams
    good = (3, 4, 4.0, 0.5, 1, 0)
    try:
        def call(params=good, cp=None, npp=None, ap=None, mp=None, sp=-1, op=-1, vp=-1, size=(w, h), context=ctx.handle):
            p = P(size[0], size[1], *params)
            return lib.rtowDenoiseVarianceDevice(context, C.byref(p), cp or ins[0].ptr, npp or ins[1].ptr, ap or ins[2].ptr, mp or mom.ptr,
                                                 scratch.ptr if sp == -1 else sp, out.ptr if op == -1 else op, var.ptr if vp == -1 else vp, None)
        # NULL: context, params, each input, moments, scratch (even with one level), outColor
        assert call(context=None) == bad
        assert lib.rtowDenoiseVarianceDevice(ctx.handle, None, ins[0].ptr, ins[1].ptr, ins[2].ptr, mom.ptr, scratch.ptr, out.ptr, var.ptr, None) == bad
        for k in range(4):
            ptrs = [ins[0].ptr, ins[1].ptr, ins[2].ptr, mom.ptr]
            ptrs[k] = None
            assert lib.rtowDenoiseVarianceDevice(ctx.handle, C.byref(P(w, h, *good)), *ptrs, scratch.ptr, out.ptr, var.ptr, None) == bad, k
        assert call(sp=None) == bad and call((1, 4, 4.0, 0.5, 1, 0), sp=None) == bad and call(op=None) == bad
        # aliasing: every written buffer on every input and on the moments, on each other, partial overlaps
        for target in (ins[0].ptr, ins[1].ptr, ins[2].ptr, mom.ptr):
            assert call(op=target) == bad and call(vp=target) == bad and call(sp=target) == bad
            assert call(vp=target + n * 12 - 4) == bad                     # the last word of the input
        assert call(sp=out.ptr) == bad and call(vp=out.ptr) == bad and call(sp=var.ptr) == bad
        assert call(op=scratch.ptr + n * 20 - 4) == bad and call(vp=scratch.ptr + n * 16) == bad and call(op=var.ptr - 8) == bad
        # parameters: rtowDenoiseDevice's
        for params in ((0, 4, 4.0, 0.5, 1, 0), (9, 4, 4.0, 0.5, 1, 0), (3, -1, 4.0, 0.5, 1, 0), (3, 9, 4.0, 0.5, 1, 0), (3, 4, -0.5, 0.5, 1, 0),
                       (3, 4, 4.0, -1e-30, 1, 0), (3, 4, float("nan"), 0.5, 1, 0), (3, 4, 4.0, float("inf"), 1, 0), (3, 4, 4.0, 0.5, 3, 0),
                       (3, 4, 4.0, 0.5, -1, 0), (3, 4, 4.0, 0.5, 1, 1), (3, 4, 4.0, 0.5, 1, -7)):
            assert call(params) == bad, params
        for size in ((0, h), (w, 0), (-1, h), (65536, 32768)):
            assert call(size=size) == bad, size
        ctx.synchronize()
        assert np.array_equal(out.download((n, 3)), sentinel) and np.array_equal(var.download((n,)), sentinel_v)       # nothing was enqueued
        assert call() == rt.abi.RTOW_SUCCESS
        ctx.synchronize()
        want_c, want_v = dv.denoise_variance_reference(w, h, c, nrm, a, m, 3, 4, 4.0, 0.5, 1)
        assert _same_bits(out.download((n, 3)), want_c) and _same_bits(var.download((n,)), want_v)

        # rtowAccumulateMomentsDevice
        mout = View(rt, ctx, n * 12).upload(sentinel)

        def acc(count=4, cols=None, ip=None, op=-1, pixels=n, context=ctx.handle, null_list=False):
            cols = cols if cols is not None else [v.ptr for v in colors[:max(count, 0)]]
            arr = (C.c_void_p * max(len(cols), 1))(*cols)
            return lib.rtowAccumulateMomentsDevice(context, pixels, count, None if null_list else arr, ip, mout.ptr if op == -1 else op, None)
        assert acc(context=None) == bad and acc(null_list=True) == bad and acc(op=None) == bad
        assert acc(cols=[colors[0].ptr, None, colors[2].ptr, colors[3].ptr]) == bad
        assert acc(pixels=0) == bad and acc(pixels=-5) == bad
        assert acc(count=0) == bad and acc(count=-1, cols=[colors[0].ptr]) == bad and acc(count=17, cols=[v.ptr for v in colors] + [colors[0].ptr]) == bad
        assert acc(op=colors[2].ptr) == bad and acc(op=colors[3].ptr + n * 16 - 4) == bad and acc(op=colors[0].ptr - n * 12 + 4) == bad      # the output on a colour buffer
        assert acc(ip=mout.ptr + 12) == bad and acc(ip=mout.ptr - 4) == bad                                       # the input overlaps the output, but not exactly
        ctx.synchronize()
        assert np.array_equal(mout.download((n, 3)), sentinel)              # nothing was enqueued
        assert acc(count=16, ip=mout.ptr) == rt.abi.RTOW_SUCCESS            # exactly in place is allowed
        ctx.synchronize()
        assert _same_bits(mout.download((n, 3)), dv.accumulate_moments(_batch_colors(n, 16, 8), sentinel))
        mout.free()
    finally:
        for f in ins + [mom, out, var, scratch] + colors:
            f.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    w, h = 320, 180
    c, nrm, a = _inputs(w, h, 9)
    m = _moment_inputs(w * h, 10)
    x = _device_outputs(rt, gpu_context, w, h, c, nrm, a, m, (8, 4, 4.0, 0.5, 1, 0))
    y = _device_outputs(rt, gpu_context, w, h, c, nrm, a, m, (8, 4, 4.0, 0.5, 1, 0))
    assert _same_bits(x[0], y[0]) and _same_bits(x[1], y[1])
    colors = _batch_colors(w * h, 4, 11)
    views = [View(rt, gpu_context, w * h * 16).upload(k) for k in colors]
    outs = [View(rt, gpu_context, w * h * 12) for _ in range(2)]
    try:
        for o in outs:
            assert _moments(rt, gpu_context, w * h, views, None, o.ptr) == rt.abi.RTOW_SUCCESS
        gpu_context.synchronize()
        assert _same_bits(outs[0].download((w * h, 3)), outs[1].download((w * h, 3)))
    finally:
        for v in views + outs:
            v.free()


# ---------------------------------------------------------------- quality

def quality_frames(rt, ctx, w=192, h=108):
    """tests/test_gpu_denoise.py's protocol (cover scene, 192 x 108, against 1024 spp of another seed) on two frames rendered as batch groups: 4 x 1 spp and
    16 x 4 spp.  Per frame: combine's (colour, normal, albedo) of the folded batches, and the moments of the batches; and the 1024-spp reference colour.
    (profiles/denoise_variance_timing.py runs its parameter grid on the same frames.)"""
    scene = rt.scenes.cover_scene()
    ctx.upload_scene(scene.desc())
    n = w * h

    def combine(acc):
        outs = [rt.DeviceBuffer(ctx, n * 12) for _ in range(3)]
        cj = rt.CombineJob(ctx, (w, h))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = acc[:3]
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = outs
        assert cj.Schedule().Complete() == 0
        ctx.synchronize()
        res = [o.download(F, (n, 3)) for o in outs]
        for b in outs:
            b.free()
        return res

    frames = []
    for batches, spp, seed0 in ((4, 1, 1), (16, 4, 101)):
        zero, outs = _group(rt, ctx, scene, w, h, batches, spp, seed0)
        acc = [rt.DeviceBuffer(ctx, n * k * 4).zero() for _, k in KEYS]
        mom = rt.DeviceBuffer(ctx, rt.abi.moments_bytes(n))
        mj = rt.MomentsJob(ctx, n)
        mj.Colors, mj.OutputMoments = [o[0] for o in outs], mom
        assert mj.Schedule().Complete() == 0
        _fold(rt, ctx, n, acc, outs)
        ctx.synchronize()
        frames.append(combine(acc) + [mom.download(F, (n, 3))])
        for b in zero + acc + [mom] + [b for o in outs for b in o]:
            b.free()
    ref = rt.sample_batch_host(ctx, rt.scenes.make_params(scene, w, h, spp=1024, trace_depth=8, seed=2), want_diag=False)
    ins = [rt.DeviceBuffer(ctx).upload(ref[k]) for k in ("color", "normal", "albedo")]
    ref_color = combine(ins)[0]
    for b in ins:
        b.free()
    return frames, ref_color


def error_ratio(den, noisy, ref):
    base = float(np.mean((noisy.astype(np.float64) - ref) ** 2))
    return float(np.mean((den.astype(np.float64) - ref) ** 2)) / base


def test_quality_on_a_noisy_and_a_clean_cover_frame(rt, gpu_context):
    """ONE parameter set (the recommended one) on a 4 x 1 spp and a 16 x 4 spp frame: the squared error against 1024 spp is at most half the noisy frame's at
    4 spp - the bound the project puts on its denoiser - and below the noisy frame's at 64 spp: a denoiser must not make a good frame worse.  The plain filter's
    ratios with its own recommended set are printed next to them.  Measured (profiles/r12_denoise_variance.json): 0.479 and 0.811; the plain filter 0.504
    and 1.798 on the same frames.  8 of the 96 points of the tuning grid meet both conditions."""
    ctx = gpu_context
    w, h = 192, 108
    frames, ref = quality_frames(rt, ctx, w, h)
    a = rt.abi
    new = (a.DENOISE_VARIANCE_DEFAULT_ITERATIONS, a.DENOISE_VARIANCE_DEFAULT_NORMAL_SHARPNESS, a.DENOISE_VARIANCE_DEFAULT_COLOR_SIGMA,
           a.DENOISE_VARIANCE_DEFAULT_ALBEDO_SIGMA, a.DENOISE_VARIANCE_DEFAULT_FLAGS, 0)
    old = (a.DENOISE_DEFAULT_ITERATIONS, a.DENOISE_DEFAULT_NORMAL_SHARPNESS, a.DENOISE_DEFAULT_COLOR_SIGMA, a.DENOISE_DEFAULT_ALBEDO_SIGMA, a.DENOISE_DEFAULT_FLAGS, 0)
    ratios = {}
    for name, (c, nrm, alb, m) in zip(("4x1", "16x4"), frames):
        den, _ = _device_outputs(rt, ctx, w, h, c, nrm, alb, m, new)
        assert np.isfinite(den).all()
        plain, _ = _device_outputs(rt, ctx, w, h, c, nrm, alb, m, old, plain=True)
        ratios[name] = (error_ratio(den, c, ref), error_ratio(plain, c, ref))
        print("denoise quality at %s spp: variance-guided / noisy %.4f, plain / noisy %.4f" % (name, *ratios[name]))
    assert ratios["4x1"][0] <= 0.5, ratios
    assert ratios["16x4"][0] < 1.0, ratios
