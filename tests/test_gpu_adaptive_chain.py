"""GPU: the adaptive schedule fed from the device (rtowSampleBatchChainAdaptiveDevice, include/rtow.h).

Each pixel picks its sample count from its accumulated weight against the frame's SampleCountWeightExtrema (JOBS/SampleBatchJob.cs:118-126), which the
ReduceMetricsJob of an earlier batch produced (UNITY/Raytracer.cs:527-543,742-751).  Defined result: for every batch k, rtowSampleBatchDevice with the extrema of
batch k - lag (the first `lag` batches: extremaIn, or their own parameters), then rtowReduceMetricsDevice over the whole W x H frame into extremaOut[k].  Every test
compares the call, bit for bit, with that sequence run from the host (accumulators, every batch's diagnostics, extremaOut), and one with the oracle."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))


def _bufs(rt, ctx, n, start=None):
    if start is None:
        return [rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS]
    return [rt.DeviceBuffer(ctx).upload(np.ascontiguousarray(start[k], dtype=np.float32)) for k, _ in KEYS]


def _download(bufs, n):
    return {k: b.download(np.float32, (n, c)) for (k, c), b in zip(KEYS, bufs)}


def _start(n, seed=3):
    rng = np.random.default_rng(seed)
    s = {"color": rng.random((n, 4)).astype(np.float32), "normal": rng.normal(size=(n, 3)).astype(np.float32),
         "albedo": rng.random((n, 3)).astype(np.float32), "scw": (rng.random(n) * 6).astype(np.float32)}
    s["color"][:, 3] = rng.integers(1, 5, n)
    return s


def _with_extrema(rt, p, e):
    q = rt.abi.SampleParams.from_buffer_copy(p)
    q.sampleCountWeightExtrema = rt.abi.Float2(*e)
    return q


def _reference(rt, ctx, plist, lag, extrema_in=None, start=None, diag_mask=None):
    """The defined result: one rtowSampleBatchDevice per batch with host-fed extrema, each followed by rtowReduceMetricsDevice over the frame."""
    lib = rt.lib.load()
    w, h = int(plist[0].size.x), int(plist[0].size.y)
    n, stride = w * h, plist[0].diagnosticsStride
    bufs = _bufs(rt, ctx, n, start)
    scratch = rt.DeviceBuffer(ctx, n * stride).zero()          # the reduction's record buffer for batches without diagnostics
    diags, ext = [], []
    for k, p in enumerate(plist):
        if k < lag:
            e = tuple(extrema_in[k]) if extrema_in is not None else (p.sampleCountWeightExtrema.x, p.sampleCountWeightExtrema.y)
        else:
            e = ext[k - lag]
        d = rt.DeviceBuffer(ctx, n * stride).zero() if diag_mask is None or diag_mask[k] else None
        job = rt.SampleBatchJob(ctx, _with_extrema(rt, p, e))
        job.InputColor, job.InputNormal, job.InputAlbedo, job.InputSampleCountWeight = bufs
        job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = bufs
        job.OutputDiagnostics = d
        assert job.Schedule().Complete() == 0
        m = rt.abi.Metrics()
        rt.lib.check(lib.rtowReduceMetricsDevice(ctx.handle, n, (d or scratch).ptr, stride, bufs[0].ptr, bufs[3].ptr, None, C.byref(m)), "rtowReduceMetricsDevice")
        ext.append((m.sampleCountWeightExtrema.x, m.sampleCountWeightExtrema.y))
        diags.append(d)
    ctx.synchronize()
    out = _download(bufs, n)
    out["diag"] = [d.download(np.float32, (n, stride // 4)) if d is not None else None for d in diags]
    out["ext"] = np.array(ext, np.float32)
    for b in bufs + [d for d in diags if d is not None] + [scratch]:
        b.free()
    return out


def _fed(rt, ctx, plist, lag, extrema_in=None, start=None, diag_mask=None, calls=1):
    """The entry point under test: `calls` consecutive calls over the batches, each continuing the schedule through extremaIn."""
    w, h = int(plist[0].size.x), int(plist[0].size.y)
    n, stride, count = w * h, plist[0].diagnosticsStride, len(plist)
    bufs = _bufs(rt, ctx, n, start)
    diags = [rt.DeviceBuffer(ctx, n * stride).zero() if diag_mask is None or diag_mask[k] else None for k in range(count)]
    ext_out = rt.DeviceBuffer(ctx).upload(np.full((count, 2), np.nan, np.float32))     # every entry must be written
    ext_in = rt.DeviceBuffer(ctx).upload(np.asarray(extrema_in, np.float32)) if extrema_in is not None else None
    per = count // calls
    for c in range(calls):
        lo = c * per
        hi = count if c == calls - 1 else lo + per
        src = ext_in.ptr if (c == 0 and ext_in is not None) else (None if c == 0 else ext_out.ptr + 8 * (lo - lag))
        assert rt.sample_batch_chain_adaptive_device(ctx, plist[lo:hi], bufs, bufs, ext_out.ptr + 8 * lo, lag=lag, extrema_in=src, diags=diags[lo:hi]) == 0
    ctx.synchronize()
    out = _download(bufs, n)
    out["diag"] = [d.download(np.float32, (n, stride // 4)) if d is not None else None for d in diags]
    out["ext"] = ext_out.download(np.float32, (count, 2))
    for b in bufs + [d for d in diags if d is not None] + [ext_out] + ([ext_in] if ext_in is not None else []):
        b.free()
    return out


def _same(a, b, what):
    for k, _ in KEYS:
        x, y = a[k].view(np.uint32), b[k].view(np.uint32)
        assert np.array_equal(x, y), (what, k, int((x != y).any(axis=-1).sum()))
    assert np.array_equal(a["ext"].view(np.uint32), b["ext"].view(np.uint32)), (what, "extremaOut", a["ext"].tolist(), b["ext"].tolist())
    assert len(a["diag"]) == len(b["diag"])
    for i, (x, y) in enumerate(zip(a["diag"], b["diag"])):
        assert (x is None) == (y is None), (what, "diagnostics of batch", i)
        if x is not None:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (what, "diagnostics of batch", i)


def _adaptive(rt, scene, w, h, depth, lo, hi, seeds, **kw):
    return [rt.scenes.make_params(scene, w, h, spp=lo, spp_max=hi, trace_depth=depth, seed=s, **kw) for s in seeds]


def _spread(rt, ctx, res):
    """The extrema must actually steer the schedule: a frame whose batches all took one count would prove nothing."""
    assert (res["ext"][:, 1] > res["ext"][:, 0]).any(), res["ext"].tolist()


@pytest.mark.parametrize("lag", [1, 2, 3, 6, 9])
@pytest.mark.parametrize("given", [False, True])
def test_fed_extrema_equal_the_host_fed_sequence(rt, gpu_context, lag, given):
    scene = rt.scenes.cover_scene()
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    plist = _adaptive(rt, scene, 200, 120, 8, 1, 9, [40 + k for k in range(6)], diagnostics_stride=16)
    ext_in = [(0.3 + 0.1 * k, 1.5 + 0.25 * k) for k in range(lag)] if given else None
    ref = _reference(rt, ctx, plist, lag, ext_in)
    got = _fed(rt, ctx, plist, lag, ext_in)
    _same(got, ref, ("lag", lag, "extremaIn", given))
    _spread(rt, ctx, ref)


def test_more_batches_than_one_launch_and_calls_chained_through_extrema_in(rt, gpu_context):
    scene = rt.scenes.cover_scene()
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    plist = _adaptive(rt, scene, 160, 96, 8, 1, 9, [200 + k for k in range(20)], diagnostics_stride=16)
    ref = _reference(rt, ctx, plist, 2)
    _same(_fed(rt, ctx, plist, 2), ref, "one call of 20")
    _same(_fed(rt, ctx, plist, 2, calls=2), ref, "two calls of 10")


def _tie_scene(rt, behind):
    # two spheres mirrored about x = 0 in front of a row the centre column threads (tests/test_gpu_ties.py): the rank-rule kernels list those pixels for the fix-up launch
    S = rt.scenes
    s = S.Scene("mirrored pair in front of a row")
    s.add_sphere((-0.3, 0.0, 5.0), 0.5, S.lambertian((0.9, 0.1, 0.1)))
    s.add_sphere((0.3, 0.0, 5.0), 0.5, S.metal((0.2, 0.9, 0.3), 0.0))
    for k in range(behind):
        s.add_sphere((0.0, 0.0, 3.5 - 1.0 * k), 0.3, S.lambertian((0.2 + 0.03 * k, 0.4, 0.8 - 0.03 * k)))
    s.camera = {"position": [0.0, 0.0, 10.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 12.0, "aperture": 0.0}
    return s


@pytest.mark.parametrize("flags", [0, "exact"])
def test_scenes_with_tied_pixels(rt, flags):
    f = rt.abi.CONTEXT_EXACT_TIES_ALWAYS if flags == "exact" else 0
    scene = _tie_scene(rt, 20)
    w = h = 33
    n = w * h
    with rt.Context(0, flags=f) as ctx:
        ctx.upload_scene(scene.desc())
        plist = _adaptive(rt, scene, w, h, 6, 1, 7, [61, 62, 63, 64, 65], jitter=False, focus=5.0, diagnostics_stride=16)
        start = _start(n)
        ref = _reference(rt, ctx, plist, 2, start=start)
        _same(_fed(rt, ctx, plist, 2, start=start), ref, ("tie scene", flags))


def test_sliced_frame_reduces_the_rows_it_does_not_own(rt, gpu_context):
    scene = rt.scenes.cover_scene()
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    w, h = 96, 60
    n = w * h
    start = _start(n, seed=5)
    start["scw"][0] = 1000.0                      # row 0 is not owned (0 % 3 != 1): the frame's maximum weight lies in a row no batch writes
    start["color"][0, 3] = 1.0
    plist = _adaptive(rt, scene, w, h, 8, 1, 9, [71, 72, 73, 74], slice_offset=1, slice_divider=3, diagnostics_stride=16)
    ref = _reference(rt, ctx, plist, 2, start=start)
    assert (ref["ext"][:, 1] == np.float32(1000.0)).all()
    _same(_fed(rt, ctx, plist, 2, start=start), ref, "sliced")


def test_fallbacks_per_sample_policy_no_fusion_and_partial_diagnostics(rt, gpu_context):
    scene = rt.scenes.cover_scene()
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    plist = _adaptive(rt, scene, 128, 72, 8, 1, 40, [81, 82, 83, 84], rng_policy=rt.abi.RNG_PER_SAMPLE)
    _same(_fed(rt, ctx, plist, 2), _reference(rt, ctx, plist, 2), "per-sample policy")
    plist = _adaptive(rt, scene, 128, 72, 8, 1, 9, [91, 92, 93, 94, 95], diagnostics_stride=16)
    mask = [True, False, True, False, True]
    _same(_fed(rt, ctx, plist, 2, diag_mask=mask), _reference(rt, ctx, plist, 2, diag_mask=mask), "diagnostics on some batches")
    with rt.Context(0, flags=rt.abi.CONTEXT_NO_CHAIN_FUSION) as c2:
        c2.upload_scene(scene.desc())
        _same(_fed(rt, c2, plist, 2), _reference(rt, c2, plist, 2), "no chain fusion")


def test_full_frame_at_the_hosts_depth(rt):
    scene = rt.scenes.cover_scene()
    with rt.Context(0, flags=rt.abi.CONTEXT_EXACT_TIES_ALWAYS) as ctx:
        ctx.upload_scene(scene.desc())
        plist = _adaptive(rt, scene, 1920, 1080, 32, 1, 50, [301, 302, 303, 304], diagnostics_stride=16)
        ref = _reference(rt, ctx, plist, 2)
        _same(_fed(rt, ctx, plist, 2), ref, "1920 x 1080, depth 32, {1, 50}")
        _spread(rt, ctx, ref)


def test_oracle_with_numpy_fed_extrema(rt, gpu_context, oracle):
    scene = rt.scenes.cover_scene()
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    w, h, lag = 48, 27, 2
    n = w * h
    plist = _adaptive(rt, scene, w, h, 8, 1, 9, [111, 112, 113, 114], diagnostics_stride=4)
    osc = oracle.OracleScene(scene.desc())
    acc = {"color": np.zeros((n, 4), np.float32), "normal": np.zeros((n, 3), np.float32), "albedo": np.zeros((n, 3), np.float32), "scw": np.zeros(n, np.float32)}
    ext, rays = [], []
    for k, p in enumerate(plist):
        e = (p.sampleCountWeightExtrema.x, p.sampleCountWeightExtrema.y) if k < lag else ext[k - lag]
        r = osc.sample_batch(_with_extrema(rt, p, e), acc)
        acc = {key: r[key] for key, _ in KEYS}
        rays.append(r["diag"][:, 0].copy())
        with np.errstate(divide="ignore", invalid="ignore"):
            wgt = acc["scw"].reshape(n) / acc["color"][:, 3].astype(np.int32).astype(np.float32)
        live = wgt[~np.isnan(wgt)]                # math.min / math.max keep the first operand when the second is NaN (the fold starts at +inf / -inf)
        ext.append((np.float32(live.min()) if live.size else np.float32(np.inf), np.float32(live.max()) if live.size else np.float32(-np.inf)))
    osc.close()
    got = _fed(rt, ctx, plist, lag)
    for key, c in KEYS:
        assert np.array_equal(got[key].view(np.uint32), acc[key].reshape(n, c).view(np.uint32)), key
    assert np.array_equal(got["ext"].view(np.uint32), np.array(ext, np.float32).view(np.uint32)), (got["ext"].tolist(), ext)
    for k in range(len(plist)):
        assert np.array_equal(got["diag"][k][:, 0], rays[k]), ("RayCount of batch", k)


def test_invalid_arguments_leave_the_buffers_untouched(rt, gpu_context):
    scene = rt.scenes.cover_scene()
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    lib = rt.lib.load()
    w, h = 64, 32
    n = w * h
    start = _start(n, seed=9)
    bufs = _bufs(rt, ctx, n, start)
    sentinel = np.full((3, 2), 7.0, np.float32)
    ext_out = rt.DeviceBuffer(ctx).upload(sentinel)
    good = _adaptive(rt, scene, w, h, 4, 1, 5, [1, 2, 3], diagnostics_stride=16)
    diags = [rt.DeviceBuffer(ctx, n * 16).zero() for _ in good]
    dptr = (C.c_void_p * 3)(*[d.ptr for d in diags])
    bi = rt.abi.AccumBuffers(*[b.ptr for b in bufs])

    def call(plist, feed):
        arr = (rt.abi.SampleParams * len(plist))(*plist)
        return lib.rtowSampleBatchChainAdaptiveDevice(ctx.handle, len(plist), arr, C.byref(bi), C.byref(bi), dptr, C.byref(feed) if feed is not None else None, None, None)

    F = rt.abi.AdaptiveFeed
    bad_size = list(good)
    bad_size[1] = rt.scenes.make_params(scene, w, h + 1, spp=1, spp_max=5, trace_depth=4, seed=2, diagnostics_stride=16)
    bad_slice = list(good)
    bad_slice[2] = rt.scenes.make_params(scene, w, h, spp=1, spp_max=5, trace_depth=4, seed=3, slice_offset=0, slice_divider=2, diagnostics_stride=16)
    bad_stride = list(good)
    bad_stride[1] = rt.scenes.make_params(scene, w, h, spp=1, spp_max=5, trace_depth=4, seed=2, diagnostics_stride=4)
    cases = [("lag 0", good, F(None, ext_out.ptr, 0, 0)), ("lag -1", good, F(None, ext_out.ptr, -1, 0)), ("no extremaOut", good, F(None, None, 2, 0)),
             ("reserved", good, F(None, ext_out.ptr, 2, 1)), ("no feed", good, None), ("size", bad_size, F(None, ext_out.ptr, 2, 0)),
             ("slice", bad_slice, F(None, ext_out.ptr, 2, 0)), ("diagnosticsStride", bad_stride, F(None, ext_out.ptr, 2, 0))]
    for what, plist, feed in cases:
        assert call(plist, feed) == rt.abi.RTOW_ERROR_INVALID_VALUE, what
    ctx.synchronize()
    after = _download(bufs, n)
    for key, c in KEYS:
        assert np.array_equal(after[key].view(np.uint32), start[key].reshape(n, c).view(np.uint32)), key
    assert np.array_equal(ext_out.download(np.float32, (3, 2)), sentinel)
    for d in diags:
        assert not d.download(np.float32, (n, 4)).any()
    assert call(good, F(None, ext_out.ptr, 2, 0)) == 0          # the same buffers with a valid feed do run
    ctx.synchronize()
    for b in bufs + diags + [ext_out]:
        b.free()


def test_first_batches_with_their_own_different_extrema(rt, gpu_context):
    """extremaIn NULL and the first `lag` batches carrying different extrema of their own: a fused launch reads one parameter block's, so those batches must not share one."""
    scene = rt.scenes.cover_scene()
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    plist = _adaptive(rt, scene, 128, 72, 8, 1, 9, [121, 122, 123, 124, 125, 126, 127], diagnostics_stride=16)
    for k, e in enumerate([(0.2, 1.1), (0.5, 2.5), (0.1, 0.9)]):
        plist[k].sampleCountWeightExtrema = rt.abi.Float2(*e)
    _same(_fed(rt, ctx, plist, 3), _reference(rt, ctx, plist, 3), "own extrema, lag 3")


@pytest.mark.parametrize("lag", [3, 4])
def test_tied_pixels_in_longer_fused_launches(rt, gpu_context, lag):
    """The default context's fix-up launch carries listed pixels through 3 and 4 fused batches and folds them into every batch's extrema."""
    scene = _tie_scene(rt, 20)
    w = h = 33
    n = w * h
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    plist = _adaptive(rt, scene, w, h, 6, 1, 7, [131 + k for k in range(9)], jitter=False, focus=5.0, diagnostics_stride=16)
    start = _start(n, seed=11)
    _same(_fed(rt, ctx, plist, lag, start=start), _reference(rt, ctx, plist, lag, start=start), ("tie scene", lag))
