"""GPU: one long-lived context through a sequence of calls chosen so that every group of device blocks the context owns (csrc/rtow_context.h, rtow_device_mem.h) is
allocated, regrown, and reused while larger than the call needs.  After every step the outputs equal, bit for bit (uint32 views, diagnostics included), what a
fresh context produces for that step alone: what a context holds from earlier calls is scheduling state and capacity, never a result.  Every call must succeed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
KEYS = ("color", "normal", "albedo", "scw")
COMPS = (4, 3, 3, 1)


def _inputs(n):
    """non-zero accumulators to start from: the tie fix-up renders a marked pixel again from the launch's inputs, which an in-place launch overwrites"""
    rng = np.random.default_rng(11)
    return {k: rng.random(n * c, dtype=F) for k, c in zip(KEYS, COMPS)}


def _device(rt, ctx, plist, mode):
    """`single` (rtowSampleBatchDevice), `chain` (both in place) or `group` (own outputs per batch) from the same inputs, one diagnostics buffer per batch"""
    n = int(plist[0].size.x) * int(plist[0].size.y)
    words = plist[0].diagnosticsStride // 4
    start = _inputs(n)
    bufs = [rt.DeviceBuffer(ctx).upload(start[k]) for k in KEYS]
    diags = [rt.DeviceBuffer(ctx, n * words * 4).zero() for _ in plist]
    outs = [[rt.DeviceBuffer(ctx, n * c * 4).zero() for c in COMPS] for _ in plist] if mode == "group" else [bufs]
    try:
        if mode == "single":
            job = rt.SampleBatchJob(ctx, plist[0])
            job.InputColor, job.InputNormal, job.InputAlbedo, job.InputSampleCountWeight = bufs
            job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = bufs
            job.OutputDiagnostics = diags[0]
            rc = job.Schedule().Complete()
        elif mode == "chain":
            rc = rt.sample_batch_chain_device(ctx, plist, bufs, bufs, diags)
        else:
            rc = rt.sample_batch_group_device(ctx, plist, bufs, outs, diags)
        assert rc == rt.abi.RTOW_SUCCESS, (mode, rc)
        ctx.synchronize()
        got = {"%s%d" % (k, b): o[i].download(np.uint32, (n * c,)) for b, o in enumerate(outs) for i, (k, c) in enumerate(zip(KEYS, COMPS))}
        got.update({"diag%d" % b: d.download(np.uint32, (n * words,)) for b, d in enumerate(diags)})
        return got
    finally:
        for b in bufs + diags + ([x for o in outs for x in o] if mode == "group" else []):
            b.free()


def _host(rt, ctx, params):
    out = rt.sample_batch_host(ctx, params)                 # (raises unless RTOW_SUCCESS)
    return {k: np.ascontiguousarray(out[k]).view(np.uint32).reshape(-1) for k in KEYS + ("diag",)}


def _pixels(rt, ctx, params, capacity):
    """rtowSamplePixelsDevice in place over a host-made list of `capacity` scattered pixels"""
    n = int(params.size.x) * int(params.size.y)
    listed = np.zeros(4 + capacity, np.uint32)
    listed[0] = capacity
    listed[4:] = (np.arange(capacity, dtype=np.uint64) * 37 + 5) % n
    start = _inputs(n)
    bufs = [rt.DeviceBuffer(ctx).upload(start[k]) for k in KEYS]
    diag = rt.DeviceBuffer(ctx, n * params.diagnosticsStride).zero()
    lst = rt.DeviceBuffer(ctx).upload(listed)
    try:
        rc = rt.sample_pixels_device(ctx, [params], lst, capacity, bufs, bufs, [diag])
        assert rc == rt.abi.RTOW_SUCCESS, rc
        ctx.synchronize()
        got = {k: b.download(np.uint32, (n * c,)) for k, b, c in zip(KEYS, bufs, COMPS)}
        got["diag"] = diag.download(np.uint32, (n * params.diagnosticsStride // 4,))
        return got
    finally:
        for b in bufs + [diag, lst]:
            b.free()


def _queries(rt, ctx, scene):
    """trace_rays and shade_hits on 256 rays from around the camera into the scene (both raise unless RTOW_SUCCESS)"""
    rng = np.random.default_rng(5)
    rays = np.zeros((256, 8), F)
    rays[:, 0:3] = np.asarray(scene.camera["position"], F) + rng.uniform(-0.2, 0.2, (256, 3)).astype(F)
    aim = np.asarray(scene.camera["target"], F) + rng.uniform(-3.0, 3.0, (256, 3)).astype(F) - rays[:, 0:3]
    rays[:, 4:7] = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    hits = ctx.trace_rays(rays)
    assert (hits["entityIndex"] >= 0).any() and (hits["entityIndex"] < 0).any()       # hits and misses
    got = {k: np.ascontiguousarray(v).view(np.uint32).reshape(-1) for k, v in hits.items()}
    got.update({k: np.ascontiguousarray(v).view(np.uint32).reshape(-1) for k, v in ctx.shade_hits(rays, hits["entityIndex"]).items()})
    return got


def test_a_context_that_has_grown_computes_what_a_fresh_one_does(rt):
    S, a = rt.scenes, rt.abi
    scenes = {"row": S.twin_row_scene(30), "stack": S.volume_stack_scene(), "mesh1": S.mesh_scene(subdivisions=1), "mesh0": S.mesh_scene(subdivisions=0)}
    skies = {"sky16": S.synthetic_sky(size=16, half=True, seed=5), "sky32": S.synthetic_sky(size=32, half=True, seed=6)}

    def params(scene, w, h, spp=2, seed=1, **more):
        return S.make_params(scenes[scene], w, h, spp=spp, trace_depth=4, seed=seed, **more)

    def batch(scene, w, h, mode="single", count=1, spp=2, **more):
        return lambda ctx: _device(rt, ctx, [params(scene, w, h, spp, seed=1 + k, **more) for k in range(count)], mode)

    # (name, scene, upload it on the long-lived context first, sky: a name = upload, None = drop, "" = leave, the call)
    steps = [
        ("1 small frame, tie watch on", "row", True, "", batch("row", 64, 40)),
        ("2 larger frame, chain of 3: chunk order, hand-over state", "row", False, "", batch("row", 512, 128, "chain", 3, spp=1)),
        ("3 larger again, group of 2", "row", False, "", batch("row", 512, 192, "group", 2, spp=1)),
        ("4 small frame in blocks that are larger", "row", False, "", batch("row", 64, 40)),
        ("5 volume slabs: hit-spill area", "stack", True, "", batch("stack", 64, 40)),
        ("6 per-sample units, two groups per pixel", "stack", False, "", batch("stack", 64, 40, spp=32, rng_policy=a.RNG_PER_SAMPLE)),
        ("7a host buffers", "stack", False, "", lambda ctx: _host(rt, ctx, params("stack", 64, 40))),
        ("7b host buffers, larger", "stack", False, "", lambda ctx: _host(rt, ctx, params("stack", 96, 54))),
        ("8a smaller scene again, pixel list of 8", "row", True, "", lambda ctx: _pixels(rt, ctx, params("row", 64, 40), 8)),
        ("8b pixel list of 64", "row", False, "", lambda ctx: _pixels(rt, ctx, params("row", 64, 40), 64)),
        ("9a mesh: entity maps", "mesh1", True, "", lambda ctx: _queries(rt, ctx, scenes["mesh1"])),
        ("9b smaller mesh: maps allocated again", "mesh0", True, "", lambda ctx: _queries(rt, ctx, scenes["mesh0"])),
        ("10a cubemap", "mesh0", False, "sky16", batch("mesh0", 64, 40, sky_type=a.SKY_CUBEMAP)),
        ("10b cubemap dropped", "mesh0", False, None, batch("mesh0", 64, 40, sky_type=a.SKY_CUBEMAP)),
        ("10c larger cubemap", "mesh0", False, "sky32", batch("mesh0", 64, 40, sky_type=a.SKY_CUBEMAP)),
    ]

    def run(ctx, step, upload):
        name, scene, _, sky, call = step
        if upload:
            ctx.upload_scene(scenes[scene].desc())
        if sky != "":
            ctx.upload_sky_cubemap(skies[sky].desc() if sky else None)
        return call(ctx)

    fresh = {}
    for step in steps:                                    # the references first: each step alone in a context of its own
        with rt.Context(0) as ctx:
            fresh[step[0]] = run(ctx, step, True)
    assert any((fresh["10a cubemap"][k] != fresh["10b cubemap dropped"][k]).any() for k in ("color0",)), "the cubemap is not seen"

    def compare(got, name):
        want = fresh[name]
        assert sorted(got) == sorted(want), name
        for k in want:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), "step %s: %s differs from a fresh context's (%d words)" % (name, k, int((got[k] != want[k]).sum()))

    with rt.Context(0) as ctx:
        for step in steps:
            compare(run(ctx, step, step[2]), step[0])
    with rt.Context(0) as ctx:                            # 11: close, create, step 1 again
        compare(run(ctx, steps[0], True), steps[0][0])
