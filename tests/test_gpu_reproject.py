"""GPU tests of rtowReprojectAccumDevice (include/rtow.h): the kernel bit for bit against the numpy restatement of its specification
(tests/reproject_reference.py) on synthetic inputs that need no scene, guard words, refusals, determinism, and the end-to-end gain on the cover scene.
All in the session context, no subprocesses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_reference as rr  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (8, 8), (9, 7), (41, 29), (96, 54), (257, 3)]
# (flags, depthTolerance, maxHistory): both flag values with each tolerance
CONFIGS = [(1, 0.0, 64), (0, 0.0, 7), (1, 0.01, 64), (0, 0.01, 1), (1, 1.0, 1000), (0, 1.0, 64)]
PLANE_Z, PLANE_ENTITY = -2.0, 3
GUARD = 0x5AFEC0DE
KEYS = ("color", "normal", "albedo", "scw")


def _views(w, h, seed):
    """two views a small step apart"""
    rng = np.random.default_rng(seed)
    pos = np.array([0.3, 1.2, 6.0]) + rng.uniform(-0.5, 0.5, 3)
    step = rng.uniform(-1, 1, 3) * np.array([0.12, 0.06, 0.2])
    target = np.array([0.0, 0.5, 0.0])
    return rr.make_view(tuple(pos), tuple(target), w, h), rr.make_view(tuple(pos + step), tuple(target + step * 0.5), w, h)


def _plane(o, d):
    with np.errstate(all="ignore"):
        return ((F(PLANE_Z) - o[:, 2]) / d[:, 2]).astype(F)


def _sky_block(w, h, n, variant):
    """a contiguous block of sky: the part of the frame beyond a diagonal (any aspect ratio); a frame of one pixel is sky in two variants of three"""
    if n == 1:
        return np.array([variant % 3 != 0])
    cx, cy = np.tile(np.arange(w), h), np.repeat(np.arange(h), w)
    return (cx + 0.5) / w + (cy + 0.5) / h > 1.05


def make_case(w, h, seed, max_history, variant=0):
    """Inputs of one call: previous view A, new view B.  Hits mix a plane both views see consistently, random distances and entities, scattered misses (-1, +inf),
    a block of sky, distances that put the point behind the previous camera, and rays that project exactly onto fx == 0 and just around fx == W; the
    accumulators mix w of 0, 0.5, 1, maxHistory, maxHistory + 1 and 10^6 with NaN and +-inf in a channel."""
    rng = np.random.default_rng(seed)
    n = w * h
    a, b = _views(w, h, seed)
    va = rr.view_arrays(a)
    oa, da = rr.pixel_centre_rays(a, w, h)
    o, d = rr.pixel_centre_rays(b, w, h)

    def hits(org, dirs, block):
        t = _plane(org, dirs)
        e = np.full(n, PLANE_ENTITY, np.int32)
        kind = rng.random(n)
        rnd = kind < 0.15
        t[rnd] = np.exp(rng.uniform(np.log(0.01), np.log(1000.0), int(rnd.sum()))).astype(F)
        e[rnd] = rng.integers(0, 6, int(rnd.sum()))
        miss = (kind >= 0.15) & (kind < 0.22)
        t[miss | block], e[miss | block] = np.inf, -1
        return t, e, kind

    pt, pe, _ = hits(oa, da, _sky_block(w, h, n, variant))
    t, e, kind = hits(o, d, _sky_block(w, h, n, variant))
    behind = (kind >= 0.22) & (kind < 0.27) & (e >= 0)
    t[behind] = -t[behind]                                           # the far side of both cameras: s < 0
    if n >= 64:                                                      # rays aimed at the previous view's image-plane edges, as sky (w = d exactly) and as hits
        llc, hz = va["lowerLeftCorner"], va["horizontal"]
        edges = [llc, llc * F(2)] + [(llc + hz * F(1 + k * 2.0 ** -22)).astype(F) for k in (-3, -1, 0, 1, 3)] + [(llc - hz * F(2.0 ** -20)).astype(F)]
        at = rng.choice(n, 2 * len(edges), replace=False)
        for j, i in enumerate(at):
            d[i] = edges[j % len(edges)]
            if j < len(edges):
                t[i], e[i] = np.inf, -1
            else:
                o[i], t[i], e[i] = va["origin"], F(1), PLANE_ENTITY
    mh = float(max_history)
    weights = np.array([0, 0.5, 1, mh, mh + 1, 1e6], F)
    wsel = weights[rng.choice(6, n, p=[0.06, 0.06, 0.22, 0.22, 0.22, 0.22])]
    prev = {"color": np.concatenate([rng.uniform(0, 3, (n, 3)) * wsel[:, None], wsel[:, None]], axis=1).astype(F),
            "normal": (rng.normal(size=(n, 3)) * wsel[:, None]).astype(F), "albedo": (rng.uniform(0, 1, (n, 3)) * wsel[:, None]).astype(F),
            "scw": (rng.uniform(0, 2, n) * wsel).astype(F)}
    for val in (np.nan, np.inf, -np.inf):
        idx = rng.integers(0, n, max(1, n // 61) if n > 1 else int(rng.random() < 0.1))
        prev["color"][idx, rng.integers(0, 4, idx.size)] = val
    prev["normal"][rng.integers(0, n, max(1, n // 97)), 1] = np.nan   # carried as it is: only the colour decides
    rays = np.zeros(n, np.dtype([("origin", "<f4", (3,)), ("time", "<f4"), ("direction", "<f4", (3,)), ("pad", "<f4")]))
    rays["origin"], rays["direction"], rays["time"], rays["pad"] = o, d, rng.random(n), rng.random(n)      # time and pad are ignored
    return {"w": w, "h": h, "n": n, "view": a, "va": va, "o": o, "d": d, "rays": rays, "t": t, "e": e, "pt": pt, "pe": pe, "prev": prev}


def reference(case, flags, tol, max_history):
    return rr.reproject(case["w"], case["h"], case["va"], case["o"], case["d"], case["t"], case["e"], case["pt"], case["pe"], case["prev"], tol, max_history, flags)


class Dev:
    """a device array `offset` bytes into its allocation, with guard words before and after it"""

    def __init__(self, rt, ctx, nbytes, offset=0, data=None):
        self.rt, self.ctx, self.nbytes, self.front = rt, ctx, nbytes, 16 + offset
        self.buf = rt.DeviceBuffer(ctx, self.front + nbytes + 16)
        host = np.full((self.front + nbytes + 16) // 4, GUARD, np.uint32)
        if data is not None:
            host[self.front // 4: (self.front + nbytes) // 4] = np.ascontiguousarray(data).view(np.uint32).ravel()
        self.buf.upload(host)

    @property
    def ptr(self):
        return self.buf.ptr + self.front

    def words(self):
        return self.buf.download(np.uint32, ((self.front + self.nbytes + 16) // 4,))

    def download(self, dtype, shape):
        return self.words()[self.front // 4: (self.front + self.nbytes) // 4].view(dtype).reshape(shape)

    def guards_intact(self):
        x = self.words()
        return (x[: self.front // 4] == GUARD).all() and (x[(self.front + self.nbytes) // 4:] == GUARD).all()

    def free(self):
        self.buf.free()


class Call:
    """the fifteen device buffers of one call"""

    def __init__(self, rt, ctx, case, offset=0, source=True):
        n = case["n"]
        self.rt, self.ctx, self.case = rt, ctx, case
        mk = lambda data: Dev(rt, ctx, np.ascontiguousarray(data).nbytes, offset, data)
        self.ins = {"rays": mk(case["rays"]), "t": mk(case["t"]), "e": mk(case["e"]), "pt": mk(case["pt"]), "pe": mk(case["pe"])}
        self.prev = {k: mk(case["prev"][k]) for k in KEYS}
        self.out = {"color": Dev(rt, ctx, n * 16, offset), "normal": Dev(rt, ctx, n * 12, offset), "albedo": Dev(rt, ctx, n * 12, offset), "scw": Dev(rt, ctx, n * 4, offset)}
        self.src = Dev(rt, ctx, n * 4, offset)
        self.with_source = source

    def run(self, flags, tol, max_history, stream=None, **over):
        a, c = self.rt.abi, self.case
        p = a.ReprojectParams(over.get("w", c["w"]), over.get("h", c["h"]), over.get("view", c["view"]), tol, max_history, flags, over.get("reserved", 0))
        ptr = {"rays": self.ins["rays"].ptr, "t": self.ins["t"].ptr, "e": self.ins["e"].ptr, "pt": self.ins["pt"].ptr, "pe": self.ins["pe"].ptr,
               "src": self.src.ptr if self.with_source else None}
        ptr.update({"p" + k: self.prev[k].ptr for k in KEYS})
        ptr.update({"o" + k: self.out[k].ptr for k in KEYS})
        ptr.update({k: v for k, v in over.items() if k in ptr})
        hits, prev_hits = a.HitBuffers(ptr["t"], ptr["e"], None), a.HitBuffers(ptr["pt"], ptr["pe"], None)
        prev, out = a.AccumBuffers(*[ptr["p" + k] for k in KEYS]), a.AccumBuffers(*[ptr["o" + k] for k in KEYS])
        return self.rt.lib.load().rtowReprojectAccumDevice(self.ctx.handle, C.byref(p), ptr["rays"], C.byref(hits), C.byref(prev_hits), C.byref(prev), C.byref(out),
                                                           ptr["src"], stream)

    def results(self):
        n = self.case["n"]
        self.ctx.synchronize()
        shapes = {"color": (n, 4), "normal": (n, 3), "albedo": (n, 3), "scw": (n,)}
        return {k: self.out[k].download(F, shapes[k]) for k in KEYS}, self.src.download(np.int32, (n,))

    def everything(self):
        return list(self.ins.values()) + list(self.prev.values()) + list(self.out.values()) + [self.src]

    def free(self):
        for b in self.everything():
            b.free()


def _compare(got, got_src, want, want_src, what):
    bad = np.flatnonzero(got_src.view(np.uint32) != want_src.view(np.uint32))
    assert bad.size == 0, (what, "source", bad[:5], got_src[bad[:5]], want_src[bad[:5]])
    for k in KEYS:
        x, y = got[k].reshape(got_src.size, -1).view(np.uint32), want[k].reshape(got_src.size, -1).view(np.uint32)
        bad = np.flatnonzero((x != y).any(1))
        assert bad.size == 0, (what, k, bad[:5], got[k][bad[:3]], want[k][bad[:3]])


def _check(rt, ctx, w, h, seed, cfg, offset, variant=0):
    flags, tol, max_history = cfg
    case = make_case(w, h, seed, max_history, variant)
    want, want_src = reference(case, flags, tol, max_history)
    carried = int((want_src >= 0).sum())
    call = Call(rt, ctx, case, offset)
    try:
        assert call.run(flags, tol, max_history) == rt.abi.RTOW_SUCCESS
        got, got_src = call.results()
        _compare(got, got_src, want, want_src, ((w, h), cfg, offset, variant))
        for b in call.everything():
            assert b.guards_intact()
    finally:
        call.free()
    return carried


@pytest.mark.parametrize("w,h", SIZES)
def test_bit_exact_against_the_restatement(rt, gpu_context, w, h):
    """Every configuration at every size, buffers 4 bytes into their allocations in every other case.  In each generated case the restatement carries between
    20 % and 80 % of the pixels, so that both branches are exercised - a frame of one pixel cannot, so that size runs ten variants per configuration and the
    condition holds over them together."""
    n = w * h
    for k, cfg in enumerate(CONFIGS):
        variants = range(10) if n == 1 else range(1)
        carried = [_check(rt, gpu_context, w, h, 1000 * w + 10 * h + k + 65537 * v, cfg, 4 if k % 2 else 0, v) for v in variants]
        share = sum(carried) / (n * len(carried))
        print("reproject %dx%d %s: carried %.3f" % (w, h, cfg, share))
        assert 0.2 <= share <= 0.8, ((w, h), cfg, share)


def test_bit_exact_at_1080p(rt, gpu_context):
    w, h = 1920, 1080
    carried = _check(rt, gpu_context, w, h, 7, CONFIGS[2], 4)
    assert 0.2 <= carried / (w * h) <= 0.8, carried / (w * h)


def test_without_out_source_nothing_is_written_there(rt, gpu_context):
    flags, tol, max_history = CONFIGS[2]
    case = make_case(41, 29, 5, max_history)
    want, _ = reference(case, flags, tol, max_history)
    call = Call(rt, gpu_context, case, 4, source=False)
    try:
        assert call.run(flags, tol, max_history) == rt.abi.RTOW_SUCCESS
        got, _ = call.results()
        for k in KEYS:
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), k
        assert (call.src.words() == GUARD).all()                      # the array a call WITH outSource would have written
        for b in call.everything():
            assert b.guards_intact()
    finally:
        call.free()


def test_refusals_enqueue_nothing(rt, gpu_context):
    flags, tol, max_history = CONFIGS[2]
    case = make_case(16, 8, 3, max_history)
    n = case["n"]
    bad = rt.abi.RTOW_ERROR_INVALID_VALUE
    call = Call(rt, gpu_context, case)
    try:
        names = ["rays", "t", "e", "pt", "pe"] + ["p" + k for k in KEYS] + ["o" + k for k in KEYS]
        for name in names:
            assert call.run(flags, tol, max_history, **{name: None}) == bad, name
        lib, a = rt.lib.load(), rt.abi
        p = a.ReprojectParams(16, 8, case["view"], tol, max_history, flags, 0)
        hb, ab = a.HitBuffers(call.ins["t"].ptr, call.ins["e"].ptr, None), a.AccumBuffers(*[call.out[k].ptr for k in KEYS])
        pb = a.AccumBuffers(*[call.prev[k].ptr for k in KEYS])
        for args in ((None, C.byref(p), call.ins["rays"].ptr, C.byref(hb), C.byref(hb), C.byref(pb), C.byref(ab)),
                     (gpu_context.handle, None, call.ins["rays"].ptr, C.byref(hb), C.byref(hb), C.byref(pb), C.byref(ab)),
                     (gpu_context.handle, C.byref(p), call.ins["rays"].ptr, None, C.byref(hb), C.byref(pb), C.byref(ab)),
                     (gpu_context.handle, C.byref(p), call.ins["rays"].ptr, C.byref(hb), None, C.byref(pb), C.byref(ab)),
                     (gpu_context.handle, C.byref(p), call.ins["rays"].ptr, C.byref(hb), C.byref(hb), None, C.byref(ab)),
                     (gpu_context.handle, C.byref(p), call.ins["rays"].ptr, C.byref(hb), C.byref(hb), C.byref(pb), None)):
            assert lib.rtowReprojectAccumDevice(*args, call.src.ptr, None) == bad
        for size in ({"w": 0}, {"h": 0}, {"w": -1}, {"w": 65536, "h": 32768}):
            assert call.run(flags, tol, max_history, **size) == bad, size
        for f, t, m in ((flags, -0.01, 64), (flags, float("nan"), 64), (flags, float("inf"), 64), (flags, tol, 0), (flags, tol, -3), (2, tol, 64), (3, tol, 64), (-1, tol, 64)):
            assert call.run(f, t, m) == bad, (f, t, m)
        assert call.run(flags, tol, max_history, reserved=1) == bad
        flat, nan_view, sideways = rt.abi.View(), rr.make_view((0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 16, 8), rr.make_view((0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 16, 8)
        nan_view.vertical.y = float("inf")
        sideways.horizontal = sideways.up                              # HR = dot(up, right) = 0 (or a rounding error's worth of it, which must then be finite and non-zero)
        assert call.run(flags, tol, max_history, view=flat) == bad and call.run(flags, tol, max_history, view=nan_view) == bad
        hr = rr.view_constants(rr.view_arrays(sideways))[3]
        if hr == 0:
            assert call.run(flags, tol, max_history, view=sideways) == bad
        # an output on a buffer the pass gathers from, or on another output; partial overlaps by one element
        for over in ({"ocolor": call.prev["color"].ptr}, {"onormal": call.prev["color"].ptr + n * 16 - 4}, {"oscw": call.prev["scw"].ptr + 4},
                     {"src": call.prev["albedo"].ptr}, {"oalbedo": call.ins["pt"].ptr}, {"src": call.ins["pe"].ptr + (n - 1) * 4},
                     {"onormal": call.out["color"].ptr + 8}, {"src": call.out["scw"].ptr}, {"oalbedo": call.out["normal"].ptr + n * 12 - 4}):
            assert call.run(flags, tol, max_history, **over) == bad, over
        gpu_context.synchronize()
        for b in list(call.out.values()) + [call.src]:
            assert (b.words() == GUARD).all()                         # nothing was enqueued
        assert call.run(flags, tol, max_history) == rt.abi.RTOW_SUCCESS
        got, got_src = call.results()
        want, want_src = reference(case, flags, tol, max_history)
        _compare(got, got_src, want, want_src, "after the refusals")
    finally:
        call.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    flags, tol, max_history = CONFIGS[2]
    case = make_case(320, 180, 9, max_history)
    res = []
    for _ in range(2):
        call = Call(rt, gpu_context, case)
        try:
            assert call.run(flags, tol, max_history) == rt.abi.RTOW_SUCCESS
            res.append(call.results())
        finally:
            call.free()
    for k in KEYS:
        assert np.array_equal(res[0][0][k].view(np.uint32), res[1][0][k].view(np.uint32)), k
    assert np.array_equal(res[0][1], res[1][1])


# the asserted bound of the end-to-end test: the ratio measured on an MI355X times 1.25 for seed-to-seed spread, never above 1
MEASURED_RATIO = 0.093
RATIO_BOUND = 1.0 if MEASURED_RATIO is None else min(1.0, 1.25 * MEASURED_RATIO)


def test_end_to_end_on_the_cover_scene(rt, gpu_context):
    """192 x 108: 64 spp at view A; the camera dollies 2 % of the way to its target (view B); trace-view A and B, reproject (recommended parameters), 4 spp at B
    on top of the result - against the same 4 spp at B from zeros, which is what a host gets today.  Both are combined on the device and compared with a
    1024-spp render at B: the reprojected frame's mean squared error must be below the restarted frame's, by the measured ratio times 1.25
    (measured on an MI355X: 0.093, 99 % of the pixels carried).
    At least half the pixels are carried, and every carried pixel's source shows the same entity in A."""
    ctx = gpu_context
    S = rt.scenes
    scene = S.cover_scene()
    ctx.upload_scene(scene.desc())
    w, h = 192, 108
    n = w * h
    pa = S.make_params(scene, w, h, spp=64, trace_depth=8, seed=1)
    cam = scene.camera
    position, target = np.asarray(cam["position"], np.float64), np.asarray(cam["target"], np.float64)
    moved = position + 0.02 * (target - position)
    focus = S.focus_distance(scene, np.asarray(cam["position"], F), S._normalize(np.asarray(cam["target"], F) - np.asarray(cam["position"], F)))
    view_b = rr.make_view(tuple(moved), tuple(target), w, h, vfov=cam["vfov"], focus=focus, up=tuple(cam["up"]))

    def at_b(spp, seed):
        p = S.make_params(scene, w, h, spp=spp, trace_depth=8, seed=seed)
        p.view = view_b
        p.view.lensRadius = pa.view.lensRadius
        return p

    acc_a = rt.sample_batch_host(ctx, pa, want_diag=False)
    hits_a = ctx.trace_view(pa.view, w, h, want=("distance", "entityIndex"))
    hits_b = ctx.trace_view(view_b, w, h, want=("distance", "entityIndex"), want_rays=True)
    bufs = []

    def up(x):
        bufs.append(rt.DeviceBuffer(ctx).upload(x))
        return bufs[-1]

    def room(nbytes):
        bufs.append(rt.DeviceBuffer(ctx, nbytes))
        return bufs[-1]

    try:
        job = rt.ReprojectJob(ctx, w, h, pa.view)
        job.Rays, job.HitDistance, job.HitEntityIndex = up(hits_b["rays"]), up(hits_b["distance"]), up(hits_b["entityIndex"])
        job.PreviousHitDistance, job.PreviousHitEntityIndex = up(hits_a["distance"]), up(hits_a["entityIndex"])
        job.PreviousColor, job.PreviousNormal, job.PreviousAlbedo, job.PreviousSampleCountWeight = [up(acc_a[k]) for k in KEYS]
        outs = [room(n * 16), room(n * 12), room(n * 12), room(n * 4)]
        job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = outs
        job.OutputSource = room(n * 4)
        assert job.Schedule().Complete() == 0
        ctx.synchronize()
        carried = {k: b.download(F, s) for k, b, s in zip(KEYS, outs, ((n, 4), (n, 3), (n, 3), (n,)))}
        src = job.OutputSource.download(np.int32, (n,))
        o, d = hits_b["rays"]["origin"], hits_b["rays"]["direction"]
        want, want_src = rr.reproject(w, h, rr.view_arrays(pa.view), o, d, hits_b["distance"], hits_b["entityIndex"], hits_a["distance"], hits_a["entityIndex"],
                                      acc_a, rt.abi.REPROJECT_DEFAULT_DEPTH_TOLERANCE, rt.abi.REPROJECT_DEFAULT_MAX_HISTORY, rt.abi.REPROJECT_DEFAULT_FLAGS)
        _compare(carried, src, want, want_src, "cover scene")
        got = src >= 0
        assert got.mean() >= 0.5, got.mean()
        assert np.array_equal(hits_a["entityIndex"][src[got]], hits_b["entityIndex"][got])
        assert carried["color"][:, 3].max() <= rt.abi.REPROJECT_DEFAULT_MAX_HISTORY

        frames = {"reprojected": rt.sample_batch_host(ctx, at_b(4, 5), inputs=carried, want_diag=False),
                  "restarted": rt.sample_batch_host(ctx, at_b(4, 5), want_diag=False),
                  "reference": rt.sample_batch_host(ctx, at_b(1024, 9), want_diag=False)}
        combined = {}
        for name, acc in frames.items():
            ins = [up(acc[k]) for k in ("color", "normal", "albedo")]
            res = [room(n * 12) for _ in range(3)]
            cj = rt.CombineJob(ctx, (w, h))
            cj.InputColor, cj.InputNormal, cj.InputAlbedo = ins
            cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = res
            assert cj.Schedule().Complete() == 0
            ctx.synchronize()
            combined[name] = res[0].download(F, (n, 3)).astype(np.float64)
    finally:
        for b in bufs:
            b.free()
    mse = {k: float(np.mean((combined[k] - combined["reference"]) ** 2)) for k in ("reprojected", "restarted")}
    ratio = mse["reprojected"] / mse["restarted"]
    print("reproject quality: carried %.4f of the pixels, restarted MSE %.6g, reprojected MSE %.6g, reprojected / restarted %.4f"
          % (got.mean(), mse["restarted"], mse["reprojected"], ratio))
    assert np.isfinite(combined["reprojected"]).all()
    assert ratio < 1.0 and ratio <= RATIO_BOUND, ratio
