"""GPU tests of rtowReprojectAccumBilinearDevice (include/rtow.h): the kernel bit for bit against the numpy restatement of its specification
(tests/reproject_bilinear_reference.py) on the synthetic inputs of tests/reproject_bilinear_cases.py, with and without moments, against
rtowReprojectAccumDevice on the same inputs, guard words, refusals, determinism, a captured graph, and the cover scene end to end.
All in the session context, no subprocesses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_bilinear_cases as bc  # noqa: E402
import reproject_bilinear_reference as rb  # noqa: E402
import reproject_reference as rr  # noqa: E402
from test_gpu_reproject import GUARD, KEYS, Call, Dev  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
CONFIGS = bc.CONFIGS


class BCall(Call):
    """the buffers of rtowReprojectAccumDevice's call plus the two moments buffers"""

    def __init__(self, rt, ctx, case, offset=0, source=True, moments=True):
        super().__init__(rt, ctx, case, offset, source)
        self.pm = Dev(rt, ctx, case["n"] * 12, offset, case["moments"])
        self.om = Dev(rt, ctx, case["n"] * 12, offset)
        self.with_moments = moments

    def run_bilinear(self, flags, tol, max_history, max_batches=16, stream=None, **over):
        a, c = self.rt.abi, self.case
        p = a.ReprojectParams(over.get("w", c["w"]), over.get("h", c["h"]), over.get("view", c["view"]), tol, max_history, flags, over.get("reserved", 0))
        ptr = {"rays": self.ins["rays"].ptr, "t": self.ins["t"].ptr, "e": self.ins["e"].ptr, "pt": self.ins["pt"].ptr, "pe": self.ins["pe"].ptr,
               "src": self.src.ptr if self.with_source else None, "pm": self.pm.ptr if self.with_moments else None,
               "om": self.om.ptr if self.with_moments else None}
        ptr.update({"p" + k: self.prev[k].ptr for k in KEYS})
        ptr.update({"o" + k: self.out[k].ptr for k in KEYS})
        ptr.update({k: v for k, v in over.items() if k in ptr})
        hits, prev_hits = a.HitBuffers(ptr["t"], ptr["e"], None), a.HitBuffers(ptr["pt"], ptr["pe"], None)
        prev, out = a.AccumBuffers(*[ptr["p" + k] for k in KEYS]), a.AccumBuffers(*[ptr["o" + k] for k in KEYS])
        return self.rt.lib.load().rtowReprojectAccumBilinearDevice(self.ctx.handle, C.byref(p), ptr["rays"], C.byref(hits), C.byref(prev_hits), C.byref(prev),
                                                                   C.byref(out), ptr["pm"], max_batches, ptr["om"], ptr["src"], stream)

    def moments(self):
        self.ctx.synchronize()
        return self.om.download(F, (self.case["n"], 3))

    def outputs(self):
        return list(self.out.values()) + [self.src, self.om]

    def everything(self):
        return super().everything() + [self.pm, self.om]


def _same_bits(got, want, what):
    x, y = got.reshape(got.shape[0], -1).view(np.uint32), want.reshape(want.shape[0], -1).view(np.uint32)
    bad = np.flatnonzero((x != y).any(1))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:3]], want[bad[:3]])


def _compare(call, want, want_src, want_m, what):
    got, got_src = call.results()
    _same_bits(got_src, want_src, (what, "source"))
    for k in KEYS:
        _same_bits(got[k], want[k], (what, k))
    if want_m is not None:
        _same_bits(call.moments(), want_m, (what, "moments"))
    else:
        assert (call.om.words() == GUARD).all(), (what, "moments written without being asked for")
    for b in call.everything():
        assert b.guards_intact(), what


def _check(rt, ctx, w, h, seed, cfg, offset, variant=0):
    """One generated case through the call without moments and with maxBatches 1 and 16 (the case's own moments mix is built around one of them), each against
    the restatement.  Returns the number of pixels with 0..4 valid taps."""
    flags, tol, max_history = cfg
    counts = None
    for max_batches in (None,) + bc.MAX_BATCHES:
        case = bc.make_bilinear_case(w, h, seed, max_history, max_batches or 16, variant)
        want, want_src, want_m, valid = bc.reference(case, flags, tol, max_history, max_batches)
        call = BCall(rt, ctx, case, offset, moments=max_batches is not None)
        try:
            assert call.run_bilinear(flags, tol, max_history, max_batches or -7) == rt.abi.RTOW_SUCCESS     # without moments maxBatches is ignored
            _compare(call, want, want_src, want_m, ((w, h), cfg, offset, variant, max_batches))
        finally:
            call.free()
        counts = np.bincount(valid.sum(0), minlength=5)
    return counts


@pytest.mark.parametrize("w,h", bc.SIZES)
def test_bit_exact_against_the_restatement(rt, gpu_context, w, h):
    """Every configuration at every size, with and without moments, buffers 4 bytes into their allocations in every other case.  Over the configurations of a size
    every number of valid taps from 0 to 4 occurs (sizes from 8 x 8 up), and at 96 x 54 each holds at least 2 % of the pixels."""
    total = np.zeros(5)
    for k, cfg in enumerate(CONFIGS):
        variants = range(10) if w * h == 1 else range(1)
        for v in variants:
            total += _check(rt, gpu_context, w, h, bc.seed_of(w, h, k, v), cfg, 4 if k % 2 else 0, v)
    share = total / total.sum()
    print("bilinear reproject %dx%d: share of pixels with 0..4 valid taps %s" % (w, h, np.round(share, 4)))
    if w * h >= 63:
        assert (total > 0).all(), total
    if (w, h) == (96, 54):
        assert share.min() >= 0.02, share


def test_bit_exact_at_1080p_with_moments(rt, gpu_context):
    w, h = 1920, 1080
    flags, tol, max_history = CONFIGS[2]
    case = bc.make_bilinear_case(w, h, 7, max_history, 16)
    want, want_src, want_m, valid = bc.reference(case, flags, tol, max_history, 16)
    share = np.bincount(valid.sum(0), minlength=5) / (w * h)
    print("bilinear reproject 1920x1080: share of pixels with 0..4 valid taps", np.round(share, 4))
    assert share.min() >= 0.02, share
    call = BCall(rt, gpu_context, case, 4)
    try:
        assert call.run_bilinear(flags, tol, max_history, 16) == rt.abi.RTOW_SUCCESS
        _compare(call, want, want_src, want_m, "1080p")
    finally:
        call.free()


@pytest.mark.parametrize("w,h", [(41, 29), (96, 54)])
def test_against_the_nearest_call_on_the_same_inputs(rt, gpu_context, w, h):
    """Every pixel rtowReprojectAccumDevice carries is carried, and where the restatement says the nearest tap is the only valid one the 11 floats of the two calls
    are equal bit for bit."""
    lone_seen = 0
    for k, cfg in enumerate(CONFIGS):
        flags, tol, max_history = cfg
        case = bc.make_bilinear_case(w, h, bc.seed_of(w, h, k), max_history, 16)
        _, _, _, valid = bc.reference(case, flags, tol, max_history)
        call = BCall(rt, gpu_context, case, 4 if k % 2 else 0, moments=False)
        try:
            assert call.run(flags, tol, max_history) == rt.abi.RTOW_SUCCESS
            near, near_src = call.results()
            assert call.run_bilinear(flags, tol, max_history) == rt.abi.RTOW_SUCCESS
            got, got_src = call.results()
        finally:
            call.free()
        assert (got_src[near_src >= 0] >= 0).all(), cfg
        lone = (near_src >= 0) & (valid.sum(0) == 1)
        lone_seen += int(lone.sum())
        assert np.array_equal(got_src[lone], near_src[lone])
        for key in KEYS:
            _same_bits(got[key][lone], near[key][lone], (cfg, key))
    assert lone_seen > 0


def test_null_source_and_null_moments_write_nothing_anywhere_else(rt, gpu_context):
    flags, tol, max_history = CONFIGS[2]
    case = bc.make_bilinear_case(41, 29, 5, max_history, 16)
    want, _, _, _ = bc.reference(case, flags, tol, max_history)
    call = BCall(rt, gpu_context, case, 4, source=False, moments=False)
    try:
        assert call.run_bilinear(flags, tol, max_history, 0) == rt.abi.RTOW_SUCCESS
        got, _ = call.results()
        for k in KEYS:
            _same_bits(got[k], want[k], k)
        assert (call.src.words() == GUARD).all() and (call.om.words() == GUARD).all()
        for b in call.everything():
            assert b.guards_intact()
    finally:
        call.free()


def test_refusals_enqueue_nothing(rt, gpu_context):
    flags, tol, max_history = CONFIGS[2]
    case = bc.make_bilinear_case(16, 8, 3, max_history, 16)
    n = case["n"]
    bad = rt.abi.RTOW_ERROR_INVALID_VALUE
    call = BCall(rt, gpu_context, case)
    run = lambda *args, **over: call.run_bilinear(*(args or (flags, tol, max_history)), **over)
    try:
        for name in ["rays", "t", "e", "pt", "pe"] + ["p" + k for k in KEYS] + ["o" + k for k in KEYS]:
            assert run(**{name: None}) == bad, name
        lib, a = rt.lib.load(), rt.abi
        p = a.ReprojectParams(16, 8, case["view"], tol, max_history, flags, 0)
        hb, ab = a.HitBuffers(call.ins["t"].ptr, call.ins["e"].ptr, None), a.AccumBuffers(*[call.out[k].ptr for k in KEYS])
        pb = a.AccumBuffers(*[call.prev[k].ptr for k in KEYS])
        good = [gpu_context.handle, C.byref(p), call.ins["rays"].ptr, C.byref(hb), C.byref(hb), C.byref(pb), C.byref(ab)]
        for hole in (0, 1, 3, 4, 5, 6):
            args = list(good)
            args[hole] = None
            assert lib.rtowReprojectAccumBilinearDevice(*args, call.pm.ptr, 16, call.om.ptr, call.src.ptr, None) == bad, hole
        for size in ({"w": 0}, {"h": 0}, {"w": -1}, {"w": 65536, "h": 32768}):
            assert run(**size) == bad, size
        for f, t, m in ((flags, -0.01, 64), (flags, float("nan"), 64), (flags, float("inf"), 64), (flags, tol, 0), (flags, tol, -3), (2, tol, 64), (3, tol, 64), (-1, tol, 64)):
            assert run(f, t, m) == bad, (f, t, m)
        assert run(reserved=1) == bad
        flat, nan_view = rt.abi.View(), rr.make_view((0.0, 1.0, 6.0), (0.0, 0.0, 0.0), 16, 8)
        nan_view.vertical.y = float("inf")
        assert run(view=flat) == bad and run(view=nan_view) == bad
        # the moments: one of the pair missing, no batch to carry
        assert run(pm=None) == bad and run(om=None) == bad
        for mb in (0, -1):
            assert run(flags, tol, max_history, mb) == bad, mb
        # an output on a buffer the pass gathers from, or on another output; partial overlaps by one element
        for over in ({"ocolor": call.prev["color"].ptr}, {"onormal": call.prev["color"].ptr + n * 16 - 4}, {"oscw": call.prev["scw"].ptr + 4},
                     {"src": call.prev["albedo"].ptr}, {"oalbedo": call.ins["pt"].ptr}, {"src": call.ins["pe"].ptr + (n - 1) * 4},
                     {"onormal": call.out["color"].ptr + 8}, {"src": call.out["scw"].ptr}, {"oalbedo": call.out["normal"].ptr + n * 12 - 4},
                     {"om": call.pm.ptr}, {"om": call.pm.ptr + n * 12 - 4}, {"om": call.prev["normal"].ptr}, {"om": call.ins["pe"].ptr}, {"om": call.prev["color"].ptr + 4},
                     {"om": call.out["albedo"].ptr}, {"om": call.src.ptr + (n - 1) * 4}, {"om": call.out["color"].ptr - 8},
                     {"ocolor": call.pm.ptr}, {"oscw": call.pm.ptr + n * 12 - 4}, {"src": call.pm.ptr + 8}):
            assert run(**over) == bad, over
        gpu_context.synchronize()
        for b in call.outputs():
            assert (b.words() == GUARD).all()                             # nothing was enqueued
        assert run() == rt.abi.RTOW_SUCCESS
        want, want_src, want_m, _ = bc.reference(case, flags, tol, max_history, 16)
        _compare(call, want, want_src, want_m, "after the refusals")
    finally:
        call.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    flags, tol, max_history = CONFIGS[2]
    case = bc.make_bilinear_case(320, 180, 9, max_history, 16)
    res = []
    for _ in range(2):
        call = BCall(rt, gpu_context, case)
        try:
            assert call.run_bilinear(flags, tol, max_history) == rt.abi.RTOW_SUCCESS
            res.append(call.results() + (call.moments(),))
        finally:
            call.free()
    for k in KEYS:
        assert np.array_equal(res[0][0][k].view(np.uint32), res[1][0][k].view(np.uint32)), k
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2].view(np.uint32), res[1][2].view(np.uint32))


def test_the_call_replays_from_a_captured_graph(rt, gpu_context):
    """The call allocates nothing and waits for nothing: captured on a caller's stream it runs nothing, and the replay writes the bits of a plain call."""
    ctx = gpu_context
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipStreamCreate.argtypes = [C.POINTER(vp)]
    hip.hipStreamBeginCapture.argtypes = [vp, C.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(vp), vp, vp, vp, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [vp, vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    for f in (hip.hipGraphExecDestroy, hip.hipGraphDestroy, hip.hipStreamDestroy):
        f.argtypes = [vp]
    flags, tol, max_history = CONFIGS[2]
    case = bc.make_bilinear_case(96, 54, 11, max_history, 16)
    call = BCall(rt, ctx, case)
    side, graph, exe = vp(), vp(), vp()
    try:
        assert call.run_bilinear(flags, tol, max_history) == rt.abi.RTOW_SUCCESS
        ctx.synchronize()
        plain = [b.words().copy() for b in call.outputs()]
        for b in call.outputs():
            b.buf.upload(np.full(b.words().size, GUARD, np.uint32))
        ctx.synchronize()
        assert hip.hipStreamCreate(C.byref(side)) == 0
        assert hip.hipStreamBeginCapture(side, 2) == 0                    # hipStreamCaptureModeRelaxed
        try:
            rc = call.run_bilinear(flags, tol, max_history, 16, side)
        finally:
            assert hip.hipStreamEndCapture(side, C.byref(graph)) == 0
        assert rc == rt.abi.RTOW_SUCCESS
        assert all((b.words() == GUARD).all() for b in call.outputs()), "capturing runs nothing"
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert hip.hipGraphLaunch(exe, side) == 0
        assert hip.hipStreamSynchronize(side) == 0
        for before, b in zip(plain, call.outputs()):
            assert np.array_equal(before, b.words())
    finally:
        if side:
            hip.hipStreamSynchronize(side)
        if exe:
            hip.hipGraphExecDestroy(exe)
        if graph:
            hip.hipGraphDestroy(graph)
        if side:
            hip.hipStreamDestroy(side)
        call.free()


def test_end_to_end_on_the_cover_scene(rt, gpu_context):
    """192 x 108, as the nearest call's end-to-end test: 64 spp at view A, a 2 % dolly to view B, both calls with the recommended parameters through their jobs, 4 spp
    at B on top of each, against 1024 spp at B.  The bilinear call equals the restatement bit for bit, carries at least the pixels the nearest call carries, and no
    color.w exceeds maxHistory; the squared-error ratio bilinear / nearest is finite - its value is reported (profiles/reproject_bilinear_timing.py --quality
    measures it over seeds and moves), not asserted."""
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

    shapes = ((n, 4), (n, 3), (n, 3), (n,))
    carried, source = {}, {}
    try:
        shared = [up(hits_b["rays"]), up(hits_b["distance"]), up(hits_b["entityIndex"]), up(hits_a["distance"]), up(hits_a["entityIndex"])]
        prev = [up(acc_a[k]) for k in KEYS]
        for name, cls in (("nearest", rt.ReprojectJob), ("bilinear", rt.ReprojectBilinearJob)):
            job = cls(ctx, w, h, pa.view)
            job.Rays, job.HitDistance, job.HitEntityIndex, job.PreviousHitDistance, job.PreviousHitEntityIndex = shared
            job.PreviousColor, job.PreviousNormal, job.PreviousAlbedo, job.PreviousSampleCountWeight = prev
            outs = [room(n * 16), room(n * 12), room(n * 12), room(n * 4)]
            job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = outs
            job.OutputSource = room(n * 4)
            assert job.Schedule().Complete() == 0
            ctx.synchronize()
            carried[name] = {k: b.download(F, s) for k, b, s in zip(KEYS, outs, shapes)}
            source[name] = job.OutputSource.download(np.int32, (n,))
        a = rt.abi
        want, want_src, _, _ = rb.reproject_bilinear(w, h, rr.view_arrays(pa.view), hits_b["rays"]["origin"], hits_b["rays"]["direction"], hits_b["distance"],
                                                     hits_b["entityIndex"], hits_a["distance"], hits_a["entityIndex"], acc_a, a.REPROJECT_DEFAULT_DEPTH_TOLERANCE,
                                                     a.REPROJECT_DEFAULT_MAX_HISTORY, a.REPROJECT_DEFAULT_FLAGS)
        _same_bits(source["bilinear"], want_src, "cover scene source")
        for k in KEYS:
            _same_bits(carried["bilinear"][k], want[k], ("cover scene", k))
        got = {k: v >= 0 for k, v in source.items()}
        assert got["bilinear"][got["nearest"]].all() and got["bilinear"].mean() >= got["nearest"].mean() >= 0.5
        assert carried["bilinear"]["color"][:, 3].max() <= a.REPROJECT_DEFAULT_MAX_HISTORY
        assert np.array_equal(hits_a["entityIndex"][source["bilinear"][got["bilinear"]]], hits_b["entityIndex"][got["bilinear"]])

        frames = {name: rt.sample_batch_host(ctx, at_b(4, 5), inputs=carried[name], want_diag=False) for name in ("nearest", "bilinear")}
        frames["reference"] = rt.sample_batch_host(ctx, at_b(1024, 9), want_diag=False)
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
    mse = {k: float(np.mean((combined[k] - combined["reference"]) ** 2)) for k in ("nearest", "bilinear")}
    ratio = mse["bilinear"] / mse["nearest"]
    print("bilinear reproject quality: carried %.4f (nearest %.4f) of the pixels, nearest MSE %.6g, bilinear MSE %.6g, bilinear / nearest %.4f"
          % (got["bilinear"].mean(), got["nearest"].mean(), mse["nearest"], mse["bilinear"], ratio))
    assert np.isfinite(combined["bilinear"]).all() and np.isfinite(ratio)
