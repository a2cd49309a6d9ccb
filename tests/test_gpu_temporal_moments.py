"""GPU tests of rtowReprojectMomentsDevice and rtowEstimateMomentsDevice (include/rtow.h): both kernels bit for bit against the numpy restatement of their
specification (tests/temporal_moments_reference.py) on synthetic inputs that need no scene - guard words, views 4 bytes into their allocations, in place, from NULL
moments, the early-out path and a single qualifying pixel -, refusals, determinism, the five passes of a frame after a camera move replayed from a captured graph, and
what the carried and estimated moments are worth on the cover scene.  All in the session context, no subprocesses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_variance_reference as dv  # noqa: E402
import reproject_reference as rr  # noqa: E402
import temporal_moments_reference as tm  # noqa: E402
from test_gpu_denoise import _inputs  # noqa: E402  (the awkward guided frames of the plain filter's tests)
from test_gpu_reproject import GUARD, Call, Dev, make_case as reproject_case  # noqa: E402  (guarded device arrays; the inputs of a reprojection)

pytestmark = pytest.mark.gpu

F = np.float32
GUARD_BYTES = np.frombuffer(np.uint32(GUARD).tobytes(), np.uint8)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(got, want, what):
    bad = np.flatnonzero((_bits(got).reshape(len(want), -1) != _bits(want).reshape(len(want), -1)).any(1))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:3]], want[bad[:3]])


# ---------------------------------------------------------------- the gather

def _gather(rt, ctx, n, src, prev, max_batches, out, stream=None):
    return rt.lib.load().rtowReprojectMomentsDevice(ctx.handle, n, src, prev, max_batches, out, stream)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 96 * 54])
def test_gather_bit_exact_against_the_restatement(rt, gpu_context, n):
    """Sources mixing valid indices, -1, INT32_MIN and values >= pixelCount; moments with NaN / inf and n in {0, 0.5, 1, maxBatches, maxBatches + 1, 1e6}; every buffer 4
    bytes into its allocation, guard words intact around all of them."""
    ctx = gpu_context
    for max_batches in (1, 7, 16):
        src, prev = tm.make_gather_case(n, 31 * n + max_batches, max_batches)
        want = tm.reproject_moments(src, prev, max_batches)
        if n >= 64:
            zeros, capped = (want[:, 2] == 0).sum(), (want[:, 2] == max_batches).sum()
            assert zeros >= 5 and capped >= 5 and (want[:, 2] > 0).sum() >= 5, (zeros, capped)
        bufs = [Dev(rt, ctx, n * 4, 4, src), Dev(rt, ctx, n * 12, 4, prev), Dev(rt, ctx, n * 12, 4)]
        try:
            assert _gather(rt, ctx, n, bufs[0].ptr, bufs[1].ptr, max_batches, bufs[2].ptr) == rt.abi.RTOW_SUCCESS
            ctx.synchronize()
            _assert_same(bufs[2].download(F, (n, 3)), want, (n, max_batches))
            assert all(b.guards_intact() for b in bufs)
        finally:
            for b in bufs:
                b.free()


# ---------------------------------------------------------------- the estimate

class Estimate:
    """the device inputs of one case, uploaded once; every run gets fresh guarded outputs"""

    def __init__(self, rt, ctx, case, offset):
        self.rt, self.ctx, self.case, self.offset = rt, ctx, case, offset
        t, e, nrm = case["hits"]
        self.ins = [Dev(rt, ctx, a.nbytes, offset, a) for a in (case["color"], t, e, nrm)]

    def run(self, cfg, moments, mode, stream=None):
        """mode: "out" (out of place), "in" (in place), "null" (inMoments NULL), "nofilled" (out of place, outFilled NULL) -> (outMoments, outFilled or None)"""
        rt, ctx, n = self.rt, self.ctx, self.case["n"]
        min_batches, min_taps, sharp, tol, flags = cfg
        p = rt.abi.EstimateMomentsParams(self.case["w"], self.case["h"], min_batches, min_taps, sharp, tol, flags, 0)
        hits = rt.abi.HitBuffers(self.ins[1].ptr, self.ins[2].ptr, self.ins[3].ptr)
        nfill = (n + 3) // 4 * 4
        out = Dev(rt, ctx, n * 12, self.offset, moments if mode == "in" else None)
        m_in = None if mode in ("in", "null") else Dev(rt, ctx, n * 12, self.offset, moments)
        fill = None if mode == "nofilled" else Dev(rt, ctx, nfill, self.offset)
        try:
            in_ptr = out.ptr if mode == "in" else (None if mode == "null" else m_in.ptr)
            rc = rt.lib.load().rtowEstimateMomentsDevice(ctx.handle, C.byref(p), self.ins[0].ptr, C.byref(hits), in_ptr, out.ptr, fill.ptr if fill else None, stream)
            assert rc == rt.abi.RTOW_SUCCESS, (rc, cfg, mode)
            ctx.synchronize()
            got = out.download(F, (n, 3))
            got_fill = None
            if fill:
                raw = fill.download(np.uint8, (nfill,))
                assert np.array_equal(raw[n:], GUARD_BYTES[4 - (nfill - n):] if nfill > n else raw[:0]), "bytes behind outFilled"
                got_fill = raw[:n]
            for b in self.ins + [x for x in (out, m_in, fill) if x is not None]:
                assert b.guards_intact(), (cfg, mode)
            if m_in is not None:
                assert np.array_equal(_bits(m_in.download(F, (n, 3))), _bits(moments)), "inMoments is read only"
            return got, got_fill
        finally:
            for b in (out, m_in, fill):
                if b is not None:
                    b.free()

    def free(self):
        for b in self.ins:
            b.free()


@pytest.mark.parametrize("w,h", tm.SIZES)
def test_estimate_bit_exact_against_the_restatement(rt, gpu_context, w, h):
    """Every configuration at every size - widths and heights below the halo, exact tiles, one past a tile: the moments as generated, the variant in which no pixel
    qualifies (the early-out path) and the one in which exactly one pixel of one tile does, each out of place, in place and without outFilled, and from NULL moments.
    Every pixel of every output is compared.  With minTaps 2 every case larger than 8 x 8 has filled pixels, qualifying pixels left unchanged and pixels that do not
    qualify (asserted on the restatement), so that agreement on "unchanged" cannot hide a kernel that does nothing."""
    ctx = gpu_context
    case = tm.make_case(w, h, tm.case_seed(w, h))
    n = w * h
    for k, cfg in enumerate(tm.CONFIGS):
        est = Estimate(rt, ctx, case, 4 * (k & 1))
        try:
            one, at = tm.one_pixel_qualifies(case, cfg)
            for name, moments in (("given", case["moments"]), ("none", tm.no_pixel_qualifies(case, cfg)), ("one", one)):
                want, want_fill, wanted = tm.reference(case, cfg, moments)
                if name == "given" and cfg[1] == 2 and n > 64:
                    assert min(tm.coverage(want_fill, wanted)) >= 3, (cfg, tm.coverage(want_fill, wanted))
                if name == "none":
                    assert not wanted.any() and np.array_equal(_bits(want), _bits(moments))
                if name == "one":
                    assert wanted.sum() == 1 and wanted[at]
                for mode in ("out", "in", "nofilled"):
                    got, got_fill = est.run(cfg, moments, mode)
                    _assert_same(got, want, ((w, h), cfg, name, mode))
                    if got_fill is not None:
                        assert np.array_equal(got_fill, want_fill), ((w, h), cfg, name, mode)
            want, want_fill, wanted = tm.reference(case, cfg, None)
            assert wanted.all()
            got, got_fill = est.run(cfg, None, "null")
            _assert_same(got, want, ((w, h), cfg, "null"))
            assert np.array_equal(got_fill, want_fill)
        finally:
            est.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    ctx = gpu_context
    w, h = 320, 180
    case = tm.make_case(w, h, 77)
    est = Estimate(rt, ctx, case, 0)
    try:
        a = est.run(tm.CONFIGS[0], case["moments"], "out")
        b = est.run(tm.CONFIGS[0], case["moments"], "out")
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(a[1], b[1])
        assert 0 < a[1].sum() < w * h
    finally:
        est.free()
    n = w * h
    src, prev = tm.make_gather_case(n, 78, 16)
    bufs = [Dev(rt, ctx, n * 4, 0, src), Dev(rt, ctx, n * 12, 0, prev), Dev(rt, ctx, n * 12), Dev(rt, ctx, n * 12)]
    try:
        for o in bufs[2:]:
            assert _gather(rt, ctx, n, bufs[0].ptr, bufs[1].ptr, 16, o.ptr) == rt.abi.RTOW_SUCCESS
        ctx.synchronize()
        assert np.array_equal(_bits(bufs[2].download(F, (n, 3))), _bits(bufs[3].download(F, (n, 3))))
    finally:
        for b in bufs:
            b.free()


def test_refusals_enqueue_nothing(rt, gpu_context):
    """Every refusal of both calls returns RTOW_ERROR_INVALID_VALUE and leaves the outputs' guard pattern as it was."""
    ctx = gpu_context
    lib = rt.lib.load()
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    w, h = 16, 8
    n = w * h
    color, t, e, nrm, m_in = Dev(rt, ctx, n * 16), Dev(rt, ctx, n * 4), Dev(rt, ctx, n * 4), Dev(rt, ctx, n * 12), Dev(rt, ctx, n * 12)
    out, fill, src = Dev(rt, ctx, n * 12 + 16), Dev(rt, ctx, n), Dev(rt, ctx, n * 4)
    everything = [color, t, e, nrm, m_in, out, fill, src]
    try:
        def estimate(values=(w, h, 4, 8, 2, 0.05, 1, 0), **over):
            ptr = {"params": True, "color": color.ptr, "hits": True, "t": t.ptr, "e": e.ptr, "n": nrm.ptr, "m_in": m_in.ptr, "out": out.ptr, "fill": fill.ptr}
            ptr.update(over)
            p = a.EstimateMomentsParams(*values)
            hits = a.HitBuffers(ptr["t"], ptr["e"], ptr["n"])
            return lib.rtowEstimateMomentsDevice(ctx.handle, C.byref(p) if ptr["params"] else None, ptr["color"], C.byref(hits) if ptr["hits"] else None, ptr["m_in"],
                                                 ptr["out"], ptr["fill"], None)

        for name in ("params", "color", "hits", "t", "e", "n", "out"):
            assert estimate(**{name: None}) == bad, name
        good = [w, h, 4, 8, 2, 0.05, 1, 0]
        for index, value in ((0, 0), (0, -1), (1, 0), (2, 0), (2, -3), (3, 1), (3, 50), (3, 0), (4, -1), (4, 9), (5, -0.01), (5, float("nan")), (5, float("inf")),
                             (6, 2), (6, 3), (6, -1), (7, 1)):
            p = list(good)
            p[index] = value
            assert estimate(tuple(p)) == bad, (index, value)
        assert estimate((65536, 32768, 4, 8, 2, 0.05, 1, 0)) == bad                   # width * height > INT32_MAX
        for name in ("color", "t", "e", "n"):
            assert estimate(out={"color": color, "t": t, "e": e, "n": nrm}[name].ptr) == bad, ("outMoments over", name)
            assert estimate(fill={"color": color, "t": t, "e": e, "n": nrm}[name].ptr) == bad, ("outFilled over", name)
        assert estimate(fill=out.ptr + 8) == bad                                       # the outputs overlap each other
        assert estimate(fill=m_in.ptr + 4) == bad                                      # outFilled over inMoments
        assert estimate(m_in=out.ptr + 12) == bad and estimate(m_in=out.ptr + 4) == bad        # inMoments overlapping outMoments other than exactly
        assert estimate(m_in=out.ptr, fill=out.ptr + 4) == bad                         # in place, with outFilled inside the moments

        def gather(count=n, max_batches=16, **over):
            ptr = {"src": src.ptr, "prev": m_in.ptr, "out": out.ptr}
            ptr.update(over)
            return lib.rtowReprojectMomentsDevice(ctx.handle, count, ptr["src"], ptr["prev"], max_batches, ptr["out"], None)

        for name in ("src", "prev", "out"):
            assert gather(**{name: None}) == bad, name
        assert gather(count=0) == bad and gather(count=-5) == bad and gather(max_batches=0) == bad and gather(max_batches=-1) == bad
        assert gather(out=m_in.ptr) == bad and gather(out=m_in.ptr + 12 * (n - 1)) == bad and gather(prev=out.ptr + 4) == bad      # a gather: never in place
        assert gather(out=src.ptr) == bad and gather(src=out.ptr + 8) == bad
        ctx.synchronize()
        for b in everything:
            assert (b.words() == GUARD).all()
        # and the calls these were variations of are accepted
        for b, data in ((color, np.ones((n, 4), F)), (t, np.ones(n, F)), (e, np.zeros(n, np.int32)), (nrm, np.ones((n, 3), F)), (m_in, np.zeros((n, 3), F)),
                        (src, np.arange(n, dtype=np.int32))):
            b.buf.upload(np.concatenate([np.full(b.front // 4, GUARD, np.uint32), _bits(data).ravel(), np.full(4, GUARD, np.uint32)]))
        assert estimate() == a.RTOW_SUCCESS and estimate(m_in=out.ptr) == a.RTOW_SUCCESS and estimate(m_in=None, fill=None) == a.RTOW_SUCCESS
        assert gather() == a.RTOW_SUCCESS
        ctx.synchronize()
    finally:
        for b in everything:
            b.free()


# ---------------------------------------------------------------- the passes of a frame after a move, replayed from a captured graph

def test_the_frame_after_a_move_replays_from_a_captured_graph(rt, gpu_context):
    """rtowReprojectAccumDevice, rtowReprojectMomentsDevice, rtowAccumulateMomentsDevice (in place), rtowEstimateMomentsDevice and rtowDenoiseVarianceDevice captured on
    a caller's stream - none allocates, none waits - and replayed once: every output equals, bit for bit, what the same calls give one by one with a wait after each."""
    ctx = gpu_context
    a = rt.abi
    lib = rt.lib.load()
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, C.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(vp), vp, vp, vp, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [vp, vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    for f in (hip.hipGraphExecDestroy, hip.hipGraphDestroy, hip.hipStreamDestroy):
        f.argtypes = [vp]
    w, h = 96, 54
    n = w * h
    case = reproject_case(w, h, 5, 64)
    rng = np.random.default_rng(6)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1)[:, None]).astype(F)
    nrm[case["e"] < 0] = 0
    prev_moments = tm.make_gather_case(n, 7, 16)[1]
    batches = [np.concatenate([rng.uniform(0, 2, (n, 3)), np.ones((n, 1))], axis=1).astype(F) for _ in range(2)]
    dc, dn, da = _inputs(w, h, 8)
    call = Call(rt, ctx, case)
    mk = lambda x: Dev(rt, ctx, np.ascontiguousarray(x).nbytes, 0, x)
    ins = {"nrm": mk(nrm), "pm": mk(prev_moments), "b0": mk(batches[0]), "b1": mk(batches[1]), "dc": mk(dc), "dn": mk(dn), "da": mk(da)}
    outs = {"mom": Dev(rt, ctx, n * 12), "est": Dev(rt, ctx, n * 12), "fill": Dev(rt, ctx, n), "den": Dev(rt, ctx, n * 12), "var": Dev(rt, ctx, n * 4)}
    scratch = rt.DeviceBuffer(ctx, a.denoise_variance_scratch_bytes(w, h))
    cfg = (a.ESTIMATE_MOMENTS_DEFAULT_MIN_BATCHES, 2, a.ESTIMATE_MOMENTS_DEFAULT_NORMAL_SHARPNESS, 1.0, 0)
    side, graph, exe = vp(), vp(), vp()

    def passes(stream, wait):
        steps = []
        steps.append(lambda: call.run(1, 0.01, 64, stream))
        steps.append(lambda: _gather(rt, ctx, n, call.src.ptr, ins["pm"].ptr, 16, outs["mom"].ptr, stream))
        colors = (vp * 2)(ins["b0"].ptr, ins["b1"].ptr)
        steps.append(lambda: lib.rtowAccumulateMomentsDevice(ctx.handle, n, 2, colors, outs["mom"].ptr, outs["mom"].ptr, stream))
        ep = a.EstimateMomentsParams(w, h, *cfg, 0)
        hits = a.HitBuffers(call.ins["t"].ptr, call.ins["e"].ptr, ins["nrm"].ptr)
        steps.append(lambda: lib.rtowEstimateMomentsDevice(ctx.handle, C.byref(ep), call.out["color"].ptr, C.byref(hits), outs["mom"].ptr, outs["est"].ptr,
                                                           outs["fill"].ptr, stream))
        dp = a.DenoiseParams(w, h, 3, 2, 2.0, 0.125, 1, 0)
        steps.append(lambda: lib.rtowDenoiseVarianceDevice(ctx.handle, C.byref(dp), ins["dc"].ptr, ins["dn"].ptr, ins["da"].ptr, outs["est"].ptr, scratch.ptr,
                                                           outs["den"].ptr, outs["var"].ptr, stream))
        for step in steps:
            assert step() == a.RTOW_SUCCESS
            if wait:
                ctx.synchronize()

    def snapshot():
        res = {k: v.words().copy() for k, v in outs.items()}
        res.update({"acc_" + k: v.words().copy() for k, v in call.out.items()})
        res["src"] = call.src.words().copy()
        return res

    try:
        passes(None, True)
        one_by_one = snapshot()
        est_host = outs["est"].download(F, (n, 3))
        assert 0 < outs["fill"].download(np.uint8, (n,)).sum() < n and (est_host[:, 2] >= 2).any()
        for v in list(outs.values()) + list(call.out.values()) + [call.src]:       # back to the guard pattern: the replay has to write everything again
            v.buf.upload(np.full(v.words().size, GUARD, np.uint32))
        ctx.synchronize()
        assert hip.hipStreamCreate(C.byref(side)) == 0
        assert hip.hipStreamBeginCapture(side, 2) == 0                             # hipStreamCaptureModeRelaxed
        try:
            passes(side, False)
        finally:
            assert hip.hipStreamEndCapture(side, C.byref(graph)) == 0
        assert all((v.words() == GUARD).all() for v in outs.values()), "capturing runs nothing"
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert hip.hipGraphLaunch(exe, side) == 0
        assert hip.hipStreamSynchronize(side) == 0
        replayed = snapshot()
        for k in one_by_one:
            assert np.array_equal(one_by_one[k], replayed[k]), k
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
        for b in list(ins.values()) + list(outs.values()):
            b.free()
        scratch.free()


# ---------------------------------------------------------------- what the moments are worth on the cover scene

KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))
W, H = 192, 108


def _params_at(rt, scene, view, lens_radius, spp, seed):
    p = rt.scenes.make_params(scene, W, H, spp=spp, trace_depth=8, seed=seed)
    if view is not None:
        p.view = view
        p.view.lensRadius = lens_radius
    return p


def _group(rt, ctx, plist):
    """independent batches from zeroed inputs (rtowSampleBatchGroupDevice) -> the per-batch host arrays [[color, normal, albedo, scw], ...]"""
    n = W * H
    zero = [rt.DeviceBuffer(ctx, n * k * 4).zero() for _, k in KEYS]
    outs = [[rt.DeviceBuffer(ctx, n * k * 4).zero() for _, k in KEYS] for _ in plist]
    ctx.synchronize()
    try:
        assert rt.sample_batch_group_device(ctx, plist, zero, outs, None, None) == 0
        ctx.synchronize()
        return [[b.download(F, (n, k)) for b, (_, k) in zip(o, KEYS)] for o in outs]
    finally:
        for b in zero + [b for o in outs for b in o]:
            b.free()


def _fold(batches):
    acc = [np.zeros_like(x) for x in batches[0]]
    for b in batches:
        acc = [s + x for s, x in zip(acc, b)]                              # rtowAddAccumDevice: dst += src, in batch order
    return acc


class Rig:
    """device buffers of one quality frame: upload once, run parameter points"""

    def __init__(self, rt, ctx):
        self.rt, self.ctx, self.bufs = rt, ctx, []

    def up(self, x):
        self.bufs.append(self.rt.DeviceBuffer(self.ctx).upload(np.ascontiguousarray(x)))
        return self.bufs[-1]

    def room(self, nbytes):
        self.bufs.append(self.rt.DeviceBuffer(self.ctx, nbytes))
        return self.bufs[-1]

    def combine(self, acc):
        n = W * H
        res = [self.room(n * 12) for _ in range(3)]
        cj = self.rt.CombineJob(self.ctx, (W, H))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = acc[:3]
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = res
        assert cj.Schedule().Complete() == 0
        self.ctx.synchronize()
        return res

    def denoise_variance(self, comb, moments):
        n = W * H
        if not hasattr(self, "den"):
            self.den, self.scratch = self.room(n * 12), self.room(self.rt.abi.denoise_variance_scratch_bytes(W, H))
        dj = self.rt.DenoiseVarianceJob(self.ctx, W, H)
        dj.InputColor, dj.InputNormal, dj.InputAlbedo, dj.Moments, dj.Scratch, dj.OutputColor = comb[0], comb[1], comb[2], moments, self.scratch, self.den
        assert dj.Schedule().Complete() == 0
        self.ctx.synchronize()
        return self.den.download(F, (n, 3))

    def estimate(self, cfg, color, hits, m_in, m_out, filled):
        min_batches, min_taps, sharp, tol, flags = cfg
        ej = self.rt.EstimateMomentsJob(self.ctx, W, H, min_batches, min_taps, sharp, tol, flags)
        ej.Color, (ej.HitDistance, ej.HitEntityIndex, ej.HitNormal) = color, hits
        ej.InputMoments, ej.OutputMoments, ej.OutputFilled = m_in, m_out, filled
        assert ej.Schedule().Complete() == 0

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def recommended_estimate(a):
    return (a.ESTIMATE_MOMENTS_DEFAULT_MIN_BATCHES, a.ESTIMATE_MOMENTS_DEFAULT_MIN_TAPS, a.ESTIMATE_MOMENTS_DEFAULT_NORMAL_SHARPNESS,
            a.ESTIMATE_MOMENTS_DEFAULT_DEPTH_TOLERANCE, a.ESTIMATE_MOMENTS_DEFAULT_FLAGS)


def mse(x, ref):
    return float(np.mean((x.astype(np.float64) - ref.astype(np.float64)) ** 2))


class MoveFrame(Rig):
    """tests/test_gpu_reproject.py's protocol with moments: the cover scene at 192 x 108; view A a group of 16 x 4 spp (seeds 1..16) with its moments; the camera
    dollies 2 % of the way to its target (view B); accumulators reprojected with their recommended values; at B a group of 4 x 1 spp (seeds 201..204) from zero,
    folded on top.  run(maxBatches, cfg) carries the moments, adds B's batches, estimates, and denoises with rtowDenoiseVarianceDevice's recommended set;
    restarted() denoises the identical accumulators with the moments of B's four batches only - what a host gets today.  Reference: 1024 spp at B (seed 9).
    (profiles/temporal_moments_timing.py runs its parameter grid on this frame.)"""

    def __init__(self, rt, ctx):
        super().__init__(rt, ctx)
        S = rt.scenes
        n = W * H
        scene = S.cover_scene()
        ctx.upload_scene(scene.desc())
        pa = _params_at(rt, scene, None, None, 4, 1)
        cam = scene.camera
        position, target = np.asarray(cam["position"], np.float64), np.asarray(cam["target"], np.float64)
        focus = S.focus_distance(scene, np.asarray(cam["position"], F), S._normalize(np.asarray(cam["target"], F) - np.asarray(cam["position"], F)))
        view_b = rr.make_view(tuple(position + 0.02 * (target - position)), tuple(target), W, H, vfov=cam["vfov"], focus=focus, up=tuple(cam["up"]))
        lens = pa.view.lensRadius
        group_a = _group(rt, ctx, [_params_at(rt, scene, None, None, 4, 1 + k) for k in range(16)])
        self.group_b = _group(rt, ctx, [_params_at(rt, scene, view_b, lens, 1, 201 + k) for k in range(4)])
        self.moments_a = dv.accumulate_moments([b[0] for b in group_a])
        acc_a = _fold(group_a)
        ref = rt.sample_batch_host(ctx, _params_at(rt, scene, view_b, lens, 1024, 9), want_diag=False)
        hits_a = ctx.trace_view(pa.view, W, H, want=("distance", "entityIndex"))
        self.hits_b = ctx.trace_view(view_b, W, H, want_rays=True)
        job = rt.ReprojectJob(ctx, W, H, pa.view)
        job.Rays, job.HitDistance, job.HitEntityIndex = self.up(self.hits_b["rays"]), self.up(self.hits_b["distance"]), self.up(self.hits_b["entityIndex"])
        job.PreviousHitDistance, job.PreviousHitEntityIndex = self.up(hits_a["distance"]), self.up(hits_a["entityIndex"])
        job.PreviousColor, job.PreviousNormal, job.PreviousAlbedo, job.PreviousSampleCountWeight = [self.up(x) for x in acc_a]
        self.acc = [self.room(n * k * 4) for _, k in KEYS]
        job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = self.acc
        job.OutputSource = self.src = self.room(n * 4)
        assert job.Schedule().Complete() == 0
        self.hits = (job.HitDistance, job.HitEntityIndex, self.up(self.hits_b["normal"]))
        self.batch_colors = [self.up(b[0]) for b in self.group_b]
        lib = rt.lib.load()
        dst = rt.abi.AccumBuffers(*[b.ptr for b in self.acc])
        for b in self.group_b:
            part = [self.up(x) for x in b]
            src = rt.abi.AccumBuffers(*[x.ptr for x in part])
            assert lib.rtowAddAccumDevice(ctx.handle, n, C.byref(dst), C.byref(src), None) == 0
        ctx.synchronize()
        self.source = self.src.download(np.int32, (n,))
        self.color = self.acc[0].download(F, (n, 4))
        self.comb = self.combine(self.acc)
        self.albedo = self.comb[2].download(F, (n, 3))
        self.noisy = self.comb[0].download(F, (n, 3))
        self.reference = self.combine([self.up(ref[k]) for k in ("color", "normal", "albedo")])[0].download(F, (n, 3))
        self.d_moments_a = self.up(self.moments_a)
        self.mom, self.est, self.filled = self.room(n * 12), self.room(n * 12), self.room(n)

    def _accumulate(self, m_in):
        mj = self.rt.MomentsJob(self.ctx, W * H)
        mj.Colors, mj.InputMoments, mj.OutputMoments = self.batch_colors, m_in, self.mom
        assert mj.Schedule().Complete() == 0

    def run(self, max_batches, cfg):
        """-> (moments before the estimate, moments after it, outFilled, the denoised frame)"""
        n = W * H
        rj = self.rt.ReprojectMomentsJob(self.ctx, n, max_batches)
        rj.Source, rj.PreviousMoments, rj.OutputMoments = self.src, self.d_moments_a, self.mom
        assert rj.Schedule().Complete() == 0
        self._accumulate(self.mom)
        self.estimate(cfg, self.acc[0], self.hits, self.mom, self.est, self.filled)
        self.ctx.synchronize()
        before, after, filled = self.mom.download(F, (n, 3)), self.est.download(F, (n, 3)), self.filled.download(np.uint8, (n,))
        return before, after, filled, self.denoise_variance(self.comb, self.est)

    def restarted(self):
        """-> (the moments of B's four batches alone, the frame denoised with them)"""
        self._accumulate(None)
        self.ctx.synchronize()
        return self.mom.download(F, (W * H, 3)), self.denoise_variance(self.comb, self.mom)


class SingleBatchFrame(Rig):
    """one 4-spp batch of the cover scene at its own camera (seed 1), which leaves no per-batch colours: run(cfg) estimates every pixel's moments (inMoments NULL) and
    denoises with rtowDenoiseVarianceDevice's recommended set; plain() is rtowDenoiseDevice with its recommended set on the same frame.  Reference: 1024 spp (seed 2)."""

    def __init__(self, rt, ctx):
        super().__init__(rt, ctx)
        n = W * H
        scene = rt.scenes.cover_scene()
        ctx.upload_scene(scene.desc())
        p = _params_at(rt, scene, None, None, 4, 1)
        acc = rt.sample_batch_host(ctx, p, want_diag=False)
        ref = rt.sample_batch_host(ctx, _params_at(rt, scene, None, None, 1024, 2), want_diag=False)
        self.hits_a = ctx.trace_view(p.view, W, H)
        self.color = acc["color"]
        self.acc = [self.up(acc[k]) for k in ("color", "normal", "albedo")]
        self.hits = tuple(self.up(self.hits_a[k]) for k in ("distance", "entityIndex", "normal"))
        self.comb = self.combine(self.acc)
        self.albedo = self.comb[2].download(F, (n, 3))
        self.noisy = self.comb[0].download(F, (n, 3))
        self.reference = self.combine([self.up(ref[k]) for k in ("color", "normal", "albedo")])[0].download(F, (n, 3))
        self.est, self.filled = self.room(n * 12), self.room(n)

    def run(self, cfg):
        n = W * H
        self.estimate(cfg, self.acc[0], self.hits, None, self.est, self.filled)
        self.ctx.synchronize()
        return self.est.download(F, (n, 3)), self.filled.download(np.uint8, (n,)), self.denoise_variance(self.comb, self.est)

    def plain(self):
        n = W * H
        out, scratch = self.room(n * 12), self.room(self.rt.abi.denoise_scratch_bytes(W, H))
        dj = self.rt.DenoiseJob(self.ctx, W, H)
        dj.InputColor, dj.InputNormal, dj.InputAlbedo, dj.Scratch, dj.OutputColor = self.comb[0], self.comb[1], self.comb[2], scratch, out
        assert dj.Schedule().Complete() == 0
        self.ctx.synchronize()
        return out.download(F, (n, 3))


# the asserted bound of the end-to-end test: the ratio measured on an MI355X times 1.25 for seed-to-seed spread, never above 1
MEASURED_RATIO = 0.6089
RATIO_BOUND = 1.0 if MEASURED_RATIO is None else min(1.0, 1.25 * MEASURED_RATIO)
# the single-batch ratio is recorded, not bounded: no point of the parameter grid brings it below 1 (profiles/r13_temporal_moments.json: 1.0036 .. 1.4693 over the 72
# points, 1.0036 at the recommended one), so the test asserts that it is finite and prints it - a measured "no gain"
MEASURED_SINGLE_BATCH_RATIO = 1.0036


def test_end_to_end_after_a_camera_move_on_the_cover_scene(rt, gpu_context):
    """MoveFrame's protocol with the recommended values.  Exact: at least half the pixels are carried; every carried pixel has n >= 2 before the estimate; the
    estimate equals the restatement bit for bit, and every pixel it fills has a known initial variance; the share of pixels with a known variance is not below that
    with restarted moments.  Quality: the squared error against 1024 spp of the frame denoised with the carried and estimated moments, over that of the identical
    accumulators denoised with restarted moments, is below 1 and within the measured ratio times 1.25 (measured on an MI355X: 0.6089, 99 % of the pixels carried; 0.6089
    .. 0.8209 over the 1080 points of the parameter grid, 0.61 .. 0.62 wherever maxBatches >= 16)."""
    a = rt.abi
    frame = MoveFrame(rt, gpu_context)
    try:
        cfg = recommended_estimate(a)
        before, after, filled, den = frame.run(a.REPROJECT_MOMENTS_DEFAULT_MAX_BATCHES, cfg)
        restarted_moments, den_restarted = frame.restarted()
    finally:
        frame.free()
    carried = frame.source >= 0
    assert carried.mean() >= 0.5, carried.mean()
    want_before = dv.accumulate_moments([b[0] for b in frame.group_b], tm.reproject_moments(frame.source, frame.moments_a, a.REPROJECT_MOMENTS_DEFAULT_MAX_BATCHES))
    _assert_same(before, want_before, "carried moments plus the new batches")
    assert (before[carried, 2] >= 2).all(), before[carried, 2].min()
    hits = (frame.hits_b["distance"], frame.hits_b["entityIndex"], frame.hits_b["normal"])
    want, want_filled, wanted = tm.estimate_moments(W, H, frame.color, hits, before, *cfg)
    _assert_same(after, want, "estimate")
    assert np.array_equal(filled, want_filled)
    flags = a.DENOISE_VARIANCE_DEFAULT_FLAGS
    v0, v0_restarted = dv.initial_variance(after, frame.albedo, flags), dv.initial_variance(restarted_moments, frame.albedo, flags)
    assert (v0[want_filled.astype(bool)] >= 0).all()
    known, known_restarted = float((v0 >= 0).mean()), float((v0_restarted >= 0).mean())
    assert known >= known_restarted, (known, known_restarted)
    assert np.isfinite(den).all()
    e_new, e_old, e_noisy = mse(den, frame.reference), mse(den_restarted, frame.reference), mse(frame.noisy, frame.reference)
    ratio = e_new / e_old
    print("temporal moments after a 2 %% dolly: carried %.4f of the pixels, qualifying %.4f, filled %.4f, known variance %.4f (restarted %.4f); MSE noisy %.6g, "
          "denoised with restarted moments %.6g, with carried and estimated moments %.6g, ratio %.4f"
          % (carried.mean(), wanted.mean(), want_filled.mean(), known, known_restarted, e_noisy, e_old, e_new, ratio))
    assert ratio < 1.0 and ratio <= RATIO_BOUND, ratio


def test_a_single_batch_frame_gets_a_variance(rt, gpu_context):
    """SingleBatchFrame's protocol with the recommended values: a known initial variance exists wherever the restatement fills (and the estimate equals it bit for
    bit).  The squared error against 1024 spp of rtowDenoiseVarianceDevice on the estimated moments, over rtowDenoiseDevice's with its recommended set, is printed
    and asserted to be finite only: measured on an MI355X it is 1.0036 at the recommended values and between 1.0036 and 1.4693 over the parameter grid - no point brings
    it below 1.  A spatial estimate gives a single-batch frame a variance (97 % of the pixels and more), and the variance-guided filter then does what the plain
    filter with its tuned fixed sigma does on a 4-spp frame, not better."""
    a = rt.abi
    frame = SingleBatchFrame(rt, gpu_context)
    try:
        cfg = recommended_estimate(a)
        est, filled, den = frame.run(cfg)
        plain = frame.plain()
    finally:
        frame.free()
    hits = (frame.hits_a["distance"], frame.hits_a["entityIndex"], frame.hits_a["normal"])
    want, want_filled, wanted = tm.estimate_moments(W, H, frame.color, hits, None, *cfg)
    _assert_same(est, want, "estimate")
    assert np.array_equal(filled, want_filled) and wanted.all()
    v0 = dv.initial_variance(est, frame.albedo, a.DENOISE_VARIANCE_DEFAULT_FLAGS)
    assert (v0[want_filled.astype(bool)] >= 0).all() and want_filled.mean() > 0.5, want_filled.mean()
    assert np.isfinite(den).all()
    e_var, e_plain, e_noisy = mse(den, frame.reference), mse(plain, frame.reference), mse(frame.noisy, frame.reference)
    ratio = e_var / e_plain
    print("single 4-spp batch: filled %.4f of the pixels; MSE noisy %.6g, rtowDenoiseDevice %.6g, rtowDenoiseVarianceDevice on estimated moments %.6g, ratio %.4f"
          % (want_filled.mean(), e_noisy, e_plain, e_var, ratio))
    assert np.isfinite(ratio), ratio
