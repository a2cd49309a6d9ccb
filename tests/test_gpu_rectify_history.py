"""GPU tests of rtowRectifyHistoryDevice (include/rtow.h): the kernel bit for bit against the numpy restatement of its specification
(tests/rectify_history_reference.py) on synthetic inputs that need no scene - every size, radius and flag, out of place, fully in place, without moments, without
outKeep and outStats, 4 bytes into every allocation, guard words intact -, refusals, determinism, one call replayed from a captured graph, and what the pass is worth
on the cover scene after a camera move.  All in the session context, no subprocesses.

The quality figures are measured, not promised (profiles/rectify_history_timing.py --quality, profiles/r15_rectify_history.json; MEASURED below): on the orbit the
rectified frame has 0.977 of the carried frame's squared error on the metal and glass pixels, on all three seeds, and the test asserts it; on the 2 % dolly the pass
is a measured "no gain" (0.999, above 1 on one seed of three), and the test asserts only that the ratios are finite."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_variance_reference as dv  # noqa: E402
import rectify_history_reference as rh  # noqa: E402
import reproject_reference as rr  # noqa: E402
from test_gpu_reproject import GUARD, Dev  # noqa: E402  (guarded device arrays)
from test_gpu_temporal_moments import KEYS, H, W, Rig, _fold, _group, _params_at, recommended_estimate  # noqa: E402  (the quality frames' plumbing)

pytestmark = pytest.mark.gpu

F = np.float32
SHAPES = {"color": 4, "normal": 3, "albedo": 3, "scw": 1, "moments": 3, "keep": 1}
MODES = ("out", "in", "nomoments", "bare", "offset")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(got, want, what):
    g, w = _bits(got).reshape(len(want), -1), _bits(want).reshape(len(want), -1)
    bad = np.flatnonzero((g != w).any(1))
    assert bad.size == 0, (what, bad.size, bad[:5], np.asarray(got).reshape(len(want), -1)[bad[:3]], np.asarray(want).reshape(len(want), -1)[bad[:3]])


class Rectify:
    """the device inputs of one case that no mode writes, uploaded once per offset; every run gets fresh guarded history and outputs"""

    def __init__(self, rt, ctx, case):
        self.rt, self.ctx, self.case, self.ins = rt, ctx, case, {}

    def _inputs(self, offset):
        if offset not in self.ins:
            t, e, nrm = self.case["hits"]
            self.ins[offset] = [Dev(self.rt, self.ctx, a.nbytes, offset, a) for a in (self.case["fresh"], t, e, nrm)]
        return self.ins[offset]

    def prepare(self, mode):
        """mode: "out" (out of place, every output), "in" (every allowed alias), "nomoments" (inMoments and outMoments NULL), "bare" (outKeep and outStats NULL),
        "offset" (as "out", every buffer 4 bytes into its allocation) -> the guarded buffers of one call"""
        rt, ctx, case = self.rt, self.ctx, self.case
        n = case["n"]
        offset = 4 if mode == "offset" else 0
        B = {"mode": mode, "ins": self._inputs(offset)}
        B["hist"] = {k: Dev(rt, ctx, n * 4 * SHAPES[k], offset, case["history"][k]) for k, _ in rh.KEYS}
        B["m_in"] = None if mode == "nomoments" else Dev(rt, ctx, n * 12, offset, case["moments"])
        if mode == "in":
            B["out"], B["m_out"] = B["hist"], B["m_in"]
        else:
            B["out"] = {k: Dev(rt, ctx, n * 4 * SHAPES[k], offset) for k, _ in rh.KEYS}
            B["m_out"] = None if B["m_in"] is None else Dev(rt, ctx, n * 12, offset)
        B["keep"] = None if mode == "bare" else Dev(rt, ctx, n * 4, offset)
        B["stats"] = None if mode == "bare" else Dev(rt, ctx, 16, offset)
        B["own"] = list({id(b): b for b in list(B["hist"].values()) + list(B["out"].values()) + [B["m_in"], B["m_out"], B["keep"], B["stats"]] if b is not None}.values())
        return B

    def launch(self, cfg, B, stream=None):
        a, case = self.rt.abi, self.case
        ptr = lambda b: b.ptr if b is not None else None
        fresh, t, e, nrm = B["ins"]
        p = a.RectifyParams(case["w"], case["h"], *cfg, 0)
        hits = a.HitBuffers(t.ptr, e.ptr, nrm.ptr)
        h_ab, o_ab = a.AccumBuffers(*[B["hist"][k].ptr for k, _ in rh.KEYS]), a.AccumBuffers(*[B["out"][k].ptr for k, _ in rh.KEYS])
        return self.rt.lib.load().rtowRectifyHistoryDevice(self.ctx.handle, C.byref(p), C.byref(h_ab), fresh.ptr, C.byref(hits), ptr(B["m_in"]), C.byref(o_ab),
                                                           ptr(B["m_out"]), ptr(B["keep"]), ptr(B["stats"]), stream)

    def collect(self, B):
        """-> {name: array} of what the mode writes; guard words and read-only inputs checked"""
        case, mode = self.case, B["mode"]
        n = case["n"]
        got = {k: B["out"][k].download(F, (n, SHAPES[k]) if SHAPES[k] > 1 else (n,)) for k, _ in rh.KEYS}
        got["moments"] = B["m_out"].download(F, (n, 3)) if B["m_out"] else None
        got["keep"] = B["keep"].download(F, (n,)) if B["keep"] else None
        got["stats"] = B["stats"].download(np.uint32, (4,)) if B["stats"] else None
        for b in B["own"] + B["ins"]:
            assert b.guards_intact(), mode
        if mode != "in":                                                  # the inputs are read only
            for k, _ in rh.KEYS:
                assert np.array_equal(B["hist"][k].download(np.uint32, (n * SHAPES[k],)), _bits(case["history"][k]).ravel()), (k, mode)
            if B["m_in"]:
                assert np.array_equal(B["m_in"].download(np.uint32, (n * 3,)), _bits(case["moments"]).ravel())
        return got

    def run(self, cfg, mode):
        B = self.prepare(mode)
        try:
            rc = self.launch(cfg, B)
            assert rc == self.rt.abi.RTOW_SUCCESS, (rc, cfg, mode)
            self.ctx.synchronize()
            return self.collect(B)
        finally:
            for b in B["own"]:
                b.free()

    def free(self):
        for bufs in self.ins.values():
            for b in bufs:
                b.free()


def _compare(got, want, mode, what):
    for k, _ in rh.KEYS:
        _assert_same(got[k], want[k], (what, mode, k))
    if mode != "nomoments":
        _assert_same(got["moments"], want["moments"], (what, mode, "moments"))
    else:
        assert got["moments"] is None
    if mode != "bare":
        _assert_same(got["keep"], want["keep"], (what, mode, "keep"))
        assert np.array_equal(got["stats"], want["stats"]), (what, mode, got["stats"], want["stats"])


@pytest.mark.parametrize("w,h", rh.SIZES)
def test_bit_exact_against_the_restatement(rt, gpu_context, w, h):
    """Every configuration - radius 1, 2 and 3 with MATCH_ENTITY on and off - at every size, in every mode: all four accumulators, the moments, outKeep and outStats,
    every pixel.  The inputs hold NaN and infinite channels, w of 0, 0.5 and 1, sky pixels, zero normals and a whole tile of holes, and every outcome covers 5 % of
    the pixels of the larger cases (tests/test_rectify_history_reference.py asserts both on the CPU)."""
    case = rh.make_case(w, h, rh.case_seed(w, h))
    run = Rectify(rt, gpu_context, case)
    try:
        for cfg in rh.CONFIGS:
            want = rh.reference(case, cfg)
            for mode in MODES:
                _compare(run.run(cfg, mode), want, mode, ((w, h), cfg))
    finally:
        run.free()


@pytest.mark.parametrize("w,h", [(70, 10), (131, 9)])
def test_a_frame_of_holes_is_copied_through(rt, gpu_context, w, h):
    """No tile has a valid history: every tile takes the early exit, nothing is judged, the outputs are the inputs (zeros) and outKeep is 1 everywhere."""
    case = rh.make_case(w, h, 5, holes="all")
    run = Rectify(rt, gpu_context, case)
    try:
        want = rh.reference(case, rh.CONFIGS[0])
        assert (want["stats"] == 0).all() and (want["keep"] == 1).all()
        for mode in MODES:
            _compare(run.run(rh.CONFIGS[0], mode), want, mode, (w, h))
    finally:
        run.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    case = rh.make_case(320, 44, 77)                                       # 55 tiles: several workgroups add to the record
    run = Rectify(rt, gpu_context, case)
    try:
        a, b = run.run(rh.CONFIGS[0], "out"), run.run(rh.CONFIGS[0], "out")
        for k in SHAPES:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), k
        assert np.array_equal(a["stats"], b["stats"]) and a["stats"][0] == a["stats"][1:].sum() and min(a["stats"]) > 0
        _compare(a, rh.reference(case, rh.CONFIGS[0]), "out", "320 x 44")
    finally:
        run.free()


def test_refusals_enqueue_nothing(rt, gpu_context):
    """Every refusal of the validation list returns RTOW_ERROR_INVALID_VALUE and leaves the outputs' guard pattern as it was."""
    ctx = gpu_context
    lib = rt.lib.load()
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    w, h = 16, 8
    n = w * h
    sizes = {"color": 16, "normal": 12, "albedo": 12, "scw": 4}
    hist = {k: Dev(rt, ctx, n * s) for k, s in sizes.items()}
    out = {k: Dev(rt, ctx, n * s + 16) for k, s in sizes.items()}
    fresh, t, e, nrm, m_in = Dev(rt, ctx, n * 16), Dev(rt, ctx, n * 4), Dev(rt, ctx, n * 4), Dev(rt, ctx, n * 12), Dev(rt, ctx, n * 12)
    m_out, keep, stats = Dev(rt, ctx, n * 12 + 16), Dev(rt, ctx, n * 4), Dev(rt, ctx, 16)
    everything = list(hist.values()) + list(out.values()) + [fresh, t, e, nrm, m_in, m_out, keep, stats]
    good = (w, h, 2, 4, 2, 0.05, 1.0, 0.125, 1, 0)
    try:
        def call(values=good, context=True, **over):
            ptr = {"params": True, "history": True, "hits": True, "out": True, "fresh": fresh.ptr, "t": t.ptr, "e": e.ptr, "n": nrm.ptr, "m_in": m_in.ptr,
                   "m_out": m_out.ptr, "keep": keep.ptr, "stats": stats.ptr}
            ptr.update({"h" + k: hist[k].ptr for k in sizes})
            ptr.update({"o" + k: out[k].ptr for k in sizes})
            ptr.update(over)
            p = a.RectifyParams(*values)
            hits = a.HitBuffers(ptr["t"], ptr["e"], ptr["n"])
            h_ab, o_ab = a.AccumBuffers(*[ptr["h" + k] for k in sizes]), a.AccumBuffers(*[ptr["o" + k] for k in sizes])
            return lib.rtowRectifyHistoryDevice(ctx.handle if context else None, C.byref(p) if ptr["params"] else None, C.byref(h_ab) if ptr["history"] else None,
                                                ptr["fresh"], C.byref(hits) if ptr["hits"] else None, ptr["m_in"], C.byref(o_ab) if ptr["out"] else None, ptr["m_out"],
                                                ptr["keep"], ptr["stats"], None)

        assert call(context=False) == bad
        for name in ["params", "history", "fresh", "hits", "out", "t", "e", "n"] + ["h" + k for k in sizes] + ["o" + k for k in sizes]:
            assert call(**{name: None}) == bad, name
        for index, value in ((0, 0), (0, -1), (1, 0), (2, 0), (2, 4), (2, -1), (3, 1), (3, 26), (3, 0), (4, -1), (4, 9), (5, -0.01), (5, float("nan")), (5, float("inf")),
                             (6, -1.0), (6, float("nan")), (6, float("inf")), (7, -0.5), (7, float("nan")), (7, float("inf")), (8, 2), (8, 3), (8, -1), (9, 1)):
            p = list(good)
            p[index] = value
            assert call(tuple(p)) == bad, (index, value)
        assert call((w, h, 1, 10, 2, 0.05, 1.0, 0.125, 1, 0)) == bad and call((w, h, 3, 50, 2, 0.05, 1.0, 0.125, 1, 0)) == bad      # minTaps above (2 r + 1)^2
        assert call((65536, 32768, 2, 4, 2, 0.05, 1.0, 0.125, 1, 0)) == bad          # width * height > INT32_MAX
        assert call(m_in=None) == bad and call(m_out=None) == bad                    # exactly one of the two
        reads = {"fresh": fresh, "t": t, "e": e, "n": nrm}
        for target in ("ocolor", "onormal", "oalbedo", "oscw", "m_out", "keep", "stats"):
            for name, b in reads.items():
                assert call(**{target: b.ptr}) == bad, (target, "over", name)
        for k in sizes:                                                              # an output over a history member that is not its own, or over its own but shifted
            for k2 in sizes:
                if k2 != k:
                    assert call(**{"o" + k: hist[k2].ptr}) == bad, (k, k2)
            assert call(**{"o" + k: hist[k].ptr + 4}) == bad, k
            assert call(keep=hist[k].ptr) == bad and call(stats=hist[k].ptr) == bad and call(m_out=hist[k].ptr) == bad, k
        assert call(m_out=m_in.ptr + 12) == bad and call(ocolor=m_in.ptr) == bad and call(keep=m_in.ptr + 4) == bad
        assert call(keep=out["color"].ptr + 8) == bad and call(stats=out["scw"].ptr) == bad and call(m_out=out["normal"].ptr + 4) == bad      # outputs over each other
        assert call(onormal=out["albedo"].ptr) == bad and call(stats=keep.ptr + 4 * (n - 1)) == bad
        ctx.synchronize()
        for b in everything:
            assert (b.words() == GUARD).all()
        # and the calls these were variations of are accepted
        data = {"color": np.ones((n, 4), F), "normal": np.ones((n, 3), F), "albedo": np.ones((n, 3), F), "scw": np.ones(n, F)}
        for b, x in [(hist[k], data[k]) for k in sizes] + [(fresh, np.ones((n, 4), F)), (t, np.ones(n, F)), (e, np.zeros(n, np.int32)), (nrm, np.ones((n, 3), F)),
                                                             (m_in, np.ones((n, 3), F))]:
            b.buf.upload(np.concatenate([np.full(b.front // 4, GUARD, np.uint32), _bits(x).ravel(), np.full(4, GUARD, np.uint32)]))
        ok = a.RTOW_SUCCESS
        assert call() == ok and call(m_in=None, m_out=None, keep=None, stats=None) == ok
        assert call(m_out=m_in.ptr, **{"o" + k: hist[k].ptr for k in sizes}) == ok and call(ocolor=hist["color"].ptr) == ok
        ctx.synchronize()
    finally:
        for b in everything:
            b.free()


def test_the_call_replays_from_a_captured_graph(rt, gpu_context):
    """The clear of the record and the launch captured on a caller's stream (a linear capture: the call neither allocates nor waits) and replayed once: every output
    equals the restatement, bit for bit."""
    ctx = gpu_context
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, C.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(vp), vp, vp, vp, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [vp, vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    for f in (hip.hipGraphExecDestroy, hip.hipGraphDestroy, hip.hipStreamDestroy):
        f.argtypes = [vp]
    case = rh.make_case(131, 9, rh.case_seed(131, 9))
    cfg = rh.CONFIGS[0]
    want = rh.reference(case, cfg)
    run = Rectify(rt, ctx, case)
    side, graph, exe = vp(), vp(), vp()
    held = None
    try:
        held = run.prepare("out")                                                  # every allocation and upload before the capture
        ctx.synchronize()
        assert hip.hipStreamCreate(C.byref(side)) == 0
        assert hip.hipStreamBeginCapture(side, 2) == 0                             # hipStreamCaptureModeRelaxed
        try:
            assert run.launch(cfg, held, side) == rt.abi.RTOW_SUCCESS
        finally:
            assert hip.hipStreamEndCapture(side, C.byref(graph)) == 0
        assert all((held["out"][k].words() == GUARD).all() for k, _ in rh.KEYS) and (held["stats"].words() == GUARD).all(), "capturing runs nothing"
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert hip.hipGraphLaunch(exe, side) == 0
        assert hip.hipStreamSynchronize(side) == 0
        _compare(run.collect(held), want, "out", "replayed")
    finally:
        if side:
            hip.hipStreamSynchronize(side)
        if exe:
            hip.hipGraphExecDestroy(exe)
        if graph:
            hip.hipGraphDestroy(graph)
        if side:
            hip.hipStreamDestroy(side)
        if held:
            for b in held["own"]:
                b.free()
        run.free()


# ---------------------------------------------------------------- what the pass is worth on the cover scene

ORBIT_DEGREES = 4.0
MOVES = ("dolly", "orbit")
SEEDS = (0, 1000, 2000)


def moved_view(rt, scene, move):
    """the cover scene's camera after the move: "dolly" = 2 % of the way to its target (the move of the reprojection and temporal-moments tests), "orbit" =
    ORBIT_DEGREES about the target around the up axis - far enough for reflections to shift on the spheres"""
    S = rt.scenes
    cam = scene.camera
    position, target, up = (np.asarray(cam[k], np.float64) for k in ("position", "target", "up"))
    focus = S.focus_distance(scene, np.asarray(cam["position"], F), S._normalize(np.asarray(cam["target"], F) - np.asarray(cam["position"], F)))
    if move == "dolly":
        new = position + 0.02 * (target - position)
    else:
        axis, v, ang = up / np.linalg.norm(up), position - target, np.radians(ORBIT_DEGREES)
        new = target + v * np.cos(ang) + np.cross(axis, v) * np.sin(ang) + axis * np.dot(axis, v) * (1 - np.cos(ang))       # Rodrigues
    return rr.make_view(tuple(new), tuple(target), W, H, vfov=cam["vfov"], focus=focus, up=tuple(cam["up"]))


def luminance64(c):
    c = c.astype(np.float64)
    return 0.2126 * c[:, 0] + 0.7152 * c[:, 1] + 0.0722 * c[:, 2]


class RectifyFrame(Rig):
    """The issue's protocol on the cover scene at 192 x 108: view A a group of 16 x 4 spp (seeds seed + 1 ..) with its moments; the camera moves; accumulators and
    moments reprojected with their recommended values; at the new view a group of 4 x 1 spp (seeds seed + 201 ..) rendered from zero - the fresh samples.  Reference:
    1024 spp of the new view (seed + 9).  frame(kind) builds one of three frames - "carried" (history as it arrived, plus the fresh sums), a tuple of
    rtowRectifyHistoryDevice's eight parameters (history rectified first), "restarted" (the fresh sums alone) - with its moments (the fresh batches accumulated onto
    the frame's history moments, then rtowEstimateMomentsDevice's recommended set), and returns its combined colour and that colour after rtowDenoiseVarianceDevice's
    recommended set.  errors() is the squared luminance error against the reference over all pixels, over those whose first hit is metal or glass
    (rtowShadeHitsDevice: a dielectric, or a standard material with metallic >= 0.5) and over the rest."""

    def __init__(self, rt, ctx, seed, move):
        super().__init__(rt, ctx)
        n = W * H
        a = rt.abi
        scene = rt.scenes.cover_scene()
        ctx.upload_scene(scene.desc())
        pa = _params_at(rt, scene, None, None, 4, seed + 1)
        view_b, lens = moved_view(rt, scene, move), pa.view.lensRadius
        group_a = _group(rt, ctx, [_params_at(rt, scene, None, None, 4, seed + 1 + k) for k in range(16)])
        group_b = _group(rt, ctx, [_params_at(rt, scene, view_b, lens, 1, seed + 201 + k) for k in range(4)])
        ref = rt.sample_batch_host(ctx, _params_at(rt, scene, view_b, lens, 1024, seed + 9), want_diag=False)
        hits_a = ctx.trace_view(pa.view, W, H, want=("distance", "entityIndex"))
        hits_b = ctx.trace_view(view_b, W, H, want_rays=True)
        surface = ctx.shade_hits(hits_b["rays"], hits_b["entityIndex"], outputs=("metallicGlossiness", "materialInfo"))
        info = surface["materialInfo"]
        hit = info != a.MATERIAL_INFO_MISS
        self.specular = hit & (((info & a.MATERIAL_INFO_TYPE_MASK) == a.MATERIAL_DIELECTRIC) | (surface["metallicGlossiness"][:, 0] >= 0.5))
        job = rt.ReprojectJob(ctx, W, H, pa.view)
        job.Rays, job.HitDistance, job.HitEntityIndex = self.up(hits_b["rays"]), self.up(hits_b["distance"]), self.up(hits_b["entityIndex"])
        job.PreviousHitDistance, job.PreviousHitEntityIndex = self.up(hits_a["distance"]), self.up(hits_a["entityIndex"])
        job.PreviousColor, job.PreviousNormal, job.PreviousAlbedo, job.PreviousSampleCountWeight = [self.up(x) for x in _fold(group_a)]
        self.hist = [self.room(n * k * 4) for _, k in KEYS]
        job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = self.hist
        job.OutputSource = src = self.room(n * 4)
        assert job.Schedule().Complete() == 0
        self.hist_m = self.room(n * 12)
        rj = rt.ReprojectMomentsJob(ctx, n)
        rj.Source, rj.PreviousMoments, rj.OutputMoments = src, self.up(dv.accumulate_moments([b[0] for b in group_a])), self.hist_m
        assert rj.Schedule().Complete() == 0
        self.hits = (job.HitDistance, job.HitEntityIndex, self.up(hits_b["normal"]))
        self.fresh = [self.up(x) for x in _fold(group_b)]
        self.batch_colors = [self.up(b[0]) for b in group_b]
        self.acc = [self.room(n * k * 4) for _, k in KEYS]
        self.mom, self.est = self.room(n * 12), self.room(n * 12)
        self.keep, self.stats = self.room(n * 4), self.room(16)
        self.comb = [self.room(n * 12) for _ in range(3)]
        ctx.synchronize()
        self.carried_share = float((src.download(np.int32, (n,)) >= 0).mean())
        self._combine([self.up(ref[k]) for k in ("color", "normal", "albedo")])
        self.reference = luminance64(self.comb[0].download(F, (n, 3)))

    def _combine(self, acc):
        cj = self.rt.CombineJob(self.ctx, (W, H))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = acc[:3]
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = self.comb
        assert cj.Schedule().Complete() == 0
        self.ctx.synchronize()

    def frame(self, kind):
        """-> (combined colour (n, 3), denoised colour (n, 3), abi.RectifyStats or None)"""
        rt, ctx, n = self.rt, self.ctx, W * H
        lib, a = rt.lib.load(), rt.abi
        m_in = None
        if kind == "restarted":
            for b in self.acc:
                b.zero()
        elif kind == "carried":
            for dst, src, (_, k) in zip(self.acc, self.hist, KEYS):
                assert lib.rtowDeviceCopy(ctx.handle, src.ptr, dst.ptr, n * k * 4, 3) == 0
            assert lib.rtowDeviceCopy(ctx.handle, self.hist_m.ptr, self.mom.ptr, n * 12, 3) == 0
            m_in = self.mom
        else:
            radius, taps, sharp, tol, sigma, rel, flags = kind
            job = rt.RectifyHistoryJob(ctx, W, H, radius, taps, sharp, tol, sigma, rel, flags)
            job.HistoryColor, job.HistoryNormal, job.HistoryAlbedo, job.HistorySampleCountWeight = self.hist
            job.Fresh, (job.HitDistance, job.HitEntityIndex, job.HitNormal) = self.fresh[0], self.hits
            job.InputMoments, job.OutputMoments, job.OutputKeep, job.OutputStats = self.hist_m, self.mom, self.keep, self.stats
            job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = self.acc
            assert job.Schedule().Complete() == 0
            m_in = self.mom
        ctx.synchronize()
        stats = None if isinstance(kind, str) else a.RectifyStats.from_buffer_copy(self.stats.download(np.uint8, (16,)).tobytes())
        mj = rt.MomentsJob(ctx, n)
        mj.Colors, mj.InputMoments, mj.OutputMoments = self.batch_colors, m_in, self.mom
        assert mj.Schedule().Complete() == 0
        dst, src = a.AccumBuffers(*[b.ptr for b in self.acc]), a.AccumBuffers(*[b.ptr for b in self.fresh])
        assert lib.rtowAddAccumDevice(ctx.handle, n, C.byref(dst), C.byref(src), None) == 0
        self.estimate(recommended_estimate(a), self.acc[0], self.hits, self.mom, self.est, None)
        self._combine(self.acc)
        noisy = self.comb[0].download(F, (n, 3))
        return noisy, self.denoise_variance(self.comb, self.est), stats

    def errors(self, colour):
        """squared luminance error against the reference: (all pixels, specular first hits, the rest)"""
        e = (luminance64(colour) - self.reference) ** 2
        return float(e.mean()), float(e[self.specular].mean()), float(e[~self.specular].mean())


def recommended_rectify(a):
    return (a.RECTIFY_DEFAULT_RADIUS, a.RECTIFY_DEFAULT_MIN_TAPS, a.RECTIFY_DEFAULT_NORMAL_SHARPNESS, a.RECTIFY_DEFAULT_DEPTH_TOLERANCE, a.RECTIFY_DEFAULT_SIGMA_SCALE,
            a.RECTIFY_DEFAULT_RELATIVE_TOLERANCE, a.RECTIFY_DEFAULT_FLAGS)


# Measured on an MI355X with the recommended parameters (profiles/r15_rectify_history.json, "recommended_set_in_abi"): the squared luminance error of the rectified frame
# over that of the carried frame on the pixels whose first hit is metal or glass, per move: (mean over seeds 0 / 1000 / 2000, the per-seed values).
#   orbit: below 1 on all three seeds - a gain, a small one; the test asserts it with the spread over the seeds (largest minus smallest) as its margin.
#   dolly: 0.9991 (1.0033 / 0.9954 / 0.9988) - NOT below 1 on all three seeds: a measured "no gain".  After a 2 % dolly what the history carries is worth ten times
#   the fresh samples even on metal and glass (restarted / carried = 10.4 / 10.1 / 12.3 there), and what is stale in it is too small a part of the error to show.
#   The test asserts nothing more for that move.
MEASURED = {"dolly": None, "orbit": (0.9766, (0.9798, 0.9682, 0.9817))}


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("move", MOVES)
def test_quality_after_a_camera_move_on_the_cover_scene(rt, gpu_context, move, seed):
    """RectifyFrame's protocol with the recommended values: the three frames (carried, rectified, restarted) before and after rtowDenoiseVarianceDevice, their squared
    luminance errors against 1024 spp over all pixels, the specular first hits and the rest.  Exact: the device's four counts are the restatement's.
    Every ratio is finite; on the orbit the rectified frame differs from the carried one; where MEASURED holds a gain for the move, (b) / (a) on the specular pixels is
    within it."""
    a = rt.abi
    frame = RectifyFrame(rt, gpu_context, seed, move)
    try:
        cfg = recommended_rectify(a)
        res = {kind: frame.frame(k) for kind, k in (("carried", "carried"), ("rectified", cfg), ("restarted", "restarted"))}
        n = W * H
        hist = {key: b.download(F, (n, k) if k > 1 else (n,)) for b, (key, k) in zip(frame.hist, KEYS)}
        hist_m, fresh = frame.hist_m.download(F, (n, 3)), frame.fresh[0].download(F, (n, 4))
        hits = tuple(b.download(np.int32 if i == 1 else F, (n, 3) if i == 2 else (n,)) for i, b in enumerate(frame.hits))
        job_stats = res["rectified"][2]
    finally:
        frame.free()
    want = rh.rectify(W, H, hist, fresh, hits, hist_m, *cfg)
    assert [job_stats.judged, job_stats.kept, job_stats.cut, job_stats.dropped] == list(want["stats"]), (list(want["stats"]), job_stats.judged)
    assert 0 < job_stats.kept <= job_stats.judged <= int((hist["color"][:, 3] >= 1).sum())        # only a pixel with a history of a sample or more is judged
    err = {kind: (frame.errors(noisy), frame.errors(den)) for kind, (noisy, den, _) in res.items()}
    ratios = {}
    for stage, name in ((0, "noisy"), (1, "denoised")):
        for region, label in enumerate(("all", "specular", "rest")):
            base = err["carried"][stage][region]
            ratios[(name, label)] = (err["rectified"][stage][region] / base, err["restarted"][stage][region] / base)
    print("rectify %s seed %d: carried %.4f of the pixels, specular %.4f; judged %d kept %d cut %d dropped %d" % (
        move, seed, frame.carried_share, frame.specular.mean(), job_stats.judged, job_stats.kept, job_stats.cut, job_stats.dropped))
    for key, (b_over_a, c_over_a) in ratios.items():
        print("  %-8s %-8s (b)/(a) %.4f  (c)/(a) %.4f" % (key + (b_over_a, c_over_a)))
        assert np.isfinite(b_over_a) and np.isfinite(c_over_a), key
    if move == "orbit":
        assert job_stats.cut + job_stats.dropped > 0 and not np.array_equal(res["rectified"][0], res["carried"][0])
    if MEASURED[move] is not None:
        mean, per_seed = MEASURED[move]
        bound = min(1.0, mean + (max(per_seed) - min(per_seed)))          # the margin: the spread over the seeds; never above 1
        assert ratios[("noisy", "specular")][0] <= bound, (ratios[("noisy", "specular")][0], bound)
