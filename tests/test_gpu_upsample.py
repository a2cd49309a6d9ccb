"""GPU tests of rtowUpsampleDevice (include/rtow.h): the kernels bit for bit against the numpy restatement of the specification (tests/upsample_reference.py),
colour and stage map, on generated inputs that need no scene; guard bytes, refusals, determinism, the combine -> denoise -> upsample -> finalize chain on a caller's
stream against the oracle, and the gain over the point blit on the cover scene.  All in the session context, no subprocesses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402
import upsample_reference as ur  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 0xA5
PAD = 16


class Dev:
    """a device array `offset` bytes into its allocation, with guard bytes before and after it"""

    def __init__(self, rt, ctx, nbytes, offset=0, data=None, fill=GUARD):
        self.rt, self.ctx, self.nbytes, self.front = rt, ctx, nbytes, PAD + offset
        self.total = (self.front + nbytes + PAD + 3) // 4 * 4
        self.buf = rt.DeviceBuffer(ctx, self.total)
        host = np.full(self.total, GUARD, np.uint8)
        host[self.front: self.front + nbytes] = np.ascontiguousarray(data).view(np.uint8).ravel() if data is not None else fill
        self.buf.upload(host)

    @property
    def ptr(self):
        return self.buf.ptr + self.front

    def raw(self):
        return self.buf.download(np.uint8, (self.total,))

    def download(self, dtype, shape):
        return self.raw()[self.front: self.front + self.nbytes].copy().view(dtype).reshape(shape)

    def guards_intact(self):
        x = self.raw()
        return (x[: self.front] == GUARD).all() and (x[self.front + self.nbytes:] == GUARD).all()

    def free(self):
        self.buf.free()


class Call:
    """the eleven device buffers of one call: float arrays `offset` bytes into their allocations, the stage map at an odd address"""

    def __init__(self, rt, ctx, case, offset=0, stage=True):
        self.rt, self.ctx, self.case = rt, ctx, case
        nd = case["dw"] * case["dh"]
        mk = lambda data: Dev(rt, ctx, np.ascontiguousarray(data).nbytes, offset, data)
        st, se, sn = case["src_hits"]
        dt, de, dn = case["dst_hits"]
        self.ins = {"c": mk(case["src_color"]), "st": mk(st), "se": mk(se), "sn": mk(sn), "sa": mk(case["src_albedo"]),
                    "dt": mk(dt), "de": mk(de), "dn": mk(dn), "da": mk(case["dst_albedo"])}
        self.out = Dev(rt, ctx, nd * 12, offset)
        self.stage = Dev(rt, ctx, nd, 1 + offset // 4 * 2)                # byte offsets 1 and 3
        self.with_stage = stage

    def run(self, cfg, stream=None, ctx_handle=-1, params=True, **over):
        a, c = self.rt.abi, self.case
        mode, sharp, tol, flags = cfg
        p = a.UpsampleParams(over.get("sw", c["sw"]), over.get("sh", c["sh"]), over.get("dw", c["dw"]), over.get("dh", c["dh"]), mode, sharp, tol, flags,
                             over.get("reserved", 0))
        ptr = {k: v.ptr for k, v in self.ins.items()}
        ptr.update({"out": self.out.ptr, "stage": self.stage.ptr if self.with_stage else None})
        ptr.update({k: v for k, v in over.items() if k in ptr})
        src_hits, dst_hits = a.HitBuffers(ptr["st"], ptr["se"], ptr["sn"]), a.HitBuffers(ptr["dt"], ptr["de"], ptr["dn"])
        return self.rt.lib.load().rtowUpsampleDevice(self.ctx.handle if ctx_handle == -1 else ctx_handle, C.byref(p) if params else None, ptr["c"],
                                                     C.byref(src_hits) if over.get("src_hits", True) else None, ptr["sa"],
                                                     C.byref(dst_hits) if over.get("dst_hits", True) else None, ptr["da"], ptr["out"], ptr["stage"], stream)

    def results(self):
        nd = self.case["dw"] * self.case["dh"]
        self.ctx.synchronize()
        return self.out.download(F, (nd, 3)), self.stage.download(np.uint8, (nd,))

    def everything(self):
        return list(self.ins.values()) + [self.out, self.stage]

    def free(self):
        for b in self.everything():
            b.free()


def _compare(got, got_stage, want, want_stage, what):
    bad = np.flatnonzero(got_stage != want_stage)
    assert bad.size == 0, (what, "stage", bad.size, bad[:5], got_stage[bad[:5]], want_stage[bad[:5]])
    bad = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(1))
    assert bad.size == 0, (what, "colour", bad.size, bad[:5], got[bad[:3]], want[bad[:3]], want_stage[bad[:5]])


def _check(rt, ctx, src, dst, configs):
    """every configuration on the pair's one case; buffers 4 bytes into their allocations in every other configuration"""
    case = ur.make_case(*src, *dst, ur.case_seed(src, dst))
    calls = {off: Call(rt, ctx, case, off) for off in (0, 4)}
    try:
        for k, cfg in enumerate(configs):
            want, want_stage, rejected = ur.reference(case, *cfg)
            if cfg[0] == ur.GUIDED and want_stage.size >= ur.COVERAGE_MIN_PIXELS:
                cov = ur.coverage(want_stage, rejected, cfg[3])
                print("upsample %s -> %s %s: %s" % (src, dst, cfg, cov))
                assert ur.coverage_ok(cov), (src, dst, cfg, cov)                  # a case that does not cover the stages is a broken test
            call = calls[4 if k % 2 else 0]
            assert call.run(cfg) == rt.abi.RTOW_SUCCESS
            got, got_stage = call.results()
            _compare(got, got_stage, want, want_stage, (src, dst, cfg))
            for b in call.everything():
                assert b.guards_intact()
    finally:
        for call in calls.values():
            call.free()


@pytest.mark.parametrize("src,dst", ur.SIZE_PAIRS)
def test_bit_exact_against_the_restatement(rt, gpu_context, src, dst):
    _check(rt, gpu_context, src, dst, ur.CONFIGS)


def test_bit_exact_at_1080p(rt, gpu_context):
    """960 x 540 -> 1920 x 1080: 32400 tiles, twice what the grid holds, so the grid-stride loop runs"""
    _check(rt, gpu_context, *ur.LARGE_PAIR, ur.LARGE_CONFIGS)


def test_without_out_stage_nothing_is_written_there(rt, gpu_context):
    src, dst = (13, 7), (37, 29)
    case = ur.make_case(*src, *dst, 5)
    cfg = ur.CONFIGS[3]
    want, _, _ = ur.reference(case, *cfg)
    call = Call(rt, gpu_context, case, 4, stage=False)
    try:
        assert call.run(cfg) == rt.abi.RTOW_SUCCESS
        got, _ = call.results()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (call.stage.raw() == GUARD).all()                      # the array a call WITH outStage would have written
        for b in call.everything():
            assert b.guards_intact()
    finally:
        call.free()


def test_refusals_enqueue_nothing(rt, gpu_context):
    a = rt.abi
    P, B, G, M, D = a.RTOW_UPSAMPLE_POINT, a.RTOW_UPSAMPLE_BILINEAR, a.RTOW_UPSAMPLE_GUIDED, a.RTOW_UPSAMPLE_MATCH_ENTITY, a.RTOW_UPSAMPLE_DEMODULATE_ALBEDO
    bad = a.RTOW_ERROR_INVALID_VALUE
    case = ur.make_case(8, 4, 16, 8, 3)
    ns, nd = 32, 128
    good = (G, 4, 0.05, M | D)
    call = Call(rt, gpu_context, case)
    try:
        for name in ("c", "st", "se", "sn", "sa", "dt", "de", "dn", "da", "out"):
            assert call.run(good, **{name: None}) == bad, name
        assert call.run(good, src_hits=False) == bad and call.run(good, dst_hits=False) == bad
        assert call.run(good, ctx_handle=None) == bad and call.run(good, params=False) == bad
        for size in ({"sw": 0}, {"sh": 0}, {"dw": 0}, {"dh": 0}, {"sw": -1}, {"dh": -3}, {"sw": 16385}, {"sh": 16385}, {"dw": 16385}, {"dh": 16385}):
            assert call.run(good, **size) == bad, size
        for cfg in ((3, 4, 0.05, 0), (-1, 4, 0.05, 0), (G, -1, 0.05, M), (G, 9, 0.05, M), (G, 4, -0.01, M), (G, 4, float("nan"), M), (G, 4, float("inf"), M),
                    (G, 4, 0.05, 4), (G, 4, 0.05, 8 | M), (G, 4, 0.05, -1), (P, 0, 0.0, M), (P, 0, 0.0, D), (B, 0, 0.0, M), (B, 0, 0.0, M | D)):
            assert call.run(cfg) == bad, cfg
        assert call.run(good, reserved=1) == bad and call.run(good, reserved=-1) == bad
        # an output on an input the mode reads, or on the other output; partial overlaps by one element
        ins = call.ins
        for over in ({"out": ins["c"].ptr}, {"out": ins["c"].ptr + ns * 12 - 4}, {"stage": ins["st"].ptr + ns * 4 - 1}, {"out": ins["se"].ptr - nd * 12 + 4},
                     {"stage": ins["sn"].ptr}, {"out": ins["sa"].ptr + 8}, {"stage": ins["dt"].ptr + 3}, {"out": ins["de"].ptr}, {"out": ins["dn"].ptr + nd * 12 - 4},
                     {"stage": ins["da"].ptr + 1}, {"stage": call.out.ptr + nd * 12 - 1}, {"stage": call.out.ptr - nd + 1}):
            assert call.run(good, **over) == bad, over
        gpu_context.synchronize()
        for b in (call.out, call.stage):
            assert (b.raw() == GUARD).all()                           # nothing was enqueued
        # pointers a mode does not read are ignored: BILINEAR without hits or albedos, on buffers a guided call may not alias
        assert call.run((B, 0, 0.0, 0), src_hits=False, dst_hits=False, sa=None, da=None) == a.RTOW_SUCCESS
        got, got_stage = call.results()
        want, want_stage, _ = ur.reference(case, B, 0, 0.0, 0)
        _compare(got, got_stage, want, want_stage, "bilinear without guides")
        assert call.run(good) == a.RTOW_SUCCESS
        got, got_stage = call.results()
        want, want_stage, _ = ur.reference(case, *good)
        _compare(got, got_stage, want, want_stage, "after the refusals")
    finally:
        call.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    case = ur.make_case(160, 90, 320, 180, 9)
    res = []
    for _ in range(2):
        call = Call(rt, gpu_context, case)
        try:
            assert call.run(ur.CONFIGS[3]) == rt.abi.RTOW_SUCCESS
            res.append(call.results())
        finally:
            call.free()
    assert np.array_equal(res[0][0].view(np.uint32), res[1][0].view(np.uint32)) and np.array_equal(res[0][1], res[1][1])


def _render(rt, ctx, scene, w, h, spp, seed):
    return rt.sample_batch_host(ctx, rt.scenes.make_params(scene, w, h, spp=spp, trace_depth=8, seed=seed), want_diag=False)


def _guides(rt, ctx, params, w, h):
    """first-hit guides of the batch's view at w x h: trace-view's distance, entity and normal, shade-hits' albedo"""
    hits = ctx.trace_view(params.view, w, h, want_rays=True)
    hits["albedo"] = ctx.shade_hits(hits["rays"], hits["entityIndex"], params.environment, outputs=("albedo",))["albedo"]
    return hits


def _hits(g):
    return g["distance"], g["entityIndex"], g["normal"]


def test_combine_denoise_upsample_finalize_chain_on_a_caller_stream(rt, oracle, gpu_context):
    """rtowCombineDevice -> rtowDenoiseDevice at 96 x 54, rtowUpsampleDevice (recommended parameters) to 192 x 108, rtowFinalizeDevice there, enqueued back to back on a
    caller-owned stream with no synchronisation in between: the RGBA32 bytes equal oracle.finalize(upsample(denoise_reference(oracle.combine(...))))."""
    ctx = gpu_context
    scene = rt.scenes.cover_scene()
    ctx.upload_scene(scene.desc())
    (sw, sh), (dw, dh) = (96, 54), (192, 108)
    ns, nd = sw * sh, dw * dh
    a = rt.abi
    params = rt.scenes.make_params(scene, sw, sh, spp=4, trace_depth=8, seed=3)
    acc = rt.sample_batch_host(ctx, params, want_diag=False)
    gs, gd = _guides(rt, ctx, params, sw, sh), _guides(rt, ctx, params, dw, dh)
    bufs = []

    def up(x):
        bufs.append(rt.DeviceBuffer(ctx).upload(np.ascontiguousarray(x)))
        return bufs[-1]

    def room(nbytes):
        bufs.append(rt.DeviceBuffer(ctx, nbytes))
        return bufs[-1]

    hip = C.CDLL("libamdhip64.so")
    side = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(side)) == 0
    try:
        ins = [up(acc[k]) for k in ("color", "normal", "albedo")]
        comb = [room(ns * 12) for _ in range(3)]
        den, scratch, big = room(ns * 12), room(a.denoise_scratch_bytes(sw, sh)), room(nd * 12)
        r8 = [room(nd * 4) for _ in range(3)]
        cj = rt.CombineJob(ctx, (sw, sh))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = ins
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = comb
        dj = rt.DenoiseJob(ctx, sw, sh)
        dj.InputColor, dj.InputNormal, dj.InputAlbedo, dj.Scratch, dj.OutputColor = comb[0], comb[1], comb[2], scratch, den
        uj = rt.UpsampleJob(ctx, sw, sh, dw, dh)
        uj.SrcColor, uj.SrcHitDistance, uj.SrcHitEntityIndex, uj.SrcHitNormal, uj.SrcAlbedo = den, up(gs["distance"]), up(gs["entityIndex"]), up(gs["normal"]), up(gs["albedo"])
        uj.DstHitDistance, uj.DstHitEntityIndex, uj.DstHitNormal, uj.DstAlbedo = up(gd["distance"]), up(gd["entityIndex"]), up(gd["normal"]), up(gd["albedo"])
        uj.OutputColor = big
        fj = rt.FinalizeTexturesJob(ctx, nd)
        fj.InputColor, fj.InputNormal, fj.InputAlbedo = big, uj.DstHitNormal, uj.DstAlbedo
        fj.OutputColor, fj.OutputNormal, fj.OutputAlbedo = r8
        ctx.synchronize()                                               # the uploads above; nothing below waits
        for job in (cj, dj, uj, fj):
            assert job.Schedule(side).Complete() == 0
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        assert hip.hipStreamSynchronize(side) == 0
        oc, on, oa = oracle.combine(sw, sh, acc["color"], acc["normal"], acc["albedo"])
        dref = dr.denoise_reference(sw, sh, oc, on, oa, a.DENOISE_DEFAULT_ITERATIONS, a.DENOISE_DEFAULT_NORMAL_SHARPNESS, a.DENOISE_DEFAULT_COLOR_SIGMA,
                                    a.DENOISE_DEFAULT_ALBEDO_SIGMA, a.DENOISE_DEFAULT_FLAGS)
        uref, stage, _ = ur.upsample(sw, sh, dw, dh, a.UPSAMPLE_DEFAULT_MODE, a.UPSAMPLE_DEFAULT_NORMAL_SHARPNESS, a.UPSAMPLE_DEFAULT_DEPTH_TOLERANCE,
                                     a.UPSAMPLE_DEFAULT_FLAGS, dref, _hits(gs), gs["albedo"], _hits(gd), gd["albedo"])
        assert np.array_equal(big.download(F, (nd, 3)).view(np.uint32), uref.view(np.uint32))
        want = oracle.finalize(uref, gd["normal"], gd["albedo"])
        for got, wv in zip(r8, want):
            assert np.array_equal(got.download(np.uint8, (nd, 4)), wv)
        point, _, _ = ur.upsample(sw, sh, dw, dh, ur.POINT, 0, 0.0, 0, dref)
        assert not np.array_equal(want[0], oracle.finalize(point, gd["normal"], gd["albedo"])[0])        # not the blit's picture
        assert (stage == 0).mean() > 0.5
    finally:
        for b in bufs:
            b.free()
        hip.hipStreamDestroy.argtypes = [C.c_void_p]
        hip.hipStreamDestroy(side)


# the asserted bound of the quality test: the ratio measured on an MI355X times 1.25 for the spread between boxes and seeds, never above 1
MEASURED_RATIO = 0.623
RATIO_BOUND = 1.0 if MEASURED_RATIO is None else min(1.0, 1.25 * MEASURED_RATIO)


def _device_upsample(rt, ctx, size, color, gs, gd, mode, sharp, tol, flags):
    (sw, sh), (dw, dh) = size
    nd = dw * dh
    bufs = [rt.DeviceBuffer(ctx).upload(np.ascontiguousarray(x)) for x in (color, gs["distance"], gs["entityIndex"], gs["normal"], gs["albedo"], gd["distance"],
                                                                             gd["entityIndex"], gd["normal"], gd["albedo"])]
    out, stage = rt.DeviceBuffer(ctx, nd * 12), rt.DeviceBuffer(ctx, nd)
    try:
        job = rt.UpsampleJob(ctx, sw, sh, dw, dh, mode, sharp, tol, flags)
        (job.SrcColor, job.SrcHitDistance, job.SrcHitEntityIndex, job.SrcHitNormal, job.SrcAlbedo, job.DstHitDistance, job.DstHitEntityIndex, job.DstHitNormal,
         job.DstAlbedo) = bufs
        job.OutputColor, job.OutputStage = out, stage
        assert job.Schedule().Complete() == 0
        ctx.synchronize()
        return out.download(F, (nd, 3)), stage.download(np.uint8, (nd,))
    finally:
        for b in bufs + [out, stage]:
            b.free()


def _combine(rt, ctx, w, h, acc):
    n = w * h
    ins = [rt.DeviceBuffer(ctx).upload(acc[k]) for k in ("color", "normal", "albedo")]
    outs = [rt.DeviceBuffer(ctx, n * 12) for _ in range(3)]
    try:
        cj = rt.CombineJob(ctx, (w, h))
        cj.InputColor, cj.InputNormal, cj.InputAlbedo = ins
        cj.OutputColor, cj.OutputNormal, cj.OutputAlbedo = outs
        assert cj.Schedule().Complete() == 0
        ctx.synchronize()
        return [o.download(F, (n, 3)) for o in outs]
    finally:
        for b in ins + outs:
            b.free()


def quality_inputs(rt, ctx):
    """The frames of the quality test (profiles/upsample_timing.py scans the parameter grid on the same ones): the cover scene at resolutionScaling 0.5, 16 spp (seed 1)
    at 96 x 54 and 1024 spp (seed 2) at 192 x 108, both combined on the device; first-hit guides of the batch's view at both sizes."""
    scene = rt.scenes.cover_scene()
    ctx.upload_scene(scene.desc())
    size = ((96, 54), (192, 108))
    (sw, sh), (dw, dh) = size
    p_src = rt.scenes.make_params(scene, sw, sh, spp=16, trace_depth=8, seed=1)
    p_ref = rt.scenes.make_params(scene, dw, dh, spp=1024, trace_depth=8, seed=2)
    src = _combine(rt, ctx, sw, sh, rt.sample_batch_host(ctx, p_src, want_diag=False))
    ref = _combine(rt, ctx, dw, dh, rt.sample_batch_host(ctx, p_ref, want_diag=False))[0].astype(np.float64)
    return size, src, ref, _guides(rt, ctx, p_src, sw, sh), _guides(rt, ctx, p_src, dw, dh)


def test_quality_on_the_cover_scene(rt, gpu_context):
    """dst 192 x 108, src 96 x 54 (the reference scenes' resolutionScaling 0.5): 16 spp at src (seed 1) combined on the device, guides from trace-view and shade-hits at
    both sizes with the batch's view, against 1024 spp at dst (seed 2).  The mean squared error of rtowUpsampleDevice GUIDED with the recommended parameters must be below
    that of the POINT upsampling of the same src colour - what the reference host shows today - by the measured ratio times 1.25.  The ratios of BILINEAR, of GUIDED
    without demodulation and of GUIDED on a denoised src frame, and the share of pixels per stage, are printed.
    Measured on an MI355X: GUIDED 0.623, BILINEAR 0.698, GUIDED without demodulation 0.623, on the denoised frame 0.694 (of that frame's POINT read); stages
    A 99.82 %, B 0.14 %, C 0.05 %."""
    ctx = gpu_context
    a = rt.abi
    size, (c_src, n_src, a_src), ref, gs, gd = quality_inputs(rt, ctx)
    (sw, sh), (dw, dh) = size
    mse = lambda x: float(np.mean((x.astype(np.float64) - ref) ** 2))
    point, _, _ = ur.upsample(sw, sh, dw, dh, ur.POINT, 0, 0.0, 0, c_src)
    mse_a = mse(point)
    rec = (a.UPSAMPLE_DEFAULT_MODE, a.UPSAMPLE_DEFAULT_NORMAL_SHARPNESS, a.UPSAMPLE_DEFAULT_DEPTH_TOLERANCE, a.UPSAMPLE_DEFAULT_FLAGS)
    guided, stage = _device_upsample(rt, ctx, size, c_src, gs, gd, *rec)
    want, want_stage, _ = ur.upsample(sw, sh, dw, dh, *rec, c_src, _hits(gs), gs["albedo"], _hits(gd), gd["albedo"])
    _compare(guided, stage, want, want_stage, "cover scene")
    ratio = mse(guided) / mse_a
    bilinear, _ = _device_upsample(rt, ctx, size, c_src, gs, gd, ur.BILINEAR, 0, 0.0, 0)
    plain, _ = _device_upsample(rt, ctx, size, c_src, gs, gd, ur.GUIDED, rec[1], rec[2], rec[3] & ~ur.DEMODULATE_ALBEDO)
    # the same on a denoised src frame (recommended denoiser settings, trace-view / shade-hits guides): against the POINT upsampling of that denoised frame
    den = dr.denoise_reference(sw, sh, c_src, gs["normal"], gs["albedo"], a.DENOISE_DEFAULT_ITERATIONS, a.DENOISE_DEFAULT_NORMAL_SHARPNESS,
                               a.DENOISE_DEFAULT_COLOR_SIGMA, a.DENOISE_DEFAULT_ALBEDO_SIGMA, a.DENOISE_DEFAULT_FLAGS)
    den_point, _, _ = ur.upsample(sw, sh, dw, dh, ur.POINT, 0, 0.0, 0, den)
    den_guided, _ = _device_upsample(rt, ctx, size, den, gs, gd, *rec)
    shares = [float((stage == k).mean()) for k in range(3)]
    print("upsample quality: POINT MSE %.6g; GUIDED / POINT %.4f, BILINEAR / POINT %.4f, GUIDED without demodulation / POINT %.4f; denoised src: POINT MSE %.6g, "
          "GUIDED / POINT %.4f; stages A %.4f B %.4f C %.4f" % (mse_a, ratio, mse(bilinear) / mse_a, mse(plain) / mse_a, mse(den_point), mse(den_guided) / mse(den_point),
                                                                 *shares))
    assert np.isfinite(guided).all()
    assert ratio < 1.0 and ratio <= RATIO_BOUND, ratio
