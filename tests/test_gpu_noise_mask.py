"""GPU tests of rtowNoiseMaskDevice (include/rtow.h): the mask, outError and every word of the statistics bit for bit against the numpy restatement of the
specification (tests/noise_mask_reference.py) on synthetic moments that need no scene - guard bytes around every output, masks at odd addresses, moments 4 bytes into
their allocation -, determinism, the optional outputs, refusals, the list builder on the mask, the call replayed from a captured graph, and one refinement round and
what refinement is worth on the cover scene.  All in the session context, no subprocesses."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_variance_reference as dv  # noqa: E402
import noise_mask_reference as nm  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = np.frombuffer(np.uint32(0x5AFEC0DE).tobytes(), np.uint8)
STATS_BYTES = 288


class Guarded:
    """`nbytes` of device memory `offset` bytes (any number) into an allocation, guard bytes before and after it - and in it, unless `data` is given"""

    def __init__(self, rt, ctx, nbytes, offset=0, data=None):
        self.front, self.nbytes = 16 + offset, nbytes
        total = (self.front + nbytes + 16 + 3) // 4 * 4
        self.initial = np.tile(GUARD, total // 4)
        if data is not None:
            self.initial[self.front: self.front + nbytes] = np.ascontiguousarray(data).view(np.uint8).ravel()
        self.buf = rt.DeviceBuffer(ctx).upload(self.initial)

    @property
    def ptr(self):
        return self.buf.ptr + self.front

    def raw(self):
        return self.buf.download(np.uint8, (self.initial.size,))

    def read(self, dtype, shape):
        """the payload, after checking the bytes around it"""
        x = self.raw()
        assert np.array_equal(x[: self.front], self.initial[: self.front]), "bytes in front of the buffer"
        assert np.array_equal(x[self.front + self.nbytes:], self.initial[self.front + self.nbytes:]), "bytes behind the buffer"
        return x[self.front: self.front + self.nbytes].copy().view(dtype).reshape(shape)

    def untouched(self):
        return np.array_equal(self.raw(), self.initial)

    def reset(self):
        self.buf.upload(self.initial)

    def free(self):
        self.buf.free()


def _call(rt, ctx, values, moments, mask, error, stats, scratch, stream=None):
    p = rt.abi.NoiseMaskParams(*values)
    ptr = lambda b: b.ptr if isinstance(b, Guarded) else b
    return rt.lib.load().rtowNoiseMaskDevice(ctx.handle, C.byref(p), ptr(moments), ptr(mask), ptr(error), ptr(stats), ptr(scratch), stream)


def _same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = np.flatnonzero((got.view(np.uint8).reshape(len(want), -1) != want.view(np.uint8).reshape(len(want), -1)).any(1))
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


def _budgets(n):
    return sorted({0, 1, n // 4, n})


THRESHOLD = 0.05


@pytest.mark.parametrize("w,h", nm.SIZES)
def test_bit_exact_against_the_restatement(rt, gpu_context, w, h):
    """Both error kinds x dilate 0..3 x both values of UNKNOWN_QUALIFIES x a budget of 0, 1, n / 4 and n, at every size: one pixel, a row and a column shorter than the
    halo, one tile less a pixel, one tile exactly, one past a tile in both directions, three tiles across and down, and a frame.  The moments hold unknown pixels on the
    image border and in tile corners, zero variance, huge n and non-finite triples (tests/noise_mask_reference.py); they start 0 or 4 bytes into their allocation, the
    mask at every byte offset 0..3, outError and outStats at 0 or 4.  Every byte of the mask, every float of outError and every word of the statistics is compared, and
    the bytes around all of them."""
    ctx = gpu_context
    n = w * h
    host = nm.make_moments(w, h, nm.case_seed(w, h))
    moments = [Guarded(rt, ctx, n * 12, off, host) for off in (0, 4)]
    scratch = Guarded(rt, ctx, STATS_BYTES, 0)
    g_of = {}
    calls = 0
    try:
        for absolute in (0, 1):
            for radius in (0, 1, 2, 3):
                floor = 0.0 if radius & 1 else 2.0 ** -6
                if (absolute, floor) not in g_of:
                    g_of[absolute, floor] = nm.filtered_error(w, h, nm.own_error(host, bool(absolute), floor))
                for uq in (0, 2):
                    for budget in _budgets(n):
                        flags = absolute | uq
                        want = nm.noise_mask(w, h, host, THRESHOLD, floor, radius, budget, flags, g=g_of[absolute, floor])
                        if n >= 64 * 4 and budget == 0:
                            assert 0 < want["qualifying"] < n and 0 < want["unknown"] < n and (want["histogram"] > 0).sum() >= 4, (want["qualifying"], want["unknown"])
                        mask = Guarded(rt, ctx, n, calls % 4)
                        error = Guarded(rt, ctx, n * 4, 4 * (calls // 4 % 2))
                        stats = Guarded(rt, ctx, STATS_BYTES, 4 * (calls // 8 % 2))
                        try:
                            what = (w, h, absolute, radius, uq, budget)
                            assert _call(rt, ctx, (w, h, THRESHOLD, floor, radius, budget, flags, 0), moments[calls % 2], mask, error, stats, scratch) == rt.abi.RTOW_SUCCESS, what
                            ctx.synchronize()
                            _same_bits(stats.read(np.uint32, (72,)), want["words"], what + ("stats",))
                            _same_bits(error.read(F, (n,)), want["error"], what + ("outError",))
                            _same_bits(mask.read(np.uint8, (n,)), want["mask"], what + ("mask",))
                            assert moments[calls % 2].untouched(), "the moments are read only"
                        finally:
                            for b in (mask, error, stats):
                                b.free()
                        calls += 1
        scratch.read(np.uint32, (72,))                             # the bytes around the scratch
    finally:
        for b in moments + [scratch]:
            b.free()


def test_errors_on_bin_edges_and_a_budget_no_bin_can_meet(rt, gpu_context):
    """ABSOLUTE errors that are powers of two exactly, in the first and the last bin too: the budget's threshold is a bin edge, and pixels ON it qualify."""
    ctx = gpu_context
    w, h = 70, 6
    n = w * h
    host = nm.power_of_two_bands(w, h)
    moments, scratch = Guarded(rt, ctx, n * 12, 0, host), Guarded(rt, ctx, STATS_BYTES)
    mask, error, stats = Guarded(rt, ctx, n, 1), Guarded(rt, ctx, n * 4), Guarded(rt, ctx, STATS_BYTES)
    try:
        thresholds = set()
        for budget in (0, 1, 3, n // 8, n // 4, n // 2, n):
            want = nm.noise_mask(w, h, host, 2.0 ** -50, 0.0, 1, budget, nm.ABSOLUTE)
            assert _call(rt, ctx, (w, h, 2.0 ** -50, 0.0, 1, budget, nm.ABSOLUTE, 0), moments, mask, error, stats, scratch) == 0
            ctx.synchronize()
            _same_bits(stats.read(np.uint32, (72,)), want["words"], (budget, "stats"))
            _same_bits(error.read(F, (n,)), want["error"], (budget, "outError"))
            _same_bits(mask.read(np.uint8, (n,)), want["mask"], (budget, "mask"))
            thresholds.add(float(want["threshold"]))
        assert np.inf in thresholds and len(thresholds) >= 4, thresholds
    finally:
        for b in (moments, scratch, mask, error, stats):
            b.free()


def test_two_calls_give_identical_bits_and_the_optional_outputs_change_nothing(rt, gpu_context):
    ctx = gpu_context
    w, h = 130, 9
    n = w * h
    host = nm.make_moments(w, h, 77)
    moments, scratch = Guarded(rt, ctx, n * 12, 0, host), Guarded(rt, ctx, STATS_BYTES)
    outs = [[Guarded(rt, ctx, n, 3), Guarded(rt, ctx, n * 4), Guarded(rt, ctx, STATS_BYTES)] for _ in range(3)]
    try:
        for budget in (0, n // 4):
            values = (w, h, THRESHOLD, 2.0 ** -6, 1, budget, 0, 0)
            for o in outs:
                for b in o:
                    b.reset()
            assert _call(rt, ctx, values, moments, *outs[0], scratch) == 0
            assert _call(rt, ctx, values, moments, *outs[1], scratch) == 0
            assert _call(rt, ctx, values, moments, outs[2][0], None, None, scratch) == 0          # no outError, no outStats
            ctx.synchronize()
            first = [b.read(np.uint8, (b.nbytes,)) for b in outs[0]]
            again = [b.read(np.uint8, (b.nbytes,)) for b in outs[1]]
            assert all(np.array_equal(x, y) for x, y in zip(first, again)), "two calls, identical bits"
            assert 0 < first[0].sum() < n
            assert np.array_equal(outs[2][0].read(np.uint8, (n,)), first[0]), "the mask without the optional outputs"
            assert outs[2][1].untouched() and outs[2][2].untouched()
    finally:
        for b in [moments, scratch] + [b for o in outs for b in o]:
            b.free()


def test_refusals_enqueue_nothing(rt, gpu_context):
    """Every refusal returns RTOW_ERROR_INVALID_VALUE and leaves the guard pattern in the outputs and in the scratch as it was."""
    ctx = gpu_context
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    w, h = 16, 8
    n = w * h
    moments = Guarded(rt, ctx, n * 12, 0, nm.make_moments(w, h, 3))
    mask, error, stats, scratch = Guarded(rt, ctx, n + 16), Guarded(rt, ctx, n * 4 + 16), Guarded(rt, ctx, STATS_BYTES + 16), Guarded(rt, ctx, STATS_BYTES + 16)
    everything = [moments, mask, error, stats, scratch]
    try:
        def call(values=(w, h, 0.01, 0.015625, 1, 16, 2, 0), **over):
            ptr = {"params": True, "moments": moments.ptr, "mask": mask.ptr, "error": error.ptr, "stats": stats.ptr, "scratch": scratch.ptr}
            ptr.update(over)
            p = a.NoiseMaskParams(*values)
            return rt.lib.load().rtowNoiseMaskDevice(ctx.handle, C.byref(p) if ptr["params"] else None, ptr["moments"], ptr["mask"], ptr["error"], ptr["stats"],
                                                     ptr["scratch"], None)

        for name in ("params", "moments", "mask", "scratch"):
            assert call(**{name: None}) == bad, name
        good = [w, h, 0.01, 0.015625, 1, 16, 2, 0]
        for index, value in ((0, 0), (0, -1), (1, 0), (1, -7), (2, 0.0), (2, -0.01), (2, float("nan")), (2, float("inf")), (3, -0.5), (3, float("nan")),
                             (3, float("inf")), (4, -1), (4, 4), (5, -1), (6, 4), (6, 7), (6, -1), (7, 1)):
            p = list(good)
            p[index] = value
            assert call(tuple(p)) == bad, (index, value)
        assert call((65536, 32768, 0.01, 0.015625, 1, 16, 2, 0)) == bad                # width * height > INT32_MAX
        for name in ("mask", "error", "stats", "scratch"):                             # an output, or the scratch, over the moments
            assert call(**{name: moments.ptr + 12 * (n - 1) + 8}) == bad, (name, "over the moments")
        assert call(error=mask.ptr + n - 1) == bad and call(mask=error.ptr + 4 * n - 1) == bad      # outputs over each other, by one byte
        assert call(stats=mask.ptr + 4) == bad and call(stats=error.ptr + 8) == bad
        assert call(scratch=mask.ptr) == bad and call(scratch=error.ptr + 4) == bad and call(scratch=stats.ptr + 284) == bad and call(stats=scratch.ptr) == bad
        ctx.synchronize()
        for b in everything:
            assert b.untouched()
        # and the calls these were variations of are accepted
        assert call() == a.RTOW_SUCCESS and call(error=None, stats=None) == a.RTOW_SUCCESS and call(tuple(good[:5]) + (0, 3, 0)) == a.RTOW_SUCCESS
        ctx.synchronize()
        assert not mask.untouched() and not stats.untouched()
    finally:
        for b in everything:
            b.free()


def test_the_list_builder_counts_what_the_mask_holds(rt, gpu_context):
    """rtowBuildPixelListDevice on the mask: words[0] == stats.masked, and the list is the mask's pixels"""
    ctx = gpu_context
    w, h = 96, 54
    n = w * h
    host = nm.make_moments(w, h, 11)
    moments, scratch = Guarded(rt, ctx, n * 12, 0, host), Guarded(rt, ctx, STATS_BYTES)
    mask, stats = Guarded(rt, ctx, n, 1), Guarded(rt, ctx, STATS_BYTES)
    lists = []
    try:
        for radius, budget in ((0, 0), (1, n // 4), (3, n // 8)):
            assert _call(rt, ctx, (w, h, THRESHOLD, 2.0 ** -6, radius, budget, 2, 0), moments, mask, None, stats, scratch) == 0
            lists = list(rt.build_pixel_list(ctx, w, h, n, mask=mask.ptr))
            ctx.synchronize()
            words = lists[0].download(np.uint32, (4 + n,))
            got = stats.read(np.uint32, (72,))
            byte = mask.read(np.uint8, (n,))
            assert words[0] == got[3] == byte.sum() and 0 < words[0] < n, (radius, budget, words[0], got[3])
            assert np.array_equal(np.sort(words[4: 4 + words[0]]), np.flatnonzero(byte))
            if budget:
                assert got[2] <= budget
            for b in lists:
                b.free()
            lists = []
    finally:
        for b in [moments, scratch, mask, stats] + lists:
            b.free()


def test_the_call_replays_from_a_captured_graph_as_a_linear_chain(rt, gpu_context):
    """With a budget - the clear, the counting pass, the pick step and the masking pass - captured on a caller's stream: nothing runs while capturing, the graph is a
    chain (every node has at most one successor and one predecessor, one root), and its replay equals the call made directly, bit for bit."""
    ctx = gpu_context
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, C.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
    hip.hipGraphInstantiate.argtypes = [C.POINTER(vp), vp, vp, vp, C.c_size_t]
    hip.hipGraphLaunch.argtypes = [vp, vp]
    hip.hipStreamSynchronize.argtypes = [vp]
    hip.hipGraphGetNodes.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]
    for f in (hip.hipGraphExecDestroy, hip.hipGraphDestroy, hip.hipStreamDestroy):
        f.argtypes = [vp]
    w, h = 130, 9
    n = w * h
    host = nm.make_moments(w, h, 5)
    values = (w, h, THRESHOLD, 2.0 ** -6, 2, n // 4, 2, 0)
    moments, scratch = Guarded(rt, ctx, n * 12, 4, host), Guarded(rt, ctx, STATS_BYTES)
    outs = [Guarded(rt, ctx, n, 1), Guarded(rt, ctx, n * 4), Guarded(rt, ctx, STATS_BYTES)]
    side, graph, exe = vp(), vp(), vp()
    try:
        assert _call(rt, ctx, values, moments, *outs, scratch) == 0
        ctx.synchronize()
        direct = [b.read(np.uint8, (b.nbytes,)) for b in outs]
        want = nm.noise_mask(w, h, host, *values[2:7])
        assert np.array_equal(direct[0], want["mask"]) and 0 < want["qualifying"] <= n // 4
        for b in outs + [scratch]:
            b.reset()
        ctx.synchronize()
        assert hip.hipStreamCreate(C.byref(side)) == 0
        assert hip.hipStreamBeginCapture(side, 2) == 0                                 # hipStreamCaptureModeRelaxed
        try:
            rc = _call(rt, ctx, values, moments, *outs, scratch, stream=side)
        finally:
            assert hip.hipStreamEndCapture(side, C.byref(graph)) == 0
        assert rc == 0
        assert all(b.untouched() for b in outs), "capturing runs nothing"
        count = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0
        nodes = count.value
        assert hip.hipGraphGetEdges(graph, None, None, C.byref(count)) == 0
        src, dst = (vp * count.value)(), (vp * count.value)()
        assert hip.hipGraphGetEdges(graph, src, dst, C.byref(count)) == 0
        assert nodes == 4 and count.value == nodes - 1, (nodes, count.value)          # a clear and three launches
        assert len(set(src)) == len(set(dst)) == nodes - 1, "a chain: no node has two successors or two predecessors"
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert hip.hipGraphLaunch(exe, side) == 0
        assert hip.hipStreamSynchronize(side) == 0
        replayed = [b.read(np.uint8, (b.nbytes,)) for b in outs]
        for name, x, y in zip(("mask", "outError", "outStats"), direct, replayed):
            assert np.array_equal(x, y), name
    finally:
        if side:
            hip.hipStreamSynchronize(side)
        if exe:
            hip.hipGraphExecDestroy(exe)
        if graph:
            hip.hipGraphDestroy(graph)
        if side:
            hip.hipStreamDestroy(side)
        for b in [moments, scratch] + outs:
            b.free()


# ---------------------------------------------------------------- on the cover scene

KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))


def _group(rt, ctx, plist, w, h):
    """independent batches from zeroed inputs (rtowSampleBatchGroupDevice) -> the per-batch host arrays [[color, normal, albedo, scw], ...]"""
    n = w * h
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


def _fold(batches, acc=None):
    acc = [np.zeros_like(x) for x in batches[0]] if acc is None else acc
    for b in batches:
        acc = [s + x for s, x in zip(acc, b)]                              # rtowAddAccumDevice: dst += src, in batch order
    return acc


def luminance_of(color):
    with np.errstate(all="ignore"):
        return dv.lum(color[:, :3].astype(np.float64) / np.maximum(color[:, 3:4].astype(np.float64), 1e-30))


class AdaptiveFrame:
    """The cover scene at w x h.  A first group of `first` batches of `spp` samples (seeds seed + 1 ...) with its moments; refine(rounds, batches, **settings) runs
    rounds of rt.refine_noisy_pixels with `batches` list batches of `spp` samples each on a copy of that frame; uniform(samples) is the first group with as many more
    full-frame batches of `spp` samples as it takes to reach at least `samples` samples in all - rounded UP to whole batches, so a comparison never favours refinement.
    (profiles/noise_mask_timing.py runs its parameter grid on this frame.)"""

    def __init__(self, rt, ctx, w, h, seed=0, first=8, spp=2, most=16):
        self.rt, self.ctx, self.w, self.h, self.n, self.spp, self.seed = rt, ctx, w, h, w * h, spp, seed
        self.scene = rt.scenes.cover_scene()
        ctx.upload_scene(self.scene.desc())
        self.first = _group(rt, ctx, [self.params(seed + 1 + k) for k in range(first)], w, h)
        self.moments = dv.accumulate_moments([b[0] for b in self.first])
        self.acc = _fold(self.first)
        self.extra_seed = seed + 101
        self.extra = None
        self.most = most

    def params(self, seed, spp=None):
        return self.rt.scenes.make_params(self.scene, self.w, self.h, spp=self.spp if spp is None else spp, trace_depth=8, seed=seed)

    def full_frame_batches(self, count):
        """the batches refine() gives its lists, rendered for every pixel"""
        if self.extra is None or len(self.extra) < count:
            self.extra = _group(self.rt, self.ctx, [self.params(self.extra_seed + k) for k in range(max(count, self.most))], self.w, self.h)
        return self.extra[:count]

    def refine(self, rounds, batches, **settings):
        """-> (accumulators, moments, [(abi.NoiseStats, listed) per round])"""
        rt, ctx, n = self.rt, self.ctx, self.n
        acc = [rt.DeviceBuffer(ctx).upload(x) for x in self.acc]
        mom = rt.DeviceBuffer(ctx).upload(self.moments)
        try:
            log = []
            for r in range(rounds):
                plist = [self.params(self.extra_seed + r * batches + k) for k in range(batches)]
                log.append(rt.refine_noisy_pixels(ctx, self.w, self.h, plist, mom, acc, **settings))
            return [b.download(F, (n, k)) for b, (_, k) in zip(acc, KEYS)], mom.download(F, (n, 3)), log
        finally:
            for b in acc + [mom]:
                b.free()

    def uniform(self, samples):
        """-> (accumulators, samples in all)"""
        total = lambda acc: float(acc[0][:, 3].astype(np.float64).sum())
        acc, count = self.acc, 0
        while total(acc) < samples:                                        # a batch may deliver fewer than n * spp samples: count what arrived
            count += 1
            acc = _fold(self.full_frame_batches(count)[count - 1:], acc)
        return acc, total(acc)

    def reference(self, spp=1024):
        ref = self.rt.sample_batch_host(self.ctx, self.params(self.seed + 9, spp), want_diag=False)
        return luminance_of(ref["color"])


def error_ratios(adaptive, uniform, reference, floor=2.0 ** -6):
    """(squared error, relative squared error err^2 / (ref^2 + floor^2)) of the luminance of `adaptive` over those of `uniform`"""
    def both(acc):
        err = (luminance_of(acc[0]) - reference) ** 2
        return float(err.mean()), float((err / (reference ** 2 + floor ** 2)).mean())
    (a_abs, a_rel), (u_abs, u_rel) = both(adaptive), both(uniform)
    return a_abs / u_abs, a_rel / u_rel


def test_one_refinement_round_on_the_cover_scene(rt, gpu_context):
    """96 x 54: 8 x 2 spp as a group with moments, then one refine_noisy_pixels round with 4 list batches and a budget of n / 4.  The statistics are the restatement's
    on those moments; every pixel the mask leaves out keeps its 11 accumulator floats and its moments bit for bit; every listed pixel holds exactly the first frame plus
    the four batches as full-frame launches render them - so its color.w and its n grew by what its own batches delivered; qualifying <= n / 4."""
    ctx = gpu_context
    a = rt.abi
    w, h = 96, 54
    n = w * h
    frame = AdaptiveFrame(rt, ctx, w, h, most=4)
    settings = dict(ErrorThreshold=0.01, LuminanceFloor=2.0 ** -6, Dilate=1, MaxQualifying=n // 4, Flags=a.NOISE_MASK_UNKNOWN_QUALIFIES)
    acc, mom, log = frame.refine(1, 4, **settings)
    stats, listed = log[0]
    want = nm.noise_mask(w, h, frame.moments, settings["ErrorThreshold"], settings["LuminanceFloor"], 1, n // 4, settings["Flags"])
    _same_bits(np.frombuffer(bytes(stats), np.uint32), want["words"], "stats")
    assert stats.qualifying <= n // 4 and stats.known + stats.unknown == n
    assert listed == stats.masked == want["masked"] and 0 < listed < n
    out = want["mask"] == 0
    for (name, _), before, after in zip(KEYS, frame.acc, acc):
        _same_bits(after[out], before[out], ("unlisted", name))
    _same_bits(mom[out], frame.moments[out], ("unlisted", "moments"))
    batches = frame.full_frame_batches(4)
    inside = ~out
    for (name, _), expect, after in zip(KEYS, _fold(batches, frame.acc), acc):
        _same_bits(after[inside], expect[inside], ("listed", name))
    _same_bits(mom[inside], dv.accumulate_moments([b[0] for b in batches], frame.moments)[inside], ("listed", "moments"))
    delivered = sum(b[0][:, 3] for b in batches)
    assert (delivered[inside] > 0).all()
    assert np.array_equal((acc[0][:, 3] - frame.acc[0][:, 3])[inside], delivered[inside])          # whole numbers: the float sums are exact
    counted = sum(((b[0][:, 3] > 0) & np.isfinite(luminance_of(b[0]))).astype(F) for b in batches)
    assert np.array_equal((mom[:, 2] - frame.moments[:, 2])[inside], counted[inside]) and (counted[inside] >= 1).all()


def test_what_refinement_is_worth_on_the_cover_scene(rt, gpu_context):
    """192 x 108 against 1024 spp, the recommended settings: 8 x 2 spp, then 4 rounds of 4 list batches, against a uniform frame with at least as many samples in all.
    profiles/r14_noise_mask.json records the two error ratios of this protocol on three seeds: squared error 0.854 / 0.764 / 0.843, relative squared error 0.752 /
    0.686 / 0.767 - below 0.95 on every seed, so this test (seed 0) asserts that refinement beats the uniform frame on both, after asserting what holds whatever the
    ratios are: the uniform frame is not short of samples, and both ratios are finite."""
    ctx = gpu_context
    a = rt.abi
    w, h = 192, 108
    n = w * h
    frame = AdaptiveFrame(rt, ctx, w, h)
    acc, _, log = frame.refine(4, 4, ErrorThreshold=a.NOISE_MASK_DEFAULT_ERROR_THRESHOLD, LuminanceFloor=a.NOISE_MASK_DEFAULT_LUMINANCE_FLOOR,
                               Dilate=a.NOISE_MASK_DEFAULT_DILATE, MaxQualifying=n // a.NOISE_MASK_DEFAULT_BUDGET_DIVISOR, Flags=a.NOISE_MASK_DEFAULT_FLAGS)
    spent = float(acc[0][:, 3].astype(np.float64).sum())
    uniform, uniform_spent = frame.uniform(spent)
    assert uniform_spent >= spent > float(frame.acc[0][:, 3].astype(np.float64).sum())
    assert uniform_spent - spent < n * frame.spp, "rounded up to whole batches, no further"
    for stats, listed in log:
        assert stats.qualifying <= n // a.NOISE_MASK_DEFAULT_BUDGET_DIVISOR and listed == stats.masked
    ratios = error_ratios(acc, uniform, frame.reference())
    print("refined / uniform: squared error %.4f, relative squared error %.4f (samples %.0f / %.0f)" % (ratios + (spent, uniform_spent)))
    assert all(np.isfinite(r) and r > 0 for r in ratios), ratios
    assert all(r < 1 for r in ratios), ratios
