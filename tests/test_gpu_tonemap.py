"""GPU tests of rtowMeterExposureDevice and rtowFinalizeToneMappedDevice (include/rtow.h): both passes bit for bit against the numpy restatement of their specification
(tests/tonemap_reference.py) on seeded frames that need no scene - the whole 1056-byte record of the meter at every size, rank range, rate and stop limit, the three
curves with and without the guide pairs and the state, CLAMP against rtowFinalizeDevice on the same device buffers, the meter feeding the finalize on one stream with no
host wait in between - and refusals, determinism and both calls replayed from one captured graph.  Every allocation carries guard words; all in the session context."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tonemap_reference as tm  # noqa: E402
from test_gpu_reproject import GUARD, Dev  # noqa: E402  (guarded device arrays)

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (67, 5), (257, 3), (96, 54)]
PERMILLES = [(0, 1000), (500, 950), (300, 300), (1000, 1000)]
COUNTS = [1, 255, 257, 5184]
SCRATCH_BYTES = 256 * 256 * 4


def _frame(w, h):
    return tm.make_frame(w * h, 1000 * w + h)


@pytest.fixture(scope="module")
def finalized(oracle):
    """the reference bytes of each (curve, count, exposure, state scale), computed once"""
    cache = {}

    def get(n, curve, exposure, state=None):
        key = (n, curve, float(exposure), None if state is None else (int(state["valid"]), float(state["exposure"])))
        if key not in cache:
            normal, albedo = tm.make_guides(n, n)
            cache[key] = tm.finalize(oracle, tm.make_frame(n, n), normal, albedo, curve, exposure, state)
        return cache[key]
    return get


class Meter:
    """one frame on the device with the scratch and a state record, all guarded; `offset` bytes into every allocation"""

    def __init__(self, rt, ctx, frame, state=None, offset=0):
        self.rt, self.ctx, self.n = rt, ctx, frame.shape[0]
        self.color = Dev(rt, ctx, frame.nbytes, offset, frame)
        self.scratch = Dev(rt, ctx, SCRATCH_BYTES, offset)
        self.state = Dev(rt, ctx, 1056, offset, tm.record(state if state is not None else tm.zero_state()))

    def call(self, w, h, low=500, high=950, compensation=tm.LOG2_GREY, min_stops=-8, max_stops=8, rate=1, flags=0, reserved=0, stream=None, **ptr):
        p = self.rt.abi.ExposureParams(w, h, low, high, float(compensation), float(min_stops), float(max_stops), float(rate), flags, reserved)
        at = {"color": self.color.ptr, "scratch": self.scratch.ptr, "state": self.state.ptr}
        at.update(ptr)
        return self.rt.lib.load().rtowMeterExposureDevice(self.ctx.handle, C.byref(p), at["color"], at["scratch"], at["state"], stream)

    def record(self):
        self.ctx.synchronize()
        assert self.color.guards_intact() and self.scratch.guards_intact() and self.state.guards_intact()
        return self.state.download(np.uint32, (tm.RECORD_WORDS,))

    def free(self):
        for b in (self.color, self.scratch, self.state):
            b.free()


def _same_record(got, want, what):
    want = tm.record(want)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], got[:8].view(F)[:4], want[:8].view(F)[:4])


@pytest.mark.parametrize("w,h", SIZES)
def test_the_meter_is_bit_exact_at_every_rank_range(rt, gpu_context, w, h):
    frame = _frame(w, h)
    fresh = tm.meter(frame, tm.zero_state())
    # from the reference alone: the frame visits the bins, the ignored stretch and the top bin (make_frame walks 320 luminance steps: a smaller frame cannot)
    if w * h >= 320:
        assert np.count_nonzero(fresh["histogram"]) >= 200 and fresh["ignored"] > 0 and fresh["histogram"][255] > 0
    for offset in (0, 4):
        m = Meter(rt, gpu_context, frame, offset=offset)
        try:
            state = tm.zero_state()
            for low, high in PERMILLES:                                    # one state through the four calls, as a host would keep it
                kw = dict(low=low, high=high, rate=0.5, min_stops=-32, max_stops=32)
                assert m.call(w, h, **kw) == rt.abi.RTOW_SUCCESS
                state = tm.meter(frame, state, **kw)
                _same_record(m.record(), state, (w, h, offset, low, high))
        finally:
            m.free()


def test_the_meter_beyond_its_256_workgroups(rt, gpu_context):
    """1031 x 257 = 264 967 pixels: more groups of four than 256 workgroups of 256 lanes take in one step, so the grid is capped, part of the lanes go round their loop
    a second time, and three pixels are left behind the last group"""
    w, h = 1031, 257
    assert (w * h) // 4 > 256 * 256 and (w * h) % 4 == 3
    frame = _frame(w, h)
    m = Meter(rt, gpu_context, frame, offset=4)
    try:
        assert m.call(w, h) == rt.abi.RTOW_SUCCESS
        _same_record(m.record(), tm.meter(frame, tm.zero_state()), (w, h))
    finally:
        m.free()


def test_a_constant_frame_and_a_frame_with_nothing_metered(rt, gpu_context):
    w, h = 67, 5
    constant = np.tile(np.array([[0.3, 0.6, 0.9]], F), (w * h, 1))
    want = tm.meter(constant, tm.zero_state())
    assert np.count_nonzero(want["histogram"]) == 1 and want["metered"] == w * h
    rng = np.random.default_rng(4)
    nothing = np.array([[0, 0, 0], [np.nan, 1, 1], [-1, -2, -3], [np.inf, 1, 1], [1e-6, 1e-6, 1e-6], [-0.0, -0.0, -0.0], [1e-40, 0, 0]], F)[rng.integers(0, 7, w * h)]
    for frame, state in ((constant, None), (nothing, None), (nothing, want)):
        m = Meter(rt, gpu_context, frame, state)
        try:
            assert m.call(w, h) == rt.abi.RTOW_SUCCESS
            after = tm.meter(frame, state if state is not None else tm.zero_state())
            _same_record(m.record(), after, "constant" if frame is constant else "nothing metered")
        finally:
            m.free()
    kept = tm.meter(nothing, want)
    assert kept["valid"] == 1 and kept["stops"] == want["stops"] and kept["metered"] == 0 and kept["ignored"] == w * h      # a valid state keeps its stops


def test_rates_and_stop_limits_on_one_state(rt, gpu_context):
    w, h = 96, 54
    frame = _frame(w, h)
    with np.errstate(over="ignore"):
        dim, bright = (frame * F(2.0 ** -6)).astype(F), (frame * F(2.0 ** 5)).astype(F)
    wide = dict(min_stops=-32, max_stops=32)
    steps = [(frame, dict(rate=0.0, **wide)), (dim, dict(rate=0.25, **wide)), (bright, dict(rate=1.0, **wide)),      # no history yet: the first call lands at once
             (dim, dict(rate=0.0, **wide)), (dim, dict(rate=0.25, **wide)), (dim, dict(rate=1.0, **wide)),           # three calls in a row on a valid state
             (bright, dict(rate=0.5, compensation=30.0, min_stops=-1, max_stops=1.5)),                     # a target beyond the upper limit
             (bright, dict(rate=0.5, compensation=-30.0, min_stops=-2.5, max_stops=1)),                    # and beyond the lower one
             (frame, dict(rate=0.75, low=0, high=1000, min_stops=-32, max_stops=32))]
    state = tm.zero_state()
    devices = {id(f): Meter(rt, gpu_context, f) for f in (frame, dim, bright)}
    try:
        for k, (f, kw) in enumerate(steps):
            m = devices[id(f)]
            m.state.buf.upload(np.concatenate([np.full(4, GUARD, np.uint32), tm.record(state), np.full(4, GUARD, np.uint32)]))      # the state so far, in this frame's record
            assert m.call(w, h, **kw) == rt.abi.RTOW_SUCCESS
            before, state = state, tm.meter(f, state, **kw)
            _same_record(m.record(), state, ("step", k))
            if k == 3:
                assert state["stops"] == before["stops"] != state["targetStops"]
            if k == 4:
                assert before["stops"] < state["stops"] < state["targetStops"]
            if k == 5:
                assert state["stops"] == state["targetStops"]
            if k == 6:
                assert state["targetStops"] == F(1.5) and state["stops"] == F(-1)                # the step itself is cut to the limits, too
            if k == 7:
                assert state["targetStops"] == F(-2.5) and F(-2.5) < state["stops"] < before["stops"]
    finally:
        for m in devices.values():
            m.free()


class Tone:
    """the buffers of one finalize call: colour and guides in, three RGBA32 textures out, all guarded"""

    def __init__(self, rt, ctx, n, state=None):
        self.rt, self.ctx, self.n = rt, ctx, n
        normal, albedo = tm.make_guides(n, n)
        self.ins = [Dev(rt, ctx, a.nbytes, 0, a) for a in (tm.make_frame(n, n), normal, albedo)]
        self.outs = [Dev(rt, ctx, n * 4) for _ in range(3)]
        self.state = None if state is None else Dev(rt, ctx, 1056, 0, tm.record(state))

    def call(self, curve, exposure=1.0, normal=True, albedo=True, state=True, pixel_count=None, flags=0, reserved=(0, 0), stream=None, **ptr):
        p = self.rt.abi.ToneMapParams(self.n if pixel_count is None else pixel_count, curve, float(exposure), flags, (C.c_int32 * 2)(*reserved))
        at = {"state": self.state.ptr if (state and self.state is not None) else None, "c": self.ins[0].ptr, "n": self.ins[1].ptr if normal else None,
              "a": self.ins[2].ptr if albedo else None, "oc": self.outs[0].ptr, "on": self.outs[1].ptr if normal else None, "oa": self.outs[2].ptr if albedo else None}
        at.update(ptr)
        return self.rt.lib.load().rtowFinalizeToneMappedDevice(self.ctx.handle, C.byref(p), at["state"], at["c"], at["n"], at["a"], at["oc"], at["on"], at["oa"], stream)

    def collect(self):
        self.ctx.synchronize()
        for b in self.ins + self.outs + ([self.state] if self.state is not None else []):
            assert b.guards_intact()
        return [b.download(np.uint8, (self.n, 4)) for b in self.outs]

    def reset(self):
        for b in self.outs:
            b.buf.upload(np.full(4 + self.n + 4, GUARD, np.uint32))

    def untouched(self):
        self.ctx.synchronize()
        return all((b.words() == GUARD).all() for b in self.outs)

    def free(self):
        for b in self.ins + self.outs + ([self.state] if self.state is not None else []):
            b.free()


def _same_bytes(got, want, what):
    for name, g, w in zip(("color", "normal", "albedo"), got, want):
        if w is None:
            assert (g.view(np.uint32) == GUARD).all(), (what, name, "a NULL pair is not written")
            continue
        bad = np.flatnonzero((g != w).any(1))
        assert bad.size == 0, (what, name, bad.size, bad[:5], g[bad[:3]], w[bad[:3]])


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("curve", tm.CURVES)
def test_the_finalize_is_bit_exact(rt, gpu_context, finalized, curve, n):
    lit = dict(tm.zero_state(), valid=1, exposure=F(0.37), stops=F(-1.4))
    t, z = Tone(rt, gpu_context, n, lit), Tone(rt, gpu_context, n, tm.zero_state())
    try:
        for exposure, state, normal, albedo in ((1.0, False, True, True), (0.75, False, True, True), (2.5, True, True, True), (1.0, True, False, True),
                                                (3.0, False, True, False), (0.5, True, False, False)):
            t.reset()
            assert t.call(curve, exposure, normal=normal, albedo=albedo, state=state) == rt.abi.RTOW_SUCCESS
            oc, on, oa = finalized(n, curve, exposure, lit if state else None)
            _same_bytes(t.collect(), (oc, on if normal else None, oa if albedo else None), (curve, n, exposure, state, normal, albedo))
        assert z.call(curve, 0.75) == rt.abi.RTOW_SUCCESS                  # a zero-filled state acts as scale 1
        _same_bytes(z.collect(), finalized(n, curve, 0.75), (curve, n, "zero-filled state"))
    finally:
        t.free()
        z.free()


@pytest.mark.parametrize("n", COUNTS)
def test_clamp_with_exposure_one_is_finalize_device(rt, gpu_context, n):
    t = Tone(rt, gpu_context, n)
    plain = [Dev(rt, gpu_context, n * 4) for _ in range(3)]
    try:
        assert t.call(tm.CLAMP, 1.0) == rt.abi.RTOW_SUCCESS
        assert rt.lib.load().rtowFinalizeDevice(gpu_context.handle, n, t.ins[0].ptr, t.ins[1].ptr, t.ins[2].ptr, plain[0].ptr, plain[1].ptr, plain[2].ptr, None) == rt.abi.RTOW_SUCCESS
        got = t.collect()
        for g, b in zip(got, plain):
            assert b.guards_intact() and np.array_equal(g, b.download(np.uint8, (n, 4)))
    finally:
        t.free()
        for b in plain:
            b.free()


def test_the_meter_feeds_the_finalize_without_a_host_wait(rt, gpu_context, oracle):
    w, h = 96, 54
    n = w * h
    t = Tone(rt, gpu_context, n, tm.zero_state())
    frame = tm.make_frame(n, n)
    scratch = Dev(rt, gpu_context, SCRATCH_BYTES)
    try:
        p = rt.abi.ExposureParams(w, h, 500, 950, float(tm.LOG2_GREY), -8.0, 8.0, 1.0, 0, 0)
        assert rt.lib.load().rtowMeterExposureDevice(gpu_context.handle, C.byref(p), t.ins[0].ptr, scratch.ptr, t.state.ptr, None) == rt.abi.RTOW_SUCCESS
        assert t.call(tm.ACES_FITTED, 1.25) == rt.abi.RTOW_SUCCESS         # same stream, nothing in between
        state = tm.meter(frame, tm.zero_state())
        assert state["valid"] == 1 and state["exposure"] != F(1)
        normal, albedo = tm.make_guides(n, n)
        _same_bytes(t.collect(), tm.finalize(oracle, frame, normal, albedo, tm.ACES_FITTED, 1.25, state), "metered")
        _same_record(t.state.download(np.uint32, (tm.RECORD_WORDS,)), state, "the state the finalize read")
        assert scratch.guards_intact()
    finally:
        t.free()
        scratch.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    w, h = 257, 3
    frame = _frame(w, h)
    records, textures = [], []
    for _ in range(2):
        m, t = Meter(rt, gpu_context, frame), Tone(rt, gpu_context, w * h)
        try:
            assert m.call(w, h) == rt.abi.RTOW_SUCCESS and t.call(tm.ACES_FITTED, 1.5) == rt.abi.RTOW_SUCCESS
            records.append(m.record())
            textures.append(np.concatenate(t.collect()))
        finally:
            m.free()
            t.free()
    assert np.array_equal(records[0], records[1]) and np.array_equal(textures[0], textures[1])


def test_refusals_enqueue_nothing(rt, gpu_context):
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    w, h = 67, 5
    n = w * h
    nan, inf = float("nan"), float("inf")
    m = Meter(rt, gpu_context, _frame(w, h))
    t = Tone(rt, gpu_context, n, tm.zero_state())
    try:
        for kw in (dict(color=None), dict(scratch=None), dict(state=None), dict(low=-1), dict(low=951), dict(high=1001), dict(compensation=nan), dict(compensation=inf),
                   dict(min_stops=-32.5), dict(max_stops=32.5), dict(min_stops=2, max_stops=1), dict(min_stops=nan), dict(max_stops=nan), dict(rate=nan), dict(rate=-0.25),
                   dict(rate=1.25), dict(flags=1), dict(reserved=1), dict(scratch=m.color.ptr + 4), dict(state=m.color.ptr + n * 12 - 4),
                   dict(state=m.scratch.ptr + SCRATCH_BYTES - 4), dict(scratch=m.state.ptr - SCRATCH_BYTES + 4)):
            assert m.call(w, h, **kw) == bad, kw
        for dims in ((0, h), (w, 0), (-1, h), (65536, 65536)):
            assert m.call(*dims) == bad, dims
        p = a.ExposureParams(w, h, 500, 950, -2.5, -8.0, 8.0, 1.0, 0, 0)
        lib = rt.lib.load()
        assert lib.rtowMeterExposureDevice(None, C.byref(p), m.color.ptr, m.scratch.ptr, m.state.ptr, None) == bad
        assert lib.rtowMeterExposureDevice(gpu_context.handle, None, m.color.ptr, m.scratch.ptr, m.state.ptr, None) == bad
        gpu_context.synchronize()
        assert (m.scratch.words() == GUARD).all() and np.array_equal(m.state.download(np.uint32, (tm.RECORD_WORDS,)), tm.record(tm.zero_state())) and m.state.guards_intact()

        for kw in (dict(c=None), dict(oc=None), dict(n=None), dict(on=None), dict(a=None), dict(oa=None), dict(pixel_count=0), dict(pixel_count=-5), dict(curve=3), dict(curve=-1),
                   dict(exposure=-0.5), dict(exposure=nan), dict(exposure=inf), dict(flags=1), dict(reserved=(1, 0)), dict(reserved=(0, 1)),
                   dict(oc=t.ins[0].ptr + n * 12 - 4), dict(on=t.ins[2].ptr), dict(oa=t.state.ptr + 1052), dict(on=t.outs[0].ptr + n * 4 - 4), dict(oa=t.outs[1].ptr)):
            kw = dict(kw)
            curve = kw.pop("curve", tm.ACES_FILM)
            assert t.call(curve, **kw) == bad, kw
        p = a.ToneMapParams(n, 1, 1.0, 0, (C.c_int32 * 2)(0, 0))
        args = [t.state.ptr] + [b.ptr for b in t.ins] + [b.ptr for b in t.outs] + [None]
        assert lib.rtowFinalizeToneMappedDevice(None, C.byref(p), *args) == bad and lib.rtowFinalizeToneMappedDevice(gpu_context.handle, None, *args) == bad
        assert t.untouched()
    finally:
        m.free()
        t.free()


def test_both_calls_replay_from_one_captured_graph(rt, gpu_context, oracle):
    """The meter's two launches and the finalize captured on a caller's stream (a linear capture: neither call allocates or waits) and replayed once: the record and the
    three textures equal the direct calls' - the restatement's, bit for bit."""
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
    w, h = 257, 3
    n = w * h
    frame = tm.make_frame(n, n)
    normal, albedo = tm.make_guides(n, n)
    state = tm.meter(frame, tm.zero_state())
    want = tm.finalize(oracle, frame, normal, albedo, tm.ACES_FILM, 1.0, state)
    t = Tone(rt, ctx, n, tm.zero_state())                                   # every allocation and upload before the capture
    scratch = Dev(rt, ctx, SCRATCH_BYTES)
    side, graph, exe = vp(), vp(), vp()
    try:
        ctx.synchronize()
        assert hip.hipStreamCreate(C.byref(side)) == 0
        assert hip.hipStreamBeginCapture(side, 2) == 0                     # hipStreamCaptureModeRelaxed
        try:
            p = rt.abi.ExposureParams(w, h, 500, 950, float(tm.LOG2_GREY), -8.0, 8.0, 1.0, 0, 0)
            assert rt.lib.load().rtowMeterExposureDevice(ctx.handle, C.byref(p), t.ins[0].ptr, scratch.ptr, t.state.ptr, side) == rt.abi.RTOW_SUCCESS
            assert t.call(tm.ACES_FILM, 1.0, stream=side) == rt.abi.RTOW_SUCCESS
        finally:
            assert hip.hipStreamEndCapture(side, C.byref(graph)) == 0
        assert t.untouched() and (scratch.words() == GUARD).all(), "capturing runs nothing"
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert hip.hipGraphLaunch(exe, side) == 0
        assert hip.hipStreamSynchronize(side) == 0
        _same_bytes(t.collect(), want, "replayed")
        _same_record(t.state.download(np.uint32, (tm.RECORD_WORDS,)), state, "replayed")
        assert scratch.guards_intact()
    finally:
        if side:
            hip.hipStreamSynchronize(side)
        if exe:
            hip.hipGraphExecDestroy(exe)
        if graph:
            hip.hipGraphDestroy(graph)
        if side:
            hip.hipStreamDestroy(side)
        t.free()
        scratch.free()
