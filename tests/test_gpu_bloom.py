"""GPU tests of rtowBloomDevice (include/rtow.h): the pass bit for bit against the numpy restatement of its specification (tests/bloom_reference.py) on seeded frames
that need no scene - the output and the pyramid the scratch is left with, at the sizes where a ceil, a clamp, a collapsed 1 x 1 mip or a tile seam can go wrong, for
1, 2 and 8 levels, with and without the Karis average, every knee and threshold, and the state NULL, zero-filled and valid - then the in-place form, determinism,
refusals, and bloom, meter and finalize replayed from one captured graph.  Every allocation carries guard words, at byte offsets 0 and 4; the scratch is exactly
RTOW_BLOOM_SCRATCH_BYTES.  All in the session context."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_reference as bl  # noqa: E402
import tonemap_reference as tm  # noqa: E402
from test_gpu_reproject import GUARD, Dev  # noqa: E402  (guarded device arrays)

pytestmark = pytest.mark.gpu

F = np.float32
# 257 x 17: one texel more than two staged tiles (a 64 x 4 tile of mip 1 stages 128 x 8 pixels of the frame) in both dimensions
SIZES = [(1, 1), (2, 1), (5, 3), (67, 5), (257, 3), (96, 54), (257, 17)]
LEVELS = (1, 2, 8)
SCATTER, INTENSITY = 0.7, 0.75
LIT = dict(tm.zero_state(), valid=1, exposure=F(0.37), stops=F(-1.4))
# (karis, knee, threshold, state, params.exposure): every value of every factor, the Karis flag with every knee and every state
CONFIGS = [(1, 0.5, 1.0, "lit", 1.25), (0, 0.0, 1.0, None, 1.0), (1, 1.0, 1.0, "zero", 2.0), (0, 0.5, 0.0, "lit", 1.0), (1, 0.0, 0.0, None, 0.5), (0, 1.0, 1.0, "lit", 3.0)]
AT_OFFSET_4 = (0, 1, 4)                                                    # the configurations that also run 4 bytes into every allocation
STATES = {None: None, "zero": tm.zero_state(), "lit": LIT}

_REFERENCES = {}


def _frame(w, h):
    return tm.make_frame(w * h, 1000 * w + h)


def reference(w, h, levels, config, scatter=SCATTER, intensity=INTENSITY):
    """the restatement's result for one call, computed once"""
    key = (w, h, levels, config, scatter, intensity)
    if key not in _REFERENCES:
        karis, knee, threshold, state, exposure = config
        s = tm.scale_of(exposure, STATES[state])
        _REFERENCES[key] = bl.bloom(_frame(w, h), w, h, levels, threshold, knee, scatter, intensity, s=s, karis=bool(karis))
    return _REFERENCES[key]


class Bloom:
    """the buffers of one call: the frame, the scratch of exactly the macro's bytes, the output and the two state records, all guarded"""

    def __init__(self, rt, ctx, w, h, offset=0, frame=None):
        self.rt, self.ctx, self.w, self.h, self.n = rt, ctx, w, h, w * h
        frame = _frame(w, h) if frame is None else frame
        self.color = Dev(rt, ctx, frame.nbytes, offset, frame)
        self.scratch_bytes = rt.abi.bloom_scratch_bytes(w, h)
        self.scratch = Dev(rt, ctx, self.scratch_bytes, offset)
        self.out = Dev(rt, ctx, self.n * 12, offset)
        self.states = {"zero": Dev(rt, ctx, 1056, offset, tm.record(tm.zero_state())), "lit": Dev(rt, ctx, 1056, offset, tm.record(LIT))}
        self.all = [self.color, self.scratch, self.out] + list(self.states.values())

    def call(self, levels=6, threshold=1.0, knee=0.5, scatter=SCATTER, intensity=INTENSITY, exposure=1.0, flags=1, reserved=0, state=None, width=None, height=None,
             stream=None, **ptr):
        p = self.rt.abi.BloomParams(self.w if width is None else width, self.h if height is None else height, levels, float(threshold), float(knee), float(scatter),
                                    float(intensity), float(exposure), flags, reserved)
        at = {"state": self.states[state].ptr if state else None, "color": self.color.ptr, "scratch": self.scratch.ptr, "out": self.out.ptr}
        at.update(ptr)
        return self.rt.lib.load().rtowBloomDevice(self.ctx.handle, C.byref(p), at["state"], at["color"], at["scratch"], at["out"], stream)

    def run(self, levels, config, **kw):
        karis, knee, threshold, state, exposure = config
        return self.call(levels, threshold, knee, exposure=exposure, flags=karis, state=state, **kw)

    def reset(self):
        for b in (self.scratch, self.out):
            b.buf.upload(np.full(b.front // 4 + b.nbytes // 4 + 4, GUARD, np.uint32))

    def collect(self, out=None):
        """the words of the output and of the scratch, after the guards of every buffer have been checked"""
        self.ctx.synchronize()
        for b in self.all:
            assert b.guards_intact()
        return (out or self.out).download(np.uint32, (self.n * 3,)), self.scratch.download(np.uint32, (self.scratch_bytes // 4,))

    def untouched(self):
        self.ctx.synchronize()
        return (self.out.words() == GUARD).all() and (self.scratch.words() == GUARD).all()

    def free(self):
        for b in self.all:
            b.free()


def _same(got, want, what):
    out, scratch = got
    words = want["out"].view(np.uint32).ravel()
    bad = np.flatnonzero(out != words)
    assert np.array_equal(out, words), (what, "out", bad.size, bad[:6] // 3, out[bad[:6]].view(F), words[bad[:6]].view(F))
    pyramid = bl.scratch_words(want["mips"])
    bad = np.flatnonzero(scratch[:pyramid.size] != pyramid)
    assert np.array_equal(scratch[:pyramid.size], pyramid), (what, "pyramid", bad.size, bad[:6] // 4, scratch[bad[:6]].view(F), pyramid[bad[:6]].view(F))
    assert (scratch[pyramid.size:] == GUARD).all(), (what, "the scratch behind the pyramid is not written")


@pytest.mark.parametrize("w,h", SIZES)
def test_the_pass_is_bit_exact(rt, gpu_context, w, h):
    # from the restatement alone: the frames of 64 pixels and more carry pixels that pass through, and something blooms
    if w * h >= 64:
        want = reference(w, h, 8, CONFIGS[0])
        assert (~np.isfinite(_frame(w, h)).all(axis=1)).any() and want["layer"].any() and np.isfinite(want["layer"]).all()
    if (w, h) == (257, 17):
        assert [m.shape[:2] for m in want["mips"]][:3] == [(9, 129), (5, 65), (3, 33)]      # mip 1: three tiles across and three down, the last of one texel
    for offset in (0, 4):
        b = Bloom(rt, gpu_context, w, h, offset)
        try:
            for levels in LEVELS:
                for k, config in enumerate(CONFIGS):
                    if offset and k not in AT_OFFSET_4:
                        continue
                    b.reset()
                    assert b.run(levels, config) == rt.abi.RTOW_SUCCESS
                    _same(b.collect(), reference(w, h, levels, config), (w, h, offset, levels, config))
        finally:
            b.free()


@pytest.mark.parametrize("w,h", [(67, 5), (96, 54)])
def test_the_in_place_call_equals_the_out_of_place_one(rt, gpu_context, w, h):
    a, b = Bloom(rt, gpu_context, w, h), Bloom(rt, gpu_context, w, h, offset=4)
    try:
        for config in CONFIGS[:2]:
            a.reset()
            a.color.buf.upload(np.concatenate([np.full(a.color.front // 4, GUARD, np.uint32), _frame(w, h).view(np.uint32).ravel(), np.full(4, GUARD, np.uint32)]))
            b.reset()
            assert a.run(8, config, out=a.color.ptr) == rt.abi.RTOW_SUCCESS and b.run(8, config) == rt.abi.RTOW_SUCCESS
            in_place, apart = a.collect(out=a.color), b.collect()
            assert np.array_equal(in_place[0], apart[0]) and np.array_equal(in_place[1], apart[1])
            _same(in_place, reference(w, h, 8, config), (w, h, "in place", config))
            assert (a.out.words() == GUARD).all()
    finally:
        a.free()
        b.free()


def test_two_calls_give_identical_bits(rt, gpu_context):
    w, h = 257, 17
    results = []
    for _ in range(2):
        b = Bloom(rt, gpu_context, w, h)
        try:
            assert b.run(8, CONFIGS[0]) == rt.abi.RTOW_SUCCESS
            results.append(np.concatenate(b.collect()))
        finally:
            b.free()
    assert np.array_equal(results[0], results[1])


def test_refusals_enqueue_nothing(rt, gpu_context):
    a = rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    w, h = 67, 5
    n = w * h
    nan, inf = float("nan"), float("inf")
    b = Bloom(rt, gpu_context, w, h)
    try:
        sb = b.scratch_bytes
        for kw in (dict(color=None), dict(scratch=None), dict(out=None), dict(levels=0), dict(levels=9), dict(levels=-1), dict(threshold=-0.5), dict(threshold=nan),
                   dict(threshold=inf), dict(knee=-0.25), dict(knee=1.25), dict(knee=nan), dict(scatter=-0.25), dict(scatter=1.25), dict(scatter=nan), dict(intensity=-1.0),
                   dict(intensity=nan), dict(intensity=inf), dict(exposure=-1.0), dict(exposure=65537.0), dict(exposure=nan), dict(exposure=inf), dict(flags=2), dict(flags=3),
                   dict(flags=-1), dict(reserved=1), dict(width=0), dict(height=0), dict(width=-1), dict(width=65536, height=65536),
                   dict(out=b.color.ptr + 4), dict(out=b.color.ptr + n * 12 - 4), dict(out=b.scratch.ptr + sb - 4), dict(scratch=b.out.ptr + n * 12 - 4),
                   dict(scratch=b.color.ptr + n * 12 - 4), dict(scratch=b.color.ptr, out=b.color.ptr), dict(state="lit", out=b.states["lit"].ptr + 1052),
                   dict(state="lit", scratch=b.states["lit"].ptr - sb + 4)):
            assert b.call(**kw) == bad, kw
        p = a.BloomParams(w, h, 6, 1.0, 0.5, 0.7, 0.05, 1.0, 1, 0)
        lib = rt.lib.load()
        assert lib.rtowBloomDevice(None, C.byref(p), None, b.color.ptr, b.scratch.ptr, b.out.ptr, None) == bad
        assert lib.rtowBloomDevice(gpu_context.handle, None, None, b.color.ptr, b.scratch.ptr, b.out.ptr, None) == bad
        assert b.untouched()
        assert np.array_equal(b.color.download(np.uint32, (n * 3,)), _frame(w, h).view(np.uint32).ravel()) and all(x.guards_intact() for x in b.all)
    finally:
        b.free()


def test_bloom_meter_and_finalize_replay_from_one_captured_graph(rt, gpu_context, oracle):
    """The 2 * levels launches of bloom, the meter's two and the finalize captured on a caller's stream (a linear capture: no call allocates or waits) and replayed
    once.  Bloom runs in front of the meter, so it sees the zero-filled state - scale 1 - and the finalize sees what the meter made of the bloomed frame."""
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
    w, h, levels = 67, 5, 3
    n = w * h
    config = (1, 0.5, 1.0, "zero", 1.0)
    bloomed = reference(w, h, levels, config)
    state = tm.meter(bloomed["out"], tm.zero_state())
    want = tm.finalize(oracle, bloomed["out"], None, None, tm.ACES_FILM, 1.0, state)[0]
    b = Bloom(rt, ctx, w, h)                                                # every allocation and upload before the capture
    meter_scratch, texture = Dev(rt, ctx, rt.abi.exposure_scratch_bytes()), Dev(rt, ctx, n * 4)
    side, graph, exe = vp(), vp(), vp()
    lib = rt.lib.load()
    try:
        ctx.synchronize()
        assert hip.hipStreamCreate(C.byref(side)) == 0
        assert hip.hipStreamBeginCapture(side, 2) == 0                     # hipStreamCaptureModeRelaxed
        try:
            assert b.run(levels, config, stream=side) == rt.abi.RTOW_SUCCESS
            ep = rt.abi.ExposureParams(w, h, 500, 950, float(tm.LOG2_GREY), -8.0, 8.0, 1.0, 0, 0)
            assert lib.rtowMeterExposureDevice(ctx.handle, C.byref(ep), b.out.ptr, meter_scratch.ptr, b.states["zero"].ptr, side) == rt.abi.RTOW_SUCCESS
            tp = rt.abi.ToneMapParams(n, tm.ACES_FILM, 1.0, 0, (C.c_int32 * 2)(0, 0))
            assert lib.rtowFinalizeToneMappedDevice(ctx.handle, C.byref(tp), b.states["zero"].ptr, b.out.ptr, None, None, texture.ptr, None, None, side) == rt.abi.RTOW_SUCCESS
        finally:
            assert hip.hipStreamEndCapture(side, C.byref(graph)) == 0
        assert b.untouched() and (texture.words() == GUARD).all(), "capturing runs nothing"
        assert hip.hipGraphInstantiate(C.byref(exe), graph, None, None, 0) == 0
        assert hip.hipGraphLaunch(exe, side) == 0
        assert hip.hipStreamSynchronize(side) == 0
        _same(b.collect(), bloomed, "replayed")
        assert np.array_equal(b.states["zero"].download(np.uint32, (tm.RECORD_WORDS,)), tm.record(state)), "the record the meter left"
        assert texture.guards_intact() and meter_scratch.guards_intact() and np.array_equal(texture.download(np.uint8, (n, 4)), want)
    finally:
        if side:
            hip.hipStreamSynchronize(side)
        if exe:
            hip.hipGraphExecDestroy(exe)
        if graph:
            hip.hipGraphDestroy(graph)
        if side:
            hip.hipStreamDestroy(side)
        b.free()
        meter_scratch.free()
        texture.free()
