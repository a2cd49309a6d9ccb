"""GPU tests of the four post passes ported straight from the reference - rtowCombineDevice, rtowFinalizeDevice, rtowCombineFinalizeDevice and rtowReduceMetricsDevice /
rtowReduceMetricsDeviceAsync (include/rtow.h) - at their edges, bit for bit against the C++ oracle on the cases of tests/postpass_reference.py (which
tests/test_postpass_reference.py holds to the oracle and to their names on the CPU): frames of one pixel, one column and one row, look-arounds across a whole column, a
workgroup boundary and onto NaN pixels, fractional and negative sample counts, normals at the threshold of normalizesafe, albedos round the LDR clamp; the floats next to
each of the 255 byte steps in all nine channel positions; sums that wrap an int32, weights that are all NaN, a frame of one pixel and one beyond the reduction's grid, both
strides.  Every allocation carries guard words, checked after every call; refusals enqueue nothing.  No tolerances.  All in the session context."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postpass_reference as pp  # noqa: E402
from test_gpu_reproject import GUARD, Dev  # noqa: E402  (guarded device arrays)

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]                 # (debugMode, ldrAlbedo)
NAMES = ("color", "normal", "albedo")


class Frame:
    """The buffers of the three passes for one frame: accumulators in (the float4 colour stays 16-byte aligned, the float3 streams sit `offset` bytes into their
    allocations), three float3 and three RGBA32 outputs, all guarded."""

    def __init__(self, rt, ctx, color4, normal, albedo, offset=0):
        self.rt, self.ctx, self.n = rt, ctx, color4.shape[0]
        self.ins = [Dev(rt, ctx, color4.nbytes, 0, color4), Dev(rt, ctx, normal.nbytes, offset, normal), Dev(rt, ctx, albedo.nbytes, offset, albedo)]
        self.f3 = [Dev(rt, ctx, self.n * 12, offset) for _ in range(3)]
        self.u8 = [Dev(rt, ctx, self.n * 4, offset) for _ in range(3)]

    def everything(self):
        return self.ins + self.f3 + self.u8

    def reset(self):
        for b in self.f3 + self.u8:
            b.buf.upload(np.full((b.front + b.nbytes + 16) // 4, GUARD, U))

    def combine(self, w, h, debug=0, ldr=0, fused=False, **ptr):
        lib, p = self.rt.lib.load(), self.rt.abi.CombineParams(w, h, debug, ldr)
        outs = self.u8 if fused else self.f3
        at = {"c": self.ins[0].ptr, "n": self.ins[1].ptr, "a": self.ins[2].ptr, "oc": outs[0].ptr, "on": outs[1].ptr, "oa": outs[2].ptr, "params": C.byref(p), "ctx": self.ctx.handle}
        at.update(ptr)
        call = lib.rtowCombineFinalizeDevice if fused else lib.rtowCombineDevice
        return call(at["ctx"], at["params"], at["c"], at["n"], at["a"], at["oc"], at["on"], at["oa"], None)

    def finalize(self, count, from_f3=False, **ptr):
        src = self.f3 if from_f3 else self.ins
        at = {"c": src[0].ptr, "n": src[1].ptr, "a": src[2].ptr, "oc": self.u8[0].ptr, "on": self.u8[1].ptr, "oa": self.u8[2].ptr, "ctx": self.ctx.handle}
        at.update(ptr)
        return self.rt.lib.load().rtowFinalizeDevice(at["ctx"], count, at["c"], at["n"], at["a"], at["oc"], at["on"], at["oa"], None)

    def guards(self):
        self.ctx.synchronize()
        for b in self.everything():
            assert b.guards_intact()

    def floats(self):
        self.guards()
        return [b.download(F, (self.n, 3)) for b in self.f3]

    def bytes(self):
        self.guards()
        return [b.download(np.uint8, (self.n, 4)) for b in self.u8]

    def untouched(self):
        self.ctx.synchronize()
        return all((b.words() == GUARD).all() for b in self.f3 + self.u8)

    def free(self):
        for b in self.everything():
            b.free()


def _same_floats(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero((pp.bits(g).reshape(-1, 3) != pp.bits(w).reshape(-1, 3)).any(1))
        assert bad.size == 0, (what, name, bad.size, bad[:5], g[bad[:3]], w[bad[:3]], pp.bits(g[bad[:3]]), pp.bits(w[bad[:3]]))


def _same_bytes(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        bad = np.flatnonzero((g != w).any(1))
        assert bad.size == 0, (what, name, bad.size, bad[:5], g[bad[:3]], w[bad[:3]])


# ---------------------------------------------------------------- combine
@pytest.mark.parametrize("w,h", pp.COMBINE_SHAPES)
def test_combine_and_the_fused_pass_are_the_oracle(rt, oracle, gpu_context, w, h):
    ok = rt.abi.RTOW_SUCCESS
    for case in pp.combine_cases(w, h):
        color, normal, albedo = case["color"], case["normal"], case["albedo"]
        want = {}
        for debug, ldr in FLAGS:
            floats = oracle.combine(w, h, color, normal, albedo, debug_mode=bool(debug), ldr_albedo=bool(ldr))
            want[debug, ldr] = (floats, oracle.finalize(*floats))
        for offset in (0, 4):
            f = Frame(rt, gpu_context, color, normal, albedo, offset)
            try:
                for debug, ldr in FLAGS:
                    what = (case["name"], offset, debug, ldr)
                    f.reset()
                    assert f.combine(w, h, debug, ldr) == ok and f.combine(w, h, debug, ldr, fused=True) == ok
                    _same_floats(f.floats(), want[debug, ldr][0], what)
                    _same_bytes(f.bytes(), want[debug, ldr][1], what + ("fused",))
                    assert f.finalize(w * h, from_f3=True) == ok                   # and the two passes one after the other
                    _same_bytes(f.bytes(), want[debug, ldr][1], what + ("combine, then finalize",))
            finally:
                f.free()


# ---------------------------------------------------------------- finalize
@pytest.fixture(scope="module")
def byte_steps(oracle):
    """the floats round every byte step (a bisection on the CPU oracle) in their nine channel positions, computed once"""
    return pp.finalize_frame(pp.finalize_operands(oracle))


@pytest.mark.parametrize("n", [None, 1, 255, 257])
def test_finalize_at_every_byte_step(rt, oracle, gpu_context, byte_steps, n):
    """rtowFinalizeDevice, and rtowCombineFinalizeDevice with w = 1 (the identity on colour and albedo; the normal is normalised first - the oracle's chain says how),
    on the 17 floats round each of the 255 byte steps and the special values, each in all nine channel positions"""
    ok = rt.abi.RTOW_SUCCESS
    color, normal, albedo = (x[:n] for x in byte_steps)
    n = color.shape[0]
    color4 = np.concatenate([color, np.ones((n, 1), F)], 1)
    direct = oracle.finalize(color, normal, albedo)
    chained = oracle.finalize(*oracle.combine(n, 1, color4, normal, albedo))
    clean = ~np.isnan(color).any(1)
    assert np.array_equal(direct[0][clean], chained[0][clean]) and np.array_equal(direct[2], chained[2])      # the same operands reach the conversion on both routes
    for offset in (0, 4):
        f = Frame(rt, gpu_context, color4, normal, albedo, offset)
        plain = Dev(rt, gpu_context, color.nbytes, offset, color)
        try:
            assert f.finalize(n, c=plain.ptr) == ok
            _same_bytes(f.bytes(), direct, (n, offset, "finalize"))
            f.reset()
            assert f.combine(n, 1, fused=True) == ok
            _same_bytes(f.bytes(), chained, (n, offset, "fused"))
            f.reset()
            assert f.combine(1, n, 1, 1, fused=True) == ok                         # one column, debug mode: nothing to borrow, NaN colours are cyan
            _same_bytes(f.bytes(), oracle.finalize(*oracle.combine(1, n, color4, normal, albedo, debug_mode=True, ldr_albedo=True)), (n, offset, "fused, one column"))
            assert plain.guards_intact()
        finally:
            f.free()
            plain.free()


# ---------------------------------------------------------------- metrics
class Reduction:
    """the inputs of one reduction and a device-resident record, all guarded; the diagnostics in both layouts"""

    def __init__(self, rt, ctx, case, offset=0):
        self.rt, self.ctx, self.n = rt, ctx, case["n"]
        self.diag = {16: Dev(rt, ctx, case["diag"].nbytes, offset, case["diag"]), 4: Dev(rt, ctx, self.n * 4, offset, np.ascontiguousarray(case["diag"][:, :1]))}
        self.color = Dev(rt, ctx, case["color"].nbytes, 0, case["color"])          # read as float4
        self.scw = Dev(rt, ctx, self.n * 4, offset, case["scw"])
        self.records = [Dev(rt, ctx, pp.RECORD.itemsize) for _ in range(3)]

    def everything(self):
        return [self.diag[4], self.diag[16], self.color, self.scw] + self.records

    def blocking(self, stride, n=None, **ptr):
        m = self.rt.abi.Metrics()
        at = {"diag": self.diag.get(stride, self.diag[4]).ptr, "color": self.color.ptr, "scw": self.scw.ptr, "out": C.byref(m), "ctx": self.ctx.handle}
        at.update(ptr)
        rc = self.rt.lib.load().rtowReduceMetricsDevice(at["ctx"], self.n if n is None else n, at["diag"], stride, at["color"], at["scw"], None, at["out"])
        return rc, pp.record_of(m)

    def enqueue(self, stride, out, n=None, **ptr):
        at = {"diag": self.diag.get(stride, self.diag[4]).ptr, "color": self.color.ptr, "scw": self.scw.ptr, "ctx": self.ctx.handle}
        at.update(ptr)
        return self.rt.lib.load().rtowReduceMetricsDeviceAsync(at["ctx"], self.n if n is None else n, at["diag"], stride, at["color"], at["scw"], None, out)

    def record(self, k=0):
        self.guards()
        return self.records[k].download(np.uint8, (pp.RECORD.itemsize,)).view(pp.RECORD)

    def guards(self):
        self.ctx.synchronize()
        for b in self.everything():
            assert b.guards_intact()

    def free(self):
        for b in self.everything():
            b.free()


def _same_record(got, want, what):
    assert got.tobytes() == want.tobytes(), (what, got, want)                      # all 40 bytes


def _metrics_cases():
    return [pp.metrics_frame(n) for n in pp.METRICS_COUNTS] + pp.metrics_edge_cases()


@pytest.fixture(scope="module")
def metrics_cases(oracle):
    """every case with the oracle's record, computed once"""
    cases = _metrics_cases()
    for c in cases:
        c["want"] = pp.record_of(oracle.reduce_metrics(c["diag"], c["color"], c["scw"]))
    return {c["name"]: c for c in cases}


@pytest.mark.parametrize("name", [c["name"] for c in _metrics_cases()])
def test_both_reductions_are_the_oracle(rt, gpu_context, metrics_cases, name):
    ok = rt.abi.RTOW_SUCCESS
    case = metrics_cases[name]
    for offset in (0, 4):
        r = Reduction(rt, gpu_context, case, offset)
        try:
            for stride in (4, 16):
                rc, got = r.blocking(stride)
                assert rc == ok
                r.guards()
                _same_record(got, case["want"], (name, offset, stride, "blocking"))
                r.records[0].buf.upload(np.full((r.records[0].front + pp.RECORD.itemsize + 16) // 4, GUARD, U))
                assert r.enqueue(stride, r.records[0].ptr) == ok
                _same_record(r.record(), case["want"], (name, offset, stride, "asynchronous, into device memory"))
        finally:
            r.free()


def test_back_to_back_reductions_and_registered_host_memory(rt, gpu_context, metrics_cases):
    """Three asynchronous reductions enqueued back to back into three records, then a blocking one: the library orders them on the context's one block of partial
    results, and all four records are the oracle's.  Then the record written by the device into registered host memory, between guard words."""
    ok = rt.abi.RTOW_SUCCESS
    ctx = gpu_context
    first, second = metrics_cases["frame-4096"], metrics_cases["both-wrap"]
    a, b = Reduction(rt, ctx, first), Reduction(rt, ctx, second)
    host = np.full(4 + pp.RECORD.itemsize // 4 + 4, GUARD, U)
    try:
        for k in range(3):
            assert a.enqueue(16, a.records[k].ptr) == ok
        rc, blocking = a.blocking(16)
        assert rc == ok
        records = [a.record(k) for k in range(3)] + [blocking]
        for k, got in enumerate(records):
            _same_record(got, first["want"], ("back to back", k))
        # two frames in turn on the same partial results: neither reads the other's
        assert a.enqueue(4, a.records[0].ptr) == ok and b.enqueue(4, b.records[0].ptr) == ok and a.enqueue(16, a.records[1].ptr) == ok
        rc, blocking = b.blocking(16)
        assert rc == ok
        _same_record(blocking, second["want"], "second frame, blocking")
        _same_record(a.record(0), first["want"], "first frame")
        _same_record(b.record(0), second["want"], "second frame")
        _same_record(a.record(1), first["want"], "first frame again")
        ctx.register_host_buffers(host)
        try:
            assert b.enqueue(4, host.ctypes.data + 16) == ok
            ctx.synchronize()
        finally:
            ctx.unregister_host_buffers()
        assert (host[:4] == GUARD).all() and (host[-4:] == GUARD).all()
        _same_record(host[4:-4].view(pp.RECORD), second["want"], "registered host memory")
        b.guards()
    finally:
        a.free()
        b.free()


# ---------------------------------------------------------------- refusals
def test_refusals_enqueue_nothing(rt, gpu_context, metrics_cases):
    bad = rt.abi.RTOW_ERROR_INVALID_VALUE
    w, h = 37, 3
    case = pp.combine_case(w, h, "scattered", 5)
    f = Frame(rt, gpu_context, case["color"], case["normal"], case["albedo"])
    r = Reduction(rt, gpu_context, metrics_cases["frame-255"])
    try:
        sizes = [(65536, 65536), (65536, 32768), (46341, 46341), (0x7fffffff, 0x7fffffff), (0x7fffffff, 2), (0, h), (w, 0), (-1, h), (w, -1), (-w, -h), (0, 0)]
        for fused in (False, True):
            for dims in sizes:                                                     # width * height beyond INT32_MAX, zero, negative
                assert f.combine(*dims, fused=fused) == bad, (dims, fused)
            for k in ("c", "n", "a", "oc", "on", "oa", "params", "ctx"):
                assert f.combine(w, h, fused=fused, **{k: None}) == bad, (k, fused)
        for n in (0, -1, -w * h, -0x80000000):
            assert f.finalize(n, from_f3=True) == bad, n
        for k in ("c", "n", "a", "oc", "on", "oa", "ctx"):
            assert f.finalize(w * h, from_f3=True, **{k: None}) == bad, k
        assert f.untouched()
        for b in f.ins:
            assert b.guards_intact()

        for n in (0, -1, -0x80000000):
            assert r.blocking(4, n)[0] == bad and r.enqueue(4, r.records[0].ptr, n) == bad, n
        for stride in (0, 8, -4, 12, 32):
            assert r.blocking(stride)[0] == bad and r.enqueue(stride, r.records[0].ptr) == bad, stride
        for k in ("diag", "color", "scw", "ctx"):
            assert r.blocking(4, **{k: None})[0] == bad and r.enqueue(4, r.records[0].ptr, **{k: None}) == bad, k
        assert r.blocking(4, out=None)[0] == bad and r.enqueue(4, None) == bad
        pageable = np.full(18, GUARD, U)
        assert r.enqueue(4, pageable.ctypes.data + 16) == bad and (pageable == GUARD).all(), "the device cannot write pageable host memory"
        r.guards()
        assert all((b.words() == GUARD).all() for b in r.records)
    finally:
        f.free()
        r.free()
