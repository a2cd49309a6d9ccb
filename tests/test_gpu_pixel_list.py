"""GPU tests of rtowBuildPixelListDevice (include/rtow.h): the builder word for word against the numpy restatement of its specification
(tests/pixel_list_reference.py) - header words, order, overflow total, guard words behind 4 + capacity - with inputs at odd addresses, the refusals with a real
context (nothing enqueued), and determinism.  All in the session context, no subprocesses, no scene."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_list_reference as ref  # noqa: E402
from test_pixel_list_abi import builder_refusals  # noqa: E402
from test_pixel_list_reference import frame_inputs, rectangles  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0x5AFEC0DE
W, H = 70, 37                 # ragged tiles on both axes: 9 x 5 tiles, the last column 6 wide, the last row 5 high


class Dev:
    """device memory `offset` bytes into its allocation, with 16 guard bytes before and after it"""

    def __init__(self, rt, ctx, nbytes, offset=0, data=None):
        self.nbytes, self.front = nbytes, 16 + offset
        total = (self.front + nbytes + 16 + 3) // 4 * 4
        host = np.full(total // 4, GUARD, np.uint32).view(np.uint8)
        if data is not None:
            host[self.front: self.front + nbytes] = np.ascontiguousarray(data).view(np.uint8).ravel()
        self.total = total
        self.buf = rt.DeviceBuffer(ctx).upload(host)

    @property
    def ptr(self):
        return self.buf.ptr + self.front

    def bytes(self):
        return self.buf.download(np.uint8, (self.total,))

    def payload(self, dtype):
        return self.bytes()[self.front: self.front + self.nbytes].copy().view(dtype)

    def guards_intact(self):
        x = self.bytes()
        pattern = np.full(self.total // 4, GUARD, np.uint32).view(np.uint8)
        return np.array_equal(x[: self.front], pattern[: self.front]) and np.array_equal(x[self.front + self.nbytes:], pattern[self.front + self.nbytes:])

    def free(self):
        self.buf.free()


def run_builder(rt, ctx, width, height, capacity, color=None, mask=None, bound=0.0, rect=None, offset=0, divider=1, color_offset=0, mask_offset=0, stream=None):
    """one call with fresh buffers: the list's words (4 + capacity, from a guard pattern) and whether every guard survived"""
    a = rt.abi
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, width, height)
    bufs = {"words": Dev(rt, ctx, a.pixel_list_bytes(capacity)), "scratch": Dev(rt, ctx, a.pixel_list_scratch_bytes(width, height))}
    if color is not None:
        bufs["color"] = Dev(rt, ctx, color.nbytes, color_offset, color)
    if mask is not None:
        bufs["mask"] = Dev(rt, ctx, mask.nbytes, mask_offset, mask)
    try:
        job = rt.PixelListJob(ctx, width, height, capacity, x0, y0, x1, y1, offset, divider, bound)
        job.Color = bufs["color"].ptr if color is not None else None
        job.Mask = bufs["mask"].ptr if mask is not None else None
        job.List, job.Scratch = bufs["words"].ptr, bufs["scratch"].ptr
        assert job.Schedule(stream).Complete() == a.RTOW_SUCCESS
        ctx.synchronize()
        return bufs["words"].payload(np.uint32), all(b.guards_intact() for b in bufs.values())
    finally:
        for b in bufs.values():
            b.free()


@pytest.mark.parametrize("width,height", [(1, 1), (7, 5), (8, 8), (W, H), (129, 65)])
def test_word_for_word_against_the_restatement(rt, gpu_context, width, height):
    """every rectangle x slice x input combination of the CPU test of the restatement, at a capacity that holds the frame; the mask one byte into its allocation and the
    colour four bytes into its allocation in every other case"""
    mask, color = frame_inputs(width, height, 1000 * width + height)
    capacity = width * height
    k = 0
    for rect in rectangles(width, height):
        for divider, offset in ((1, 0), (2, 1), (3, 2)):
            for use_mask, use_color, bound in ((False, False, 0.0), (True, False, 0.0), (False, True, 1.0), (True, True, 2.0)):
                m, c = mask if use_mask else None, color if use_color else None
                want = ref.build_pixel_list(width, height, capacity, fill=GUARD, color=c, mask=m, min_sample_count=bound, rect=rect, slice_offset=offset, slice_divider=divider)
                got, intact = run_builder(rt, gpu_context, width, height, capacity, c, m, bound, rect, offset, divider, color_offset=4 * (k % 2), mask_offset=k % 2)
                assert np.array_equal(got, want), (rect, divider, offset, use_mask, use_color, bound, got[:8], want[:8])
                assert intact
                k += 1


def test_overflow_total_and_guards_behind_the_capacity(rt, gpu_context):
    """capacities of 0, one below the total, the total and one above it: the FIRST capacity qualifiers, words[0] the total, nothing behind min(total, capacity)"""
    mask, color = frame_inputs(W, H, 7)
    total = int(ref.qualifiers(W, H, color=color, mask=mask, min_sample_count=2.0).size)
    assert 64 < total < W * H
    for capacity in (0, 1, 63, 64, 65, total - 1, total, total + 1):
        want = ref.build_pixel_list(W, H, capacity, fill=GUARD, color=color, mask=mask, min_sample_count=2.0)
        got, intact = run_builder(rt, gpu_context, W, H, capacity, color, mask, 2.0, color_offset=4, mask_offset=1)
        assert got[0] == total and not got[1:4].any()
        assert np.array_equal(got, want), (capacity, got[:8], want[:8])
        assert intact, capacity


def test_a_frame_of_many_scan_rounds(rt, gpu_context):
    """1100 x 1000: 17 250 tiles, 17 rounds of the scan's 1024 with a ragged last one; a sparse random mask"""
    width, height = 1100, 1000
    rng = np.random.default_rng(3)
    mask = (rng.random(width * height) < 0.03).astype(np.uint8)
    want = ref.build_pixel_list(width, height, 40000, fill=GUARD, mask=mask)
    assert 4 + want[0] < want.size
    got, intact = run_builder(rt, gpu_context, width, height, 40000, mask=mask, mask_offset=3)
    assert np.array_equal(got, want) and intact


def test_two_calls_give_identical_words(rt, gpu_context):
    mask, color = frame_inputs(129, 65, 11)
    a, _ = run_builder(rt, gpu_context, 129, 65, 5000, color, mask, 3.0)
    b, _ = run_builder(rt, gpu_context, 129, 65, 5000, color, mask, 3.0)
    assert np.array_equal(a, b)


def test_refusals_enqueue_nothing(rt, gpu_context):
    lib, a = rt.lib.load(), rt.abi
    bad = a.RTOW_ERROR_INVALID_VALUE
    capacity = 100
    mask, color = frame_inputs(W, H, 5)
    # real device buffers, each between guard words: a call that were enqueued after all would show in them
    bufs = {"color": Dev(rt, gpu_context, color.nbytes, 0, color), "mask": Dev(rt, gpu_context, mask.nbytes, 0, mask),
            "scratch": Dev(rt, gpu_context, a.pixel_list_scratch_bytes(W, H)), "words": Dev(rt, gpu_context, a.pixel_list_bytes(capacity))}
    addr = {k: b.ptr for k, b in bufs.items()}

    def call(params, ctx=gpu_context.handle, **over):
        p, with_list = dict(addr), True
        for k, v in over.items():
            if k == "list":
                with_list = False
            else:
                p[k] = None if v is None else addr[v[0]] + v[1]
        lst = a.PixelList(p["words"], capacity)
        return lib.rtowBuildPixelListDevice(ctx, C.byref(a.PixelListParams(*params)), p["color"], p["mask"], p["scratch"], C.byref(lst) if with_list else None, None)

    try:
        good, cases = builder_refusals(a, W, H, capacity)
        assert call(good, ctx=None) == bad
        lst = a.PixelList(addr["words"], capacity)
        assert lib.rtowBuildPixelListDevice(gpu_context.handle, None, addr["color"], addr["mask"], addr["scratch"], C.byref(lst), None) == bad
        for label, params, over in cases:
            assert call(params, **over) == bad, (label, params, over)
        gpu_context.synchronize()
        for k in ("scratch", "words"):
            assert (bufs[k].bytes().view(np.uint32) == GUARD).all(), k       # nothing was enqueued
        # a negative or NaN bound is only refused where a colour is given; an empty rectangle and a capacity of 0 are valid
        assert call(good[:8] + (-1.0,) + good[9:], color=None) == a.RTOW_SUCCESS
        assert call(good[:8] + (float("nan"),) + good[9:], color=None) == a.RTOW_SUCCESS
        assert call((W, H, 5, 5, 5, 9) + good[6:]) == a.RTOW_SUCCESS
        gpu_context.synchronize()
        assert bufs["words"].payload(np.uint32)[:4].tolist() == [0, 0, 0, 0]
        assert call(good) == a.RTOW_SUCCESS
        gpu_context.synchronize()
        want = ref.build_pixel_list(W, H, capacity, fill=GUARD, color=color, mask=mask, min_sample_count=1.0)
        assert np.array_equal(bufs["words"].payload(np.uint32), want)
        assert all(b.guards_intact() for b in bufs.values())
    finally:
        for b in bufs.values():
            b.free()
