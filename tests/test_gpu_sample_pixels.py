"""GPU tests of rtowSamplePixelsDevice (include/rtow.h): at the pixels of a device list the four accumulators and the diagnostics records are, bit for bit, what the
frame calls store there - rtowSampleBatchDevice, and rtowSampleBatchChainDevice for chains - and what the CPU oracle's sample_pixels computes; every other element of
every output keeps a guard pattern (separate outputs) or its input (in place).  Scenes of every kind with list-capable kernels, lists of 0, 1, 63, 64, 65 entries
and every pixel, built and host-made (shuffled) lists, entries beyond the frame, chains, texture-driven noise, the context's timing and status, what a list launch
leaves behind for the next full batch, the refusals, and hole filling after a reprojection end to end.  Frames are 70 x 37 (ragged tiles), 4 spp at depth 8."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_list_holes as ph  # noqa: E402
import pixel_list_reference as ref  # noqa: E402
from test_gpu_pixel_list import GUARD, Dev  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 70, 37
N = W * H
KEYS = ("color", "normal", "albedo", "scw")
COMPS = (4, 3, 3, 1)


def _zeros(n=N):
    return {k: np.zeros(n * c, F) for k, c in zip(KEYS, COMPS)}


def _upload(rt, ctx, values, n=N):
    """four accumulators between guard words: `values` (a dict of float32 arrays of n pixels), or the guard pattern itself"""
    return [Dev(rt, ctx, n * c * 4, 0, None if values is None else values[k]) for k, c in zip(KEYS, COMPS)]


def _download(devs, n=N):
    return {k: d.payload(np.uint32).reshape(n, c) for k, d, c in zip(KEYS, devs, COMPS)}


def _bits(values):
    return {k: np.ascontiguousarray(values[k], F).view(np.uint32).reshape(-1, c) for k, c in zip(KEYS, COMPS)}


def frame_call(rt, ctx, plist, inputs, n=N):
    """rtowSampleBatchChainDevice (one batch: rtowSampleBatchDevice's launch) from `inputs` into guard-filled outputs: (accumulators, [diagnostics per batch]) as uint32"""
    stride = plist[0].diagnosticsStride
    ins, outs, diags = _upload(rt, ctx, _zeros(n) if inputs is None else inputs, n), _upload(rt, ctx, None, n), [Dev(rt, ctx, n * stride) for _ in plist]
    try:
        rt.lib.check(rt.sample_batch_chain_device(ctx, plist, ins, outs, diags), "rtowSampleBatchChainDevice")
        ctx.synchronize()
        return _download(outs, n), [d.payload(np.uint32).reshape(n, stride // 4) for d in diags]
    finally:
        for d in ins + outs + diags:
            d.free()


def list_call(rt, ctx, plist, inputs, words, capacity, alias=False, n=N, expect=0, diagnostics=True):
    """rtowSamplePixelsDevice over the host-made list `words` (4 + capacity uint32, uploaded) or a device list (an object with .ptr): outputs start as the guard
    pattern, or are the inputs themselves (alias).  Returns (accumulators, [diagnostics], every guard word around every buffer intact) after the call returned `expect`."""
    stride = plist[0].diagnosticsStride
    ins = _upload(rt, ctx, inputs, n)
    outs = ins if alias else _upload(rt, ctx, None, n)
    diags = [Dev(rt, ctx, n * stride) for _ in plist] if diagnostics else None
    lst = Dev(rt, ctx, (4 + capacity) * 4, 0, words) if isinstance(words, np.ndarray) else None
    every = ins + ([] if alias else outs) + (diags or []) + ([lst] if lst else [])
    try:
        rc = rt.sample_pixels_device(ctx, plist, lst.ptr if lst else words.ptr, capacity, ins, outs, diags)
        assert rc == expect, (rc, expect)
        ctx.synchronize()
        if lst:
            assert np.array_equal(lst.payload(np.uint32), words)              # the caller's list is read, never written
        return _download(outs, n), [d.payload(np.uint32).reshape(n, stride // 4) for d in (diags or [])], all(d.guards_intact() for d in every)
    finally:
        for d in every:
            d.free()


def host_list(indices, capacity=None, count=None):
    indices = np.asarray(indices, np.uint32)
    capacity = indices.size if capacity is None else capacity
    words = np.zeros(4 + capacity, np.uint32)
    words[0] = indices.size if count is None else count
    words[4:4 + min(indices.size, capacity)] = indices[:capacity]
    return words, capacity


def listed_pixels(words, capacity, n=N):
    entries = words[4:4 + min(int(words[0]), capacity)]
    return entries[entries < n].astype(np.int64)


def compare(got, got_diag, want, want_diag, untouched, listed, what, n=N):
    """listed pixels: the frame call's bits, in every accumulator and every diagnostics record; all others: `untouched` (a dict of uint32 arrays, or the guard pattern)"""
    sel = np.zeros(n, bool)
    sel[listed] = True
    for k in KEYS:
        bad = np.flatnonzero((got[k][sel] != want[k][sel]).any(1))
        assert bad.size == 0, (what, k, "listed pixels differ from the frame call", np.flatnonzero(sel)[bad[:5]])
        rest = got[k][~sel]
        keep = np.full_like(rest, GUARD) if untouched is None else untouched[k][~sel]
        assert np.array_equal(rest, keep), (what, k, "an unlisted element was written")
    for b, (g, w) in enumerate(zip(got_diag, want_diag)):
        assert np.array_equal(g[sel], w[sel]), (what, "diagnostics of batch %d at listed pixels" % b)
        assert (g[~sel] == GUARD).all(), (what, "diagnostics of batch %d written at an unlisted pixel" % b)


def make_lists(rt, ctx, seed):
    """(name, host words or device list, capacity, device buffers to free): 0, 1, 63, 64, 65 entries, every pixel, a shuffled host list, a list whose count exceeds
    its capacity, and two built lists (a rectangle that sticks out of the frame under a mask; a 2-way row slice)"""
    rng = np.random.default_rng(seed)
    out = []
    for count in (0, 1, 63, 64, 65):
        out.append(("%d entries" % count,) + host_list(rng.choice(N, count, replace=False), capacity=max(count, 1 if count == 0 else count)) + ([],))
    out.append(("every pixel",) + host_list(np.arange(N)) + ([],))
    out.append(("shuffled",) + host_list(rng.permutation(N)[:700]) + ([],))
    out.append(("count beyond the capacity",) + host_list(rng.permutation(N)[:300], capacity=130, count=100000) + ([],))
    mask = (rng.random(N) < 0.6).astype(np.uint8)
    mdev = rt.DeviceBuffer(ctx).upload(mask)
    built, scratch = rt.build_pixel_list(ctx, W, H, 2000, mask=mdev, rect=(-3, 5, 61, H + 4))
    out.append(("built: rectangle and mask", built, 2000, [built, scratch, mdev]))
    sliced, scratch2 = rt.build_pixel_list(ctx, W, H, 400, slice_offset=1, slice_divider=2)        # overflows: 1260 qualify
    out.append(("built: row slice, overflowing", sliced, 400, [sliced, scratch2]))
    ctx.synchronize()
    return out


def words_of(lst, capacity):
    return lst if isinstance(lst, np.ndarray) else lst.download(np.uint32, (4 + capacity,))


def check_scene(rt, ctx, oracle, scene, alias_lists=("every pixel", "shuffled", "65 entries")):
    desc = scene.desc()
    ctx.upload_scene(desc)
    S = rt.scenes
    base = rt.sample_batch_host(ctx, S.make_params(scene, W, H, spp=3, trace_depth=8, seed=11), want_diag=False)      # non-zero inputs: a frame of 3 spp
    base = {k: base[k] for k in KEYS}
    lists = make_lists(rt, ctx, 5)
    try:
        for stride in (4, 16):
            p = S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5, diagnostics_stride=stride)
            want, want_diag = frame_call(rt, ctx, [p], base)
            for name, lst, capacity, _ in lists:
                words = words_of(lst, capacity)
                listed = listed_pixels(words, capacity)
                for alias in ((False, True) if name in alias_lists else (False,)):
                    got, got_diag, intact = list_call(rt, ctx, [p], base, lst, capacity, alias=alias)
                    compare(got, got_diag, want, want_diag, _bits(base) if alias else None, listed, (scene.name, stride, name, alias))
                    assert intact, (scene.name, stride, name, alias)
            if name == "built: row slice, overflowing":
                assert words[0] == (H // 2) * W and listed.size == 400
        # against the oracle: SampleBatchJob.Execute for at least 200 listed pixels
        words, capacity = next((w, c) for nm, w, c, _ in lists if nm == "shuffled")
        p = S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5)
        got, got_diag, _ = list_call(rt, ctx, [p], base, words, capacity)
        some = listed_pixels(words, capacity)[:256]
        osc = oracle.OracleScene(desc)
        try:
            cpu = osc.sample_pixels(p, some, base)
        finally:
            osc.close()
        assert some.size >= 200
        for k, c in zip(KEYS, COMPS):
            assert np.array_equal(got[k][some], np.ascontiguousarray(cpu[k], F).view(np.uint32).reshape(-1, c)), (scene.name, k, "differs from the oracle")
        assert np.array_equal(got_diag[0][some, 0].view(F), cpu["diag"][:, 0]), (scene.name, "ray count differs from the oracle")
    finally:
        for _, _, _, bufs in lists:
            for b in bufs:
                b.free()


SCENES = {"tiny": lambda S: S.tiny_scene(), "cover": lambda S: S.cover_scene(), "moving": lambda S: S.moving_scene(), "twin_spheres": lambda S: S.twin_spheres_scene(),
          "twin_row": lambda S: S.twin_row_scene(), "mesh": lambda S: S.mesh_scene(1), "textured_mesh": lambda S: S.textured_mesh_scene(),
          "triangle_tie_field": lambda S: S.triangle_tie_field_scene()}


@pytest.mark.parametrize("name", list(SCENES))
def test_listed_pixels_equal_the_frame_call_and_the_oracle(rt, gpu_context, oracle, name):
    scene = SCENES[name](rt.scenes)
    if name == "moving":
        assert scene.camera.get("aperture", 0) > 0                       # a lens: the defocus draws are part of the stream
    check_scene(rt, gpu_context, oracle, scene)


@pytest.mark.parametrize("flag,name", [("CONTEXT_FORCE_WIDE_CODES", "cover"), ("CONTEXT_EXACT_TIES_ALWAYS", "twin_spheres")])
def test_under_context_flags(rt, oracle, flag, name):
    ctx = rt.Context(0, flags=getattr(rt.abi, flag))
    try:
        check_scene(rt, ctx, oracle, SCENES[name](rt.scenes), alias_lists=("shuffled",))
        info = ctx.scene_info()
        assert bool(info.wideCodes) == (flag == "CONTEXT_FORCE_WIDE_CODES")
    finally:
        ctx.close()


def test_chains_equal_the_chain_call(rt, gpu_context):
    """three batches that differ only in seed (one launch that carries each pixel through them) and three that also differ in traceDepth (batch by batch): both equal
    rtowSampleBatchChainDevice, which is by definition the sequential calls - accumulators and every batch's diagnostics, separate outputs and in place"""
    ctx, S = gpu_context, rt.scenes
    scene = S.cover_scene()
    ctx.upload_scene(scene.desc())
    base = rt.sample_batch_host(ctx, S.make_params(scene, W, H, spp=3, trace_depth=8, seed=11), want_diag=False)
    base = {k: base[k] for k in KEYS}
    rng = np.random.default_rng(8)
    words, capacity = host_list(rng.permutation(N)[:900])
    listed = listed_pixels(words, capacity)
    for stride in (4, 16):
        seeds = [S.make_params(scene, W, H, spp=4, trace_depth=8, seed=s, diagnostics_stride=stride) for s in (5, 6, 7)]
        depths = [S.make_params(scene, W, H, spp=4, trace_depth=d, seed=s, diagnostics_stride=stride) for s, d in ((5, 8), (6, 5), (7, 8))]
        for plist in (seeds, depths):
            want, want_diag = frame_call(rt, ctx, plist, base)
            sequential = base
            for p in plist:                                              # the definition itself, once more: batch k from batch k - 1's outputs
                step, _ = frame_call(rt, ctx, [p], sequential)
                sequential = {k: step[k].view(F) for k in KEYS}
            for k in KEYS:
                assert np.array_equal(step[k], want[k])
            for alias in (False, True):
                got, got_diag, intact = list_call(rt, ctx, plist, base, words, capacity, alias=alias)
                compare(got, got_diag, want, want_diag, _bits(base) if alias else None, listed, ("chain", stride, plist is seeds, alias))
                assert intact
    # sixteen batches are the most one call takes
    many = [S.make_params(scene, W, H, spp=1, trace_depth=8, seed=s) for s in range(16)]
    want, _ = frame_call(rt, ctx, many, base)
    got, _, intact = list_call(rt, ctx, many, base, words, capacity, diagnostics=False)
    compare(got, [], want, [], None, listed, "sixteen batches")
    assert intact


def test_texture_driven_noise(rt, gpu_context):
    ctx, S, a = gpu_context, rt.scenes, rt.abi
    scene = S.cover_scene()
    ctx.upload_scene(scene.desc())
    noise = S.NoiseTextures(row_stride=8, count=2, seed=3)
    ctx.upload_blue_noise(noise.blue_desc())
    ctx.upload_stb_noise(noise.stb_desc())
    try:
        base = rt.sample_batch_host(ctx, S.make_params(scene, W, H, spp=3, trace_depth=8, seed=11), want_diag=False)
        base = {k: base[k] for k in KEYS}
        words, capacity = host_list(np.random.default_rng(2).permutation(N)[:500])
        for color in (a.NOISE_BLUE, a.NOISE_SPATIOTEMPORAL_BLUE):
            p = S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5, noise_color=color, noise_texture_index=1)
            want, want_diag = frame_call(rt, ctx, [p], base)
            got, got_diag, intact = list_call(rt, ctx, [p], base, words, capacity)
            compare(got, got_diag, want, want_diag, None, listed_pixels(words, capacity), ("noise", color))
            assert intact
    finally:
        ctx.upload_blue_noise(None)
        ctx.upload_stb_noise(None)


def test_entries_beyond_the_frame_are_dropped(rt, gpu_context):
    """an entry >= W * H is never used as an address: the valid entries around it are rendered, nothing else is written, every guard word survives"""
    ctx, S = gpu_context, rt.scenes
    scene = S.cover_scene()
    ctx.upload_scene(scene.desc())
    rng = np.random.default_rng(4)
    good = rng.permutation(N)[:150].astype(np.uint32)
    bad = np.array([N, N + 1, N + 63, 2 * N, 1 << 27, (1 << 27) + 5, (1 << 27) | 3, 1 << 31, 0x7fffffff, 0xfffffffe, 0xffffffff], np.uint32)
    mixed = np.concatenate([good[:70], bad, good[70:], bad[::-1]])
    rng.shuffle(mixed)
    p = S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5)
    want, want_diag = frame_call(rt, ctx, [p], None)
    zeros = _zeros()
    for words, capacity in (host_list(mixed), host_list(bad), host_list(np.full(64, 0xffffffff, np.uint32))):
        listed = listed_pixels(words, capacity)
        for plist in ([p], [p, rt.scenes.make_params(scene, W, H, spp=4, trace_depth=8, seed=6)]):
            if len(plist) == 2:
                want2, want_diag2 = frame_call(rt, ctx, plist, None)
            got, got_diag, intact = list_call(rt, ctx, plist, zeros, words, capacity)
            compare(got, got_diag, want if len(plist) == 1 else want2, want_diag if len(plist) == 1 else want_diag2, None, listed, ("bad entries", len(plist), capacity))
            assert intact
    assert listed_pixels(*host_list(mixed)).size == 150 and listed_pixels(*host_list(bad)).size == 0


def test_timing_and_status_answer_for_the_list_launch(rt, gpu_context):
    ctx, S = gpu_context, rt.scenes
    scene = S.cover_scene()
    ctx.upload_scene(scene.desc())
    p = S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5)
    words, capacity = host_list(np.arange(0, N, 3))
    ins = _upload(rt, ctx, _zeros())
    lst = rt.DeviceBuffer(ctx).upload(words)
    try:
        rt.lib.check(rt.sample_pixels_device(ctx, [p], lst, capacity, ins, ins), "rtowSamplePixelsDevice")
        ctx.batch_status()                                               # waits for the list launch; raises on anything but success
        ms = ctx.last_sample_kernel_ms()
        assert np.isfinite(ms) and 0.0 < ms < 1000.0, ms
        done = _download(ins)
        assert (done["color"][::3, 3].view(F) >= 0).all() and (done["color"].view(F)[np.arange(N) % 3 != 0] == 0).all()
        # an empty list: a launch that leaves at once, still the context's most recent batch
        empty, cap0 = host_list([], capacity=0)
        lst.upload(np.concatenate([empty, np.zeros(4, np.uint32)]))
        rt.lib.check(rt.sample_pixels_device(ctx, [p], lst, cap0, ins, ins), "rtowSamplePixelsDevice")
        ctx.synchronize()
        ms = ctx.last_sample_kernel_ms()
        assert np.isfinite(ms) and 0.0 <= ms < 1000.0, ms
        again = _download(ins)
        for k in KEYS:
            assert np.array_equal(again[k], done[k])
        # the cancel byte: clear, the call waits and reports success
        cancel = C.c_uint8(0)
        assert rt.sample_pixels_device(ctx, [p], lst, cap0, ins, ins, cancel=C.addressof(cancel)) == 0
    finally:
        lst.free()
        for d in ins:
            d.free()


def test_a_list_launch_leaves_no_scheduling_state_behind(rt):
    """320 x 240 (more chunks than four per CU: the frame launches run in chunk order with a ticket map): the full-frame batches of a context that ran list launches
    in between equal those of a context that did not, and what rtowGetSceneInfo says of the thresholds is the same"""
    S = rt.scenes
    scene = S.cover_scene()
    w, h = 320, 240
    n = w * h
    plist = [S.make_params(scene, w, h, spp=4, trace_depth=8, seed=s) for s in (3, 4)]
    between = [S.make_params(scene, w, h, spp=4, trace_depth=8, seed=s) for s in range(20, 36)]      # 64 spp per list call: were they counted, the threshold probes would start
    words, capacity = host_list(np.random.default_rng(1).permutation(n)[:20000])
    results, infos = [], []
    for with_lists in (False, True):
        ctx = rt.Context(0)
        try:
            ctx.upload_scene(scene.desc())
            acc, scrap = _upload(rt, ctx, _zeros(n), n), _upload(rt, ctx, _zeros(n), n)
            lst = rt.DeviceBuffer(ctx).upload(words)
            for p in plist:
                if with_lists:
                    rt.lib.check(rt.sample_pixels_device(ctx, between, lst, capacity, scrap, scrap), "rtowSamplePixelsDevice")
                rt.lib.check(rt.sample_batch_chain_device(ctx, [p], acc, acc), "rtowSampleBatchChainDevice")
            ctx.synchronize()
            results.append(_download(acc, n))
            info = ctx.scene_info()
            infos.append((info.thresholdSet, list(info.schedulerTune), info.hitListCapacity))
            for d in acc + scrap:
                assert d.guards_intact()
                d.free()
            lst.free()
        finally:
            ctx.close()
    for k in KEYS:
        assert np.array_equal(results[0][k], results[1][k]), k
    assert infos[0] == infos[1], infos


def test_unsupported_cases_touch_nothing(rt, gpu_context):
    S, a = rt.scenes, rt.abi
    words, capacity = host_list(np.arange(0, N, 2))
    zeros = _zeros()

    def refused(ctx, p):
        got, got_diag, intact = list_call(rt, ctx, [p], zeros, words, capacity, expect=a.RTOW_ERROR_UNSUPPORTED)
        assert intact and all((got[k] == GUARD).all() for k in KEYS) and (got_diag[0] == GUARD).all()

    for make in (S.mixed_scene, S.volume_scene):                         # the GENERAL and VOLUMES kernels
        scene = make()
        gpu_context.upload_scene(scene.desc())
        refused(gpu_context, S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5))
    scene = S.cover_scene()
    gpu_context.upload_scene(scene.desc())
    for policy in (a.RNG_PER_SAMPLE, a.RNG_PER_SAMPLE_XOROSHIRO):
        refused(gpu_context, S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5, rng_policy=policy))
    ctx = rt.Context(0, flags=a.CONTEXT_EXACT_TIES_NEVER)
    try:
        ctx.upload_scene(scene.desc())
        refused(ctx, S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5))
    finally:
        ctx.close()


def test_refusals_enqueue_nothing(rt, gpu_context):
    lib, a, S = rt.lib.load(), rt.abi, rt.scenes
    bad = a.RTOW_ERROR_INVALID_VALUE
    scene = S.cover_scene()
    good = S.make_params(scene, W, H, spp=4, trace_depth=8, seed=5)
    words, capacity = host_list(np.arange(N))
    ctx = gpu_context
    ctx.upload_scene(scene.desc())
    outs = _upload(rt, ctx, None)
    diag = Dev(rt, ctx, N * 4)
    lst = rt.DeviceBuffer(ctx).upload(words)
    bufs = a.AccumBuffers(*[d.ptr for d in outs])

    def call(params_list, handle=ctx.handle, with_list=True, list_words=lst.ptr, ins=bufs, out=bufs, count=None):
        arr = (a.SampleParams * len(params_list))(*params_list)
        l = a.PixelList(list_words, capacity)
        dptr = (C.c_void_p * len(params_list))(*[diag.ptr] * len(params_list))
        return lib.rtowSamplePixelsDevice(handle, len(params_list) if count is None else count, arr, C.byref(l) if with_list else None,
                                          C.byref(ins) if ins is not None else None, C.byref(out) if out is not None else None, dptr, None, None)

    def edited(**fields):
        q = a.SampleParams.from_buffer_copy(good)
        for k, v in fields.items():
            setattr(q, k, v)
        return q

    try:
        assert call([good], handle=None) == bad
        assert call([good], with_list=False) == bad and call([good], list_words=None) == bad
        assert call([good], ins=None) == bad and call([good], out=None) == bad
        assert call([good], out=a.AccumBuffers(outs[0].ptr, None, outs[2].ptr, outs[3].ptr)) == bad
        assert call([good], count=0) == bad and call([good] * 17) == bad
        for q in (edited(sliceDivider=2), edited(sliceOffset=1, sliceDivider=2), edited(sliceDivider=0), edited(size=a.Float2(float(1 << 14), float((1 << 13) + 1))),
                  edited(size=a.Float2(0.0, 37.0)), edited(traceDepth=0), edited(noiseColor=7), edited(rngPolicy=9), edited(diagnosticsStride=8)):
            assert call([q]) == bad
            assert call([good, q]) == bad
        assert call([good, edited(size=a.Float2(37.0, 70.0))]) == bad
        assert call([edited(traceDepth=65)]) == a.RTOW_ERROR_CAPACITY
        assert call([edited(noiseColor=a.NOISE_BLUE)]) == bad             # no blue-noise set is uploaded
        fresh = rt.Context(0)
        try:
            assert call([good], handle=fresh.handle) == a.RTOW_ERROR_NO_SCENE
        finally:
            fresh.close()
        ctx.synchronize()
        assert all((d.bytes().view(np.uint32) == GUARD).all() for d in outs + [diag])      # nothing was enqueued
        assert call([good]) == a.RTOW_SUCCESS                            # and the same arguments, unedited, render
        ctx.synchronize()
        assert not (diag.payload(np.uint32) == GUARD).any() and all(d.guards_intact() for d in outs + [diag])      # every pixel's ray count is there
    finally:
        lst.free()
        for d in outs + [diag]:
            d.free()


def test_hole_filling_after_a_reprojection(rt, gpu_context):
    """The cover scene at 96 x 54: 8 spp, the camera dollies (tests/pixel_list_holes.py; its holes are checked on the CPU by tests/test_pixel_list_holes.py),
    rtowTraceViewDevice at both views, rtowReprojectAccumDevice, a list of the pixels with color.w < 1, a list launch of 8 spp in place.  Then every pixel has
    color.w >= 1 except pixels whose 8 samples all failed (the frame call from the same reprojected inputs says which), listed pixels equal that frame call, and
    unlisted pixels are the reprojected values bit for bit.  The holes are non-empty and under half the frame."""
    ctx, S = gpu_context, rt.scenes
    scene = S.cover_scene()
    ctx.upload_scene(scene.desc())
    w, h = ph.W, ph.H
    n = w * h
    view_a, view_b = ph.views(scene)
    pa = S.make_params(scene, w, h, spp=8, trace_depth=8, seed=1)
    pb = S.make_params(scene, w, h, spp=8, trace_depth=8, seed=5)
    pb.view = view_b
    acc_a = rt.sample_batch_host(ctx, pa, want_diag=False)
    hits_a = ctx.trace_view(view_a, w, h, want=("distance", "entityIndex"))
    hits_b = ctx.trace_view(view_b, w, h, want=("distance", "entityIndex"), want_rays=True)
    bufs = []

    def up(x):
        bufs.append(rt.DeviceBuffer(ctx).upload(x))
        return bufs[-1]

    try:
        job = rt.ReprojectJob(ctx, w, h, view_a)
        job.Rays, job.HitDistance, job.HitEntityIndex = up(hits_b["rays"]), up(hits_b["distance"]), up(hits_b["entityIndex"])
        job.PreviousHitDistance, job.PreviousHitEntityIndex = up(hits_a["distance"]), up(hits_a["entityIndex"])
        job.PreviousColor, job.PreviousNormal, job.PreviousAlbedo, job.PreviousSampleCountWeight = [up(acc_a[k]) for k in KEYS]
        outs = [rt.DeviceBuffer(ctx, n * c * 4) for c in COMPS]
        bufs.extend(outs)
        job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = outs
        assert job.Schedule().Complete() == 0
        ctx.synchronize()
        carried = {k: b.download(F, (n * c,)) for k, b, c in zip(KEYS, outs, COMPS)}
        holes, scratch = rt.build_pixel_list(ctx, w, h, n, color=outs[0], min_sample_count=1.0)
        bufs.extend([holes, scratch])
        rt.lib.check(rt.sample_pixels_device(ctx, [pb], holes, n, outs, outs), "rtowSamplePixelsDevice")
        ctx.synchronize()
        words = holes.download(np.uint32, (4 + n,))
        filled = {k: b.download(np.uint32, (n, c)) for k, b, c in zip(KEYS, outs, COMPS)}
    finally:
        for b in bufs:
            b.free()
    total = int(words[0])
    print("hole filling: %d of %d pixels (%.3f) listed" % (total, n, total / n))
    assert 0 < total and total < n / 2
    want_words = ref.build_pixel_list(w, h, n, color=carried["color"], min_sample_count=1.0)
    assert np.array_equal(words[:4 + total], want_words[:4 + total])
    listed = words[4:4 + total].astype(np.int64)
    want, _ = frame_call(rt, ctx, [pb], carried, n)
    sel = np.zeros(n, bool)
    sel[listed] = True
    before = _bits(carried)
    for k in KEYS:
        assert np.array_equal(filled[k][sel], want[k][sel]), (k, "listed pixels differ from the frame call")
        assert np.array_equal(filled[k][~sel], before[k][~sel]), (k, "an unlisted pixel changed")
    count, frame_count = filled["color"][:, 3].view(F), want["color"][:, 3].view(F)
    short = count < 1
    assert (sel[short]).all() and (frame_count[short] == 0).all()         # only pixels whose 8 samples all failed are left without one
    assert (count[~sel] >= 1).all()
    assert short.sum() < total                                            # and the launch did give samples to the holes
