"""GPU: one context, many launches - what launchSample carries from one batch to the next must never show in a frame - and a fractional Size.

Almost every other GPU test renders on a context prepared for that one launch.  A real host keeps one context for hours and changes one field of RtowSampleParams at a
time; the camera-ray lists, the chunk order with its cost and ticket maps, the threshold probes, the LDS plan with its spill areas, the tie watch and the unit records
each decide for themselves when they are stale.  Here every change of tests/launch_sequences.py is made under a warm context and inside one call of every multi-batch
entry point, and SampleBatchJob.Size - a float2 whose fraction the reference divides by - is rendered with a fraction through every form of launch.

Everything is bit for bit against the oracle: the four accumulators as uint32 and RayCount, on every pixel, from random non-zero accumulators so that a row or a pixel a
launch must not touch would show.  Frames are 32 x 18 (64 x 36 for the cover scene), 4 samples per pixel at depth 8 unless the change says otherwise.  An oracle frame is
computed once per (scene, block) and shared by the tests of this file."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_sequences as L  # noqa: E402
import pixel_list_reference as pixel_lists  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
KEYS = ("color", "normal", "albedo", "scw")
COMPS = (4, 3, 3, 1)
SENTINEL = f32(-7777.25)
SCENES = ("cover", "tiny", "mixed", "mesh", "textured", "volume")      # one per kernel family


def _make_scene(rt, name):
    S = rt.scenes
    return {"cover": lambda: S.cover_scene(60, 600), "tiny": S.tiny_scene, "mixed": S.mixed_scene, "mesh": lambda: S.mesh_scene(1), "textured": S.textured_scene,
            "volume": S.volume_scene}[name]()


def _frame(name):
    return (64, 36) if name == "cover" else (32, 18)


_starts = {}


def start(n):
    """random non-zero accumulators of n pixels (as in tests/test_gpu_matrix.py); never modified"""
    if n not in _starts:
        rng = np.random.default_rng(3)
        s = {"color": rng.random((n, 4)).astype(f32), "normal": rng.normal(size=(n, 3)).astype(f32), "albedo": rng.random((n, 3)).astype(f32), "scw": rng.random(n).astype(f32)}
        s["color"][:, 3] = rng.integers(0, 4, n)
        for v in s.values():
            v.setflags(write=False)
        _starts[n] = s
    return _starts[n]


class Reference:
    """a scene, its oracle with the noise sets and the cubemap every context of this file uploads, and the oracle's frames from start(), once per block"""

    def __init__(self, rt, oracle, name):
        S = rt.scenes
        self.name, self.scene = name, _make_scene(rt, name)
        self.desc = self.scene.desc()
        self.textures = S.NoiseTextures(row_stride=8, count=3, seed=7)
        self.cube = S.synthetic_sky(size=8, half=True, seed=5)
        self.osc = oracle.OracleScene(self.desc)
        self.osc.set_blue_noise(self.textures.blue_desc()); self.osc.set_stb_noise(self.textures.stb_desc()); self.osc.set_cubemap(self.cube.desc())
        self.frames = {}

    def prepare(self, ctx):
        ctx.upload_blue_noise(self.textures.blue_desc()); ctx.upload_stb_noise(self.textures.stb_desc()); ctx.upload_sky_cubemap(self.cube.desc())
        ctx.upload_scene(self.desc)

    def batch(self, p, inputs):
        return self.osc.sample_batch(p, {k: inputs[k] for k in KEYS})

    def frame(self, p):
        """the oracle's frame for this block from start(W * H)"""
        key = bytes(p)
        if key not in self.frames:
            w, h = L.frame_size(p)
            self.frames[key] = self.batch(p, start(w * h))
        return self.frames[key]


_references = {}


def reference(rt, oracle, name):
    if name not in _references:
        _references[name] = Reference(rt, oracle, name)
    return _references[name]


def differences(got, want):
    """[] when the four accumulators agree as uint32 on every pixel; else which differ, in how many pixels"""
    out = []
    for k, c in zip(KEYS, COMPS):
        g, w = np.ascontiguousarray(got[k], f32).reshape(-1, c).view(np.uint32), np.ascontiguousarray(want[k], f32).reshape(-1, c).view(np.uint32)
        if g.shape != w.shape:
            out.append((k, "shape", g.shape, w.shape))
        elif not np.array_equal(g, w):
            out.append((k, int((g != w).any(axis=1).sum()), "pixels"))
    return out


def record_differences(diag, want_diag, every_counter=False, rows=slice(None)):
    """[] when RayCount - with every_counter all four counters of a 16-byte record, as uint32 - agrees on every pixel of `rows`"""
    g, w = np.ascontiguousarray(diag, f32)[rows], np.ascontiguousarray(want_diag, f32)[rows]
    if every_counter:
        g, w = g.view(np.uint32), w.view(np.uint32)
    else:
        g, w = g[:, :1], w[:, :1]
    if g.shape != w.shape:
        return [("diagnostics", "shape", g.shape, w.shape)]
    return [] if np.array_equal(g, w) else [("diagnostics" if every_counter else "RayCount", int((g != w).any(axis=1).sum()), "pixels")]


def _single(rt, ctx, ref, p, every_counter=False):
    w, h = L.frame_size(p)
    want = ref.frame(p)
    got = rt.sample_batch_host(ctx, p, start(w * h))
    return differences(got, want) + record_differences(got["diag"], want["diag"], every_counter)


def _device(rt, ctx, values):
    return [rt.DeviceBuffer(ctx).upload(np.ascontiguousarray(values[k], f32)) for k in KEYS]


def _sentinels(n):
    return {k: np.full((n, c), SENTINEL, f32) for k, c in zip(KEYS, COMPS)}


def _download(bufs, n):
    return {k: b.download(f32, (n, c)) for k, b, c in zip(KEYS, bufs, COMPS)}


def _seeded(p, seed):
    q = L.copy_params(p)
    q.seed = seed
    return q


def _with_size(p, size):
    q = L.copy_params(p)
    q.size = L.abi.Float2(*size)
    return q


def _oracle_chain(ref, plist, first):
    """the batches one after the other over flat buffers of max(W * H) pixels (a batch of another frame size indexes the same memory): (accumulators, [diag per batch])"""
    acc = {k: np.array(first[k], f32, copy=True).reshape(-1, c) for k, c in zip(KEYS, COMPS)}
    diags = []
    for p in plist:
        w, h = L.frame_size(p)
        n = w * h
        r = ref.batch(p, {k: acc[k][:n].reshape(-1) if k == "scw" else acc[k][:n] for k in KEYS})
        for k, c in zip(KEYS, COMPS):
            acc[k][:n] = r[k].reshape(n, c)
        diags.append(r["diag"])
    return acc, diags


def _owned(p, n_total):
    """which of the n_total pixels of a flat buffer this batch writes: the rows of its slice, inside its frame"""
    w, h = L.frame_size(p)
    rows = (np.arange(h) % p.sliceDivider) == p.sliceOffset
    own = np.zeros(n_total, bool)
    own[:w * h] = np.repeat(rows, w)
    return own


# ================================================================== fractional Size, single launches ==================================================================
@pytest.mark.parametrize("name", SCENES)
def test_fractional_size_in_a_batch_a_fused_chain_and_a_group(rt, oracle, name):
    """The four fractional sizes through rtowSampleBatch, as a chain of three that differs in the seed alone (rtowSampleBatchChainDevice: one fused launch where the device
    fuses), and as a group of three (rtowSampleBatchGroupDevice) - on one context per scene, so that each size also follows another with the same integer frame."""
    ref = reference(rt, oracle, name)
    w, h = _frame(name)
    n = w * h
    P = L.base_params(ref.scene, w, h)
    bad = []
    with rt.Context(0) as ctx:
        ref.prepare(ctx)
        for size in L.fractional_sizes(w, h):
            p = _with_size(P, size)
            plist = [_seeded(p, s) for s in (p.seed, 41, 97)]
            bad += [(size, "batch") + d for d in _single(rt, ctx, ref, p)]
            # chain, in place in device buffers
            want, want_diags = _oracle_chain(ref, plist, start(n))
            bufs = _device(rt, ctx, start(n))
            diags = [rt.DeviceBuffer(ctx, n * 4).zero() for _ in plist]
            assert rt.sample_batch_chain_device(ctx, plist, bufs, bufs, diags) == 0
            ctx.synchronize()
            got = _download(bufs, n)
            bad += [(size, "chain") + d for d in differences(got, want)]
            for b, d in enumerate(diags):
                bad += [(size, "chain batch %d" % b) + x for x in record_differences(d.download(f32, (n, 1)), want_diags[b])]
            # group: every batch from the same inputs into its own outputs
            ins, outs = _device(rt, ctx, start(n)), [_device(rt, ctx, _sentinels(n)) for _ in plist]
            assert rt.sample_batch_group_device(ctx, plist, ins, outs, diags) == 0
            ctx.synchronize()
            for b, q in enumerate(plist):
                alone = ref.frame(q)
                bad += [(size, "group batch %d" % b) + x for x in differences(_download(outs[b], n), alone) + record_differences(diags[b].download(f32, (n, 1)), alone["diag"])]
            for buf in bufs + ins + diags + [x for o in outs for x in o]:
                buf.free()
    assert not bad, bad


SWITCHES = ("per_sample", "xoroshiro", "blue noise", "slice 1/3", "reference diagnostics", "tree in HBM", "wide codes")


@pytest.mark.parametrize("switch", SWITCHES)
def test_fractional_size_cover_scene_under_every_switch(rt, oracle, switch):
    """rtowSampleBatch at the four fractional sizes under both per-sample policies, blue noise, slice 1 of 3, 16-byte records with RTOW_CONTEXT_REFERENCE_DIAGNOSTICS (all
    four counters compared), lds_scene_budget = 1024 and RTOW_CONTEXT_FORCE_WIDE_CODES"""
    a = rt.abi
    ref = reference(rt, oracle, "cover")
    w, h = _frame("cover")
    P = L.base_params(ref.scene, w, h)
    options = {}
    if switch == "per_sample":
        P.rngPolicy = a.RNG_PER_SAMPLE
    elif switch == "xoroshiro":
        P.rngPolicy = a.RNG_PER_SAMPLE_XOROSHIRO
    elif switch == "blue noise":
        P.noiseColor = a.NOISE_BLUE
    elif switch == "slice 1/3":
        P.sliceOffset, P.sliceDivider = 1, 3
    elif switch == "reference diagnostics":
        P.diagnosticsStride = 16
        options["flags"] = a.CONTEXT_REFERENCE_DIAGNOSTICS
    elif switch == "tree in HBM":
        options["lds_scene_budget"] = 1024
    elif switch == "wide codes":
        options["flags"] = a.CONTEXT_FORCE_WIDE_CODES
    bad = []
    with rt.Context(0, **options) as ctx:
        ref.prepare(ctx)
        info = ctx.scene_info()
        if switch == "tree in HBM":
            assert not info.sceneInLds
        if switch == "wide codes":
            assert info.wideCodes
        for size in [(float(w), float(h))] + L.fractional_sizes(w, h):        # the integer size first: the fractional ones follow it on a warm context
            bad += [(size,) + d for d in _single(rt, ctx, ref, _with_size(P, size), every_counter=switch == "reference diagnostics")]
    assert not bad, bad


def _checkerboard(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return ((x + y) % 2 == 0).astype(np.uint8)


def test_fractional_size_over_a_pixel_list(rt, oracle):
    """rtowSamplePixelsDevice over a checkerboard list (tests/pixel_list_reference.py): the listed pixels are the oracle's frame, every other element keeps its sentinel"""
    ref = reference(rt, oracle, "cover")
    w, h = _frame("cover")
    n = w * h
    P = L.base_params(ref.scene, w, h)
    words = pixel_lists.build_pixel_list(w, h, n, mask=_checkerboard(w, h))
    listed = words[4:4 + int(words[0])].astype(np.int64)
    assert listed.size == n // 2
    sel = np.zeros(n, bool)
    sel[listed] = True
    bad = []
    with rt.Context(0) as ctx:
        ref.prepare(ctx)
        lst = rt.DeviceBuffer(ctx).upload(words)
        for size in [(float(w), float(h))] + L.fractional_sizes(w, h):
            p = _with_size(P, size)
            want = ref.frame(p)
            ins, outs, diag = _device(rt, ctx, start(n)), _device(rt, ctx, _sentinels(n)), rt.DeviceBuffer(ctx).upload(np.full((n, 1), SENTINEL, f32))
            assert rt.sample_pixels_device(ctx, [p], lst, n, ins, outs, [diag]) == 0
            ctx.synchronize()
            got, got_diag = _download(outs, n), diag.download(f32, (n, 1))
            bad += [(size, "listed") + d for d in differences({k: got[k][sel] for k in KEYS}, {k: want[k].reshape(n, -1)[sel] for k in KEYS})
                    + record_differences(got_diag, want["diag"], rows=sel)]
            for k in KEYS:
                if not (got[k][~sel] == SENTINEL).all():
                    bad.append((size, k, "an unlisted pixel was written"))
            if not (got_diag[~sel] == SENTINEL).all():
                bad.append((size, "diagnostics of an unlisted pixel were written"))
            for b in ins + outs + [diag]:
                b.free()
        lst.free()
    assert not bad, bad


def test_fractional_size_recorded_paths_add_up_to_the_frame(rt, oracle):
    """rtowRecordPathsDevice: the four recorded samples of every listed pixel add up, in float32 and in order, to what the sample kernel stores there from zeroed
    accumulators (tests/test_gpu_record_paths.py checks the same at integer sizes) - and that frame is the oracle's"""
    from test_gpu_record_paths import _accumulate, _bits, _zeros
    ref = reference(rt, oracle, "cover")
    w, h = _frame("cover")
    n = w * h
    listed = np.flatnonzero(_checkerboard(w, h).reshape(-1))
    P = L.base_params(ref.scene, w, h)
    zeros = _zeros(n)
    bad = []
    with rt.Context(0) as ctx:
        ref.prepare(ctx)
        for size in L.fractional_sizes(w, h):
            p = _with_size(P, size)
            out = rt.sample_batch_host(ctx, p, zeros)
            want = ref.batch(p, zeros)
            bad += [(size, "frame") + d for d in differences(out, want) + record_differences(out["diag"], want["diag"])]
            records = [ctx.record_paths(p, listed, sample_index=k, want_segments=False) for k in range(4)]
            acc, count, rays = _accumulate({k: zeros[k][listed] for k in ("color", "normal", "albedo")}, records, upto=np.full(listed.size, 4))
            for key in ("color", "normal", "albedo"):
                has = count > 0 if key != "color" else np.ones(listed.size, bool)
                if not np.array_equal(_bits(out[key][listed][:, :3][has]), _bits(acc[key][has])):
                    bad.append((size, "records", key))
            if not np.array_equal(out["color"][listed, 3], count) or not np.array_equal(rays.astype(f32), out["diag"][listed, 0]):
                bad.append((size, "records", "sample or ray counts"))
    assert not bad, bad


# ================================================================== a warm context forgets the previous launch ==================================================================
@pytest.mark.parametrize("name", SCENES)
def test_a_warm_context_forgets_the_previous_launch(rt, oracle, name):
    """One context per scene, the scene uploaded once with blue noise, STBN and a cubemap.  For every mutation m of tests/launch_sequences.py: P0, m(P0), P0 back to back
    through rtowSampleBatch, each of the three frames the oracle's for that block.  The sequence is never reset between mutations, so whatever one launch leaves behind
    meets every later one.  After 16 launches of 4 samples the context has passed kTuneMinSamplesPerPixel (64 samples per pixel since the upload), the first condition of
    the threshold probes; the second is a chunk order on hand, which frames of fewer than 4 * CUs chunks never have - test_order_cost_map_and_ticket_map_live renders
    behind the probes.  scene_info().thresholdSet is read at the end without error; its value is not asserted (when probes finish is timing)."""
    ref = reference(rt, oracle, name)
    w, h = _frame(name)
    P = L.base_params(ref.scene, w, h)
    bad = []
    with rt.Context(0) as ctx:
        ref.prepare(ctx)
        for m in L.MUTATIONS:
            p0 = m.base(P, ref.scene)
            for step, p in enumerate((p0, m.apply(p0, ref.scene), p0)):
                bad += [(m.name, ("P0", "m(P0)", "P0 again")[step]) + d for d in _single(rt, ctx, ref, p)]
        print(name, "thresholdSet after the sequence:", int(ctx.scene_info().thresholdSet))
    assert not bad, bad


# ================================================================== the same changes inside one call ==================================================================
def _run_entry(rt, ctx, ref, entry, plist, listed_words=None):
    """[P0, m(P0), P0] through one call: (status, differences from the oracle - or from the sentinels where the call is refused)"""
    a = rt.abi
    lib = rt.lib.load()
    sizes = [L.frame_size(p) for p in plist]
    n = max(w * h for w, h in sizes)
    count = len(plist)
    first = start(n)
    diag_words = [p.diagnosticsStride // 4 for p in plist]
    diag_start = [np.full((w * h, c), SENTINEL, f32) for (w, h), c in zip(sizes, diag_words)]
    expect = L.expected_status(entry, plist)
    bad = []

    def check_diags(got_diags, want_diags, owned=None):
        for b in range(count):
            rows = slice(None) if owned is None else owned[b][:got_diags[b].shape[0]]
            bad.extend(("batch %d" % b,) + d for d in record_differences(got_diags[b], want_diags[b], rows=rows))

    if entry == "rtowSampleBatchChain":
        ins = {k: np.ascontiguousarray(first[k], f32) for k in KEYS}
        out = _sentinels(n)
        out["scw"] = out["scw"].reshape(n)
        diags = [d.copy() for d in diag_start]
        arr = (a.SampleParams * count)(*plist)
        bi = a.AccumBuffers(*[ins[k].ctypes.data for k in KEYS])
        bo = a.AccumBuffers(*[out[k].ctypes.data for k in KEYS])
        dptr = (C.c_void_p * count)(*[d.ctypes.data for d in diags])
        rc = lib.rtowSampleBatchChain(ctx.handle, count, arr, C.byref(bi), C.byref(bo), dptr, None)
        if expect == 0 and rc == 0:
            want, want_diags = _oracle_chain(ref, plist, first)
            bad += differences(out, want)
            check_diags(diags, want_diags)
        elif rc == expect:
            bad += [("refused, but written:",) + d for d in differences(out, _sentinels(n))]
            bad += [("refused, but diagnostics of batch %d written" % b,) for b in range(count) if not np.array_equal(diags[b], diag_start[b])]
        return rc, expect, bad

    diags = [rt.DeviceBuffer(ctx).upload(d) for d in diag_start]
    every = list(diags)
    try:
        if entry in ("rtowSampleBatchChainDevice", "rtowSampleBatchChainAdaptiveDevice"):
            bufs = _device(rt, ctx, first)                       # in place: rows a sliced batch does not own keep what the batch before left there
            every += bufs
            if entry == "rtowSampleBatchChainDevice":
                rc = rt.sample_batch_chain_device(ctx, plist, bufs, bufs, diags)
            else:
                ext_out = rt.DeviceBuffer(ctx).upload(np.full((count, 2), SENTINEL, f32))
                every.append(ext_out)
                rc = rt.sample_batch_chain_adaptive_device(ctx, plist, bufs, bufs, ext_out, lag=2, diags=diags)
            ctx.synchronize()
            got = _download(bufs, n)
            got_diags = [d.download(f32, s.shape) for d, s in zip(diags, diag_start)]
            if expect == 0 and rc == 0:
                if entry == "rtowSampleBatchChainDevice":
                    want, want_diags = _oracle_chain(ref, plist, first)
                else:
                    want, want_diags, want_ext = _oracle_adaptive(rt, ref, plist, first, lag=2)
                    ext = ext_out.download(f32, (count, 2))
                    if not np.array_equal(ext.view(np.uint32), want_ext.view(np.uint32)):
                        bad.append(("extremaOut", ext.tolist(), want_ext.tolist()))
                bad += differences(got, want)
                check_diags(got_diags, want_diags, [_owned(p, n) for p in plist])
            elif rc == expect:
                bad += [("refused, but written:",) + d for d in differences(got, first)]
                bad += [("refused, but diagnostics of batch %d written" % b,) for b in range(count) if not np.array_equal(got_diags[b], diag_start[b])]
                if entry == "rtowSampleBatchChainAdaptiveDevice" and not (ext_out.download(f32, (count, 2)) == SENTINEL).all():
                    bad.append(("refused, but extremaOut written",))
            return rc, expect, bad

        ins = _device(rt, ctx, first)
        every += ins
        if entry == "rtowSampleBatchGroupDevice":
            outs = [_device(rt, ctx, _sentinels(n)) for _ in plist]
            every += [b for o in outs for b in o]
            rc = rt.sample_batch_group_device(ctx, plist, ins, outs, diags)
            ctx.synchronize()
            got_diags = [d.download(f32, s.shape) for d, s in zip(diags, diag_start)]
            assert expect == 0
            if rc == 0:
                for b, p in enumerate(plist):                 # each alone from the inputs; a batch writes the rows of its slice inside its frame and nothing else
                    alone, alone_diags = _oracle_chain(ref, [p], first)
                    own = _owned(p, n)
                    got = _download(outs[b], n)
                    want = {k: np.where(own[:, None], alone[k], SENTINEL) for k in KEYS}
                    bad += [("batch %d" % b,) + d for d in differences(got, want)]
                    bad += [("batch %d" % b,) + d for d in record_differences(got_diags[b], alone_diags[0], rows=own[:got_diags[b].shape[0]])]
            return rc, expect, bad

        assert entry == "rtowSamplePixelsDevice"
        outs = _device(rt, ctx, _sentinels(n))
        lst = rt.DeviceBuffer(ctx).upload(listed_words)
        every += outs + [lst]
        capacity = listed_words.size - 4
        rc = rt.sample_pixels_device(ctx, plist, lst, capacity, ins, outs, diags)
        ctx.synchronize()
        got = _download(outs, n)
        got_diags = [d.download(f32, s.shape) for d, s in zip(diags, diag_start)]
        if expect == 0 and rc == 0:
            want, want_diags = _oracle_chain(ref, plist, first)
            sel = np.zeros(n, bool)
            sel[listed_words[4:4 + int(listed_words[0])].astype(np.int64)] = True
            bad += differences(got, {k: np.where(sel[:, None], want[k], SENTINEL) for k in KEYS})
            for b in range(count):
                bad += [("batch %d" % b,) + d for d in record_differences(got_diags[b], want_diags[b], rows=sel)]
                if not (got_diags[b][~sel] == SENTINEL).all():
                    bad.append(("diagnostics of batch %d written at an unlisted pixel" % b,))
        elif rc == expect:
            bad += [("refused, but written:",) + d for d in differences(got, _sentinels(n))]
            bad += [("refused, but diagnostics of batch %d written" % b,) for b in range(count) if not np.array_equal(got_diags[b], diag_start[b])]
        return rc, expect, bad
    finally:
        for b in every:
            b.free()


def _oracle_adaptive(rt, ref, plist, first, lag):
    """rtowSampleBatchChainAdaptiveDevice as include/rtow.h defines it: batch k >= lag reads the extrema the frame had after batch k - lag (min and max over the whole frame
    of scw / (float) (int) color.w, a NaN weight skipped), the first `lag` batches their own"""
    acc = {k: np.array(first[k], f32, copy=True) for k in KEYS}
    ext, diags = [], []
    for k, p in enumerate(plist):
        q = L.copy_params(p)
        if k >= lag:
            q.sampleCountWeightExtrema = rt.abi.Float2(float(ext[k - lag][0]), float(ext[k - lag][1]))
        r = ref.batch(q, acc)
        acc = {key: r[key] for key in KEYS}
        diags.append(r["diag"])
        with np.errstate(divide="ignore", invalid="ignore"):
            wgt = acc["scw"].reshape(-1) / acc["color"].reshape(-1, 4)[:, 3].astype(np.int32).astype(f32)
        live = wgt[~np.isnan(wgt)]
        ext.append((f32(live.min()) if live.size else f32(np.inf), f32(live.max()) if live.size else f32(-np.inf)))
    return {k: acc[k].reshape(-1, c) for k, c in zip(KEYS, COMPS)}, diags, np.array(ext, f32)


@pytest.mark.parametrize("entry", L.ENTRY_POINTS)
def test_the_same_changes_inside_one_call(rt, oracle, entry):
    """[P0, m(P0), P0] as the batches of one call, for every mutation, on one context of the cover scene.  Where include/rtow.h and the entry point's per-batch check refuse
    the combination (launch_sequences.expected_status: one staging set, one list and one frame, one reduction) the call returns that code and every output keeps its
    sentinel; everywhere else the result is the oracle's batches, one after the other for a chain and each alone for a group.  The fractional sizes are accepted by the host
    chain and the pixel-list call - batches of one integer frame - and each batch gets the lists of its own Size."""
    ref = reference(rt, oracle, "cover")
    w, h = _frame("cover")
    P = L.base_params(ref.scene, w, h)
    words = pixel_lists.build_pixel_list(w, h, w * h, mask=_checkerboard(w, h))
    bad, verdicts = [], {}
    with rt.Context(0) as ctx:
        ref.prepare(ctx)
        for m in L.MUTATIONS:
            p0 = m.base(P, ref.scene)
            rc, expect, found = _run_entry(rt, ctx, ref, entry, [p0, m.apply(p0, ref.scene), p0], words)
            verdicts[m.name] = rc
            if rc != expect:
                bad.append((m.name, "returned", rc, "expected", expect))
            bad += [(m.name,) + d for d in found]
    print(entry, "refused:", sorted(k for k, v in verdicts.items() if v != 0))
    assert not bad, bad


# ================================================================== order, cost map and ticket map live ==================================================================
HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63      # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)


def _cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count where this process has torch's device runtime up; otherwise the same number from the HIP runtime the
    product library has loaded (torch cannot initialise its own once that library is in the process: bench.py imports torch first for that reason, a test cannot)"""
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    hip = C.CDLL("libamdhip64.so")
    value = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(value), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, 0) == 0
    assert 1 <= value.value <= 4096, value.value
    return value.value


def _order_frame():
    cus = _cu_count()
    # at least 4 * CUs chunks of 64 owned pixels also at 510 wide, the height a multiple of 16
    height = -(-(4 * cus * 64) // 510)
    height = -(-height // 16) * 16
    return cus, height


def _order_steps(rt, ref, height):
    """(label, block or list of blocks for a host chain) in the order they are rendered"""
    a = rt.abi
    S = rt.scenes

    def make(w=512, size=None, **kw):
        p = S.make_params(ref.scene, w, height, spp=2, trace_depth=4, seed=5, **kw)
        if size is not None:
            p.size = a.Float2(*size)
        return p

    wide = make()
    # 2 .. 64 samples with extrema no finite weight reaches: the quarter of the pixels whose inputs hold no sample yet (weight +inf) take 64, all others 2
    many = make(spp_max=64, extrema=(1e30, 2e30))
    return [("512 wide", wide), ("2 .. 64 samples: past kTuneMinSamplesPerPixel", many), ("510 wide: no ticket tiles", make(510)), ("512 wide again", wide), ("slice 1/2: the order is not wanted", make(slice_offset=1, slice_divider=2)),
            ("slice 0/1", wide), ("rngPolicy 1", make(rng_policy=a.RNG_PER_SAMPLE)), ("rngPolicy 0", wide), ("stride 16", make(diagnostics_stride=16)), ("stride 4", wide),
            ("Size (512.9, H + 0.9)", make(size=(float(f32(512.9)), float(f32(height + 0.9))))), ("a chain of three", [_seeded(wide, s) for s in (5, 6, 7)])]


def test_order_cost_map_and_ticket_map_live(rt, oracle):
    """A frame of at least 4 * CUs chunks of 64 owned pixels (512 x 144 for 256 CUs; the height follows the device's CU count) - where the launches run their chunks in the
    recorded order, with the pixel cost map and the ticket map - on one context of the cover scene, 2 samples at depth 4, each frame against the oracle in turn: 512 wide,
    510 wide (no multiple of kTileW = 8: no ticket tiles), 512 again, slice 1/2 (half the chunks: no order), slice 0/1, rngPolicy 1, rngPolicy 0, stride 16, stride 4,
    Size (512.9, H + 0.9), a chain of three.  A scheduling table that is not a permutation leaves pixels untouched or written twice: the random inputs show both.
    After the first frame one launch of 2 .. 64 samples takes the context past kTuneMinSamplesPerPixel (64 samples per pixel since the upload) with an order on hand: the
    threshold probes are enqueued in front of the next such launch, and the frames after it run behind them and, once a later call has read them, with the thresholds they
    chose.  When that happens is timing: thresholdSet is read and printed, not asserted."""
    cus, height = _order_frame()
    print("%d CUs: 512 x %d" % (cus, height))
    if height > 512:
        pytest.skip("%d CUs: 4 * CUs chunks of 64 pixels need a frame beyond 512 x 512" % cus)
    ref = reference(rt, oracle, "cover")
    bad = []
    with rt.Context(0) as ctx:
        ref.prepare(ctx)
        for label, p in _order_steps(rt, ref, height):
            if isinstance(p, list):
                w, h = L.frame_size(p[0])
                want, want_diags = _oracle_chain(ref, p, start(w * h))
                got = rt.sample_batch_chain_host(ctx, p, start(w * h))
                found = differences(got, want)
                for b in range(len(p)):
                    found += record_differences(got["diag"][b], want_diags[b])
            else:
                found = _single(rt, ctx, ref, p)
            bad += [(label,) + d for d in found]
        print("thresholdSet after the sequence:", int(ctx.scene_info().thresholdSet))
    assert not bad, bad


# ================================================================== across uploads ==================================================================
def test_across_uploads(rt, oracle):
    """One context, one parameter block whose view bits never change: the cover scene, then a triangle mesh, then fog, then the cover scene again - each frame against the
    oracle of the scene then uploaded (lists, order and plans of the scene before must not survive the upload).  Then, under a cubemap sky and blue noise with identical
    params: another cubemap and another blue set give the oracle's frame with the new data; without a blue set the same launch is RTOW_ERROR_INVALID_VALUE and stores
    nothing."""
    a, S = rt.abi, rt.scenes
    w, h = _frame("cover")
    n = w * h
    cover = _make_scene(rt, "cover")
    P = L.base_params(cover, w, h)
    bad = []
    with rt.Context(0) as ctx:
        for name in ("cover", "mesh", "volume", "cover"):
            scene = _make_scene(rt, name)
            scene.camera = dict(cover.camera)
            desc = scene.desc()
            ctx.upload_scene(desc)
            osc = oracle.OracleScene(desc)
            want = osc.sample_batch(P, dict(start(n)))
            osc.close()
            got = rt.sample_batch_host(ctx, P, start(n))
            bad += [(name,) + d for d in differences(got, want) + record_differences(got["diag"], want["diag"])]
        # the cover scene is uploaded: now the data behind a cubemap sky and blue noise changes under identical params
        Q = L.copy_params(P)
        Q.environment.skyType, Q.noiseColor = a.SKY_CUBEMAP, a.NOISE_BLUE
        osc = oracle.OracleScene(cover.desc())
        for seed in (5, 6):
            textures, cube = S.NoiseTextures(row_stride=8, count=3, seed=seed + 2), S.synthetic_sky(size=8, half=True, seed=seed)
            ctx.upload_sky_cubemap(cube.desc()); ctx.upload_blue_noise(textures.blue_desc())
            osc.set_cubemap(cube.desc()); osc.set_blue_noise(textures.blue_desc())
            want = osc.sample_batch(Q, dict(start(n)))
            got = rt.sample_batch_host(ctx, Q, start(n))
            bad += [("cubemap and blue set %d" % seed,) + d for d in differences(got, want) + record_differences(got["diag"], want["diag"])]
            if seed == 6:
                assert differences(want, previous), "the two data sets give different frames"
            previous = want
        osc.close()
        ctx.upload_blue_noise(None)
        ins = {k: np.ascontiguousarray(start(n)[k]) for k in KEYS}
        out = _sentinels(n)
        diag = np.full((n, 1), SENTINEL, f32)
        job = rt.SampleBatchJob(ctx, Q)
        job.InputColor, job.InputNormal, job.InputAlbedo, job.InputSampleCountWeight = [ins[k] for k in KEYS]
        job.OutputColor, job.OutputNormal, job.OutputAlbedo, job.OutputSampleCountWeight = [out[k] for k in KEYS]
        job.OutputDiagnostics = diag
        assert job.Schedule().Complete() == a.RTOW_ERROR_INVALID_VALUE
        ctx.synchronize()
        assert not differences(out, _sentinels(n)) and (diag == SENTINEL).all(), "a refused launch stored something"
    assert not bad, bad
