"""GPU: rtowRecordPathsDevice - one sample of a pixel replayed segment by segment - held to the sample kernel and to rtowTraceRaysDevice, with no reference in the loop.

The recorded sample is what rtowSampleBatchDevice adds for that pixel (colour, AOVs, success, ray count: bit for bit, one sample and every sample of six, fixed and
adaptive counts, failed samples, three noise sources); every recorded segment is one ray of rtowTraceRaysDevice (distance, entity, normal: bit for bit) and the
segments chain by the header's float32 expressions; the brightest sample is the one the six indexed calls rank first; the launch's edges are walked between guard
words; refusals touch nothing.  Frames are a few thousand pixels; what the GPU computed for a frame is computed once per module and shared.  One GPU context at a
time."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guides_reference as guides  # noqa: E402  (mirror_scene)
from test_gpu_shade_hits import GUARD, _Guarded  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SCENES = ["cover", "tiny", "mixed", "textured", "mesh", "mirrors"]
SUMMARY_WORDS, SEGMENT_WORDS = 17, 24


def _rt():
    return sys.modules["rtow_amd"]


def _scene(name):
    rt = _rt()
    S = rt.scenes
    return {"cover": S.cover_scene, "tiny": S.tiny_scene, "mixed": S.mixed_scene, "textured": S.textured_scene, "mesh": lambda: S.mesh_scene(3),
            "mirrors": lambda: guides.mirror_scene(rt), "volumes": S.volume_scene}[name]()


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _event(info):
    a = _rt().abi
    return (info >> a.PATH_INFO_EVENT_SHIFT) & a.PATH_INFO_EVENT_MASK


def _zeros(n):
    return {"color": np.zeros((n, 4), f32), "normal": np.zeros((n, 3), f32), "albedo": np.zeros((n, 3), f32), "scw": np.zeros(n, f32)}


def _check_against_batch(p, ins, out, summaries, what):
    """One recorded sample per pixel against a batch that took exactly one sample per pixel from `ins`: a sample that succeeded is added to the accumulators (in + s in
    float32), a failed one leaves the colour and stores its AOVs as they are where no sample has succeeded before (the fallback)."""
    a = _rt().abi
    ok = (summaries["flags"] & a.PATH_FLAG_SUCCEEDED) != 0
    assert np.array_equal(summaries["flags"] & ~np.uint32(a.PATH_FLAG_SUCCEEDED), np.zeros_like(summaries["flags"])), what
    assert np.array_equal(ok, out["color"][:, 3] == ins["color"][:, 3] + 1), what
    assert np.array_equal(summaries["sampleCount"], np.ones_like(summaries["sampleCount"])), what
    for key in ("color", "normal", "albedo"):
        added = (ins[key][:, :3] + summaries[key]).astype(f32)
        stored = summaries[key] if key != "color" else ins[key][:, :3]
        want = np.where(ok[:, None], added, stored)
        bad = (_bits(out[key][:, :3]) != _bits(want)).any(axis=1)
        assert not bad.any(), (what, key, np.flatnonzero(bad)[:8], out[key][bad][:3], want[bad][:3])
    assert not _bits(summaries["color"][~ok]).any(), what                                    # a failed sample's colour is +0
    assert np.array_equal(summaries["segmentCount"].astype(f32), out["diag"][:, 0]), what   # RayCount
    assert np.array_equal(summaries["segmentCount"][~ok], np.full(int((~ok).sum()), int(p.traceDepth), np.int32)), what
    assert np.array_equal(_bits(summaries["luminance"]), _bits(_luminance(summaries["color"]))), what
    assert np.array_equal(summaries["pixel"], np.arange(len(summaries), dtype=np.int32)), what


def _luminance(c):
    c = np.asarray(c, f32)
    return ((f32(0.2126) * c[..., 0] + f32(0.7152) * c[..., 1]).astype(f32) + f32(0.0722) * c[..., 2]).astype(f32)


@functools.lru_cache(maxsize=None)
def _one_sample_frame(name, depth=9):
    """case 1 (and 4, 5): a 61 x 37 frame (not a multiple of the 8 x 8 tile), every pixel listed, zeroed accumulators, one sample, jitter on, white noise: the batch, the
    records, and rtowTraceRaysDevice on every recorded segment's (from, time, direction)."""
    rt = _rt()
    w, h = 61, 37
    n = w * h
    scene = _scene(name)
    p = rt.scenes.make_params(scene, w, h, spp=1, trace_depth=depth, jitter=True, noise_color=rt.abi.NOISE_WHITE)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        out = rt.sample_batch_host(ctx, p)
        summaries, segments = ctx.record_paths(p, np.arange(n))
        rays = np.zeros((n, depth), np.dtype(rt.abi.RAY_DTYPE))
        rays["origin"], rays["direction"] = segments["from"], segments["direction"]
        rays["time"] = summaries["time"][:, None]
        traced = ctx.trace_rays(rays.reshape(-1))
    return p, out, summaries, segments, {k: v.reshape((n, depth) + v.shape[1:]) for k, v in traced.items()}


@pytest.mark.parametrize("name", SCENES)
def test_one_sample_equals_the_batch(name):
    """1. colour, normal and albedo as uint32 words equal what rtowSampleBatchDevice stores from zeroed accumulators, flags bit 0 equals color.w == 1, segmentCount equals
    the diagnostics' RayCount - on every pixel of six scenes.  Not vacuous: sky ends, surface ends and all six events on `cover`, REFLECT on `tiny`."""
    a = _rt().abi
    p, out, summaries, segments, _ = _one_sample_frame(name)
    n = len(summaries)
    _check_against_batch(p, _zeros(n), out, summaries, name)
    counts = summaries["segmentCount"]
    last = segments[np.arange(n), counts - 1]
    events = _event(segments["info"])[np.arange(p.traceDepth)[None, :] < counts[:, None]]
    seen = {int(e): int((events == e).sum()) for e in a.PATH_EVENTS}
    print(name, "events", seen, "failed", int((last["entityIndex"] >= 0).sum()), "rays", int(counts.sum()))
    if name == "cover":
        assert (last["entityIndex"] < 0).any() and (last["entityIndex"] >= 0).any(), "sky ends and surface ends"
        assert all(seen[e] > 0 for e in a.PATH_EVENTS), seen
    if name == "tiny":
        assert seen[a.PATH_REFLECT] > 0, seen


@pytest.mark.parametrize("name", SCENES)
def test_segments_against_the_trace_call(name):
    """5. every recorded surface segment: rtowTraceRaysDevice on (from, summary.time, direction) returns distance, entityIndex and normal bit for bit; a sky segment is a
    miss and to == direction * 99999; to == P = from + distance * direction; the next from == P + 0.001f * (dot(next.direction, N) >= 0 ? N : -N); GLOSSY and REFLECT
    attenuate by exactly (1, 1, 1); the numpy fold tail -> head of the recorded attenuation and emission is summary.color; slots beyond segmentCount are zero."""
    a = _rt().abi
    p, out, summaries, segments, traced = _one_sample_frame(name)
    n, depth = segments.shape
    counts = summaries["segmentCount"]
    used = np.arange(depth)[None, :] < counts[:, None]
    ok = (summaries["flags"] & a.PATH_FLAG_SUCCEEDED) != 0
    sky = used & (segments["entityIndex"] < 0)
    surface = used & ~sky
    assert np.array_equal(sky.sum(axis=1), ok.astype(np.int64)) and np.array_equal(sky[np.arange(n), counts - 1], ok), name     # the sky ends a path, and only a successful one
    assert not segments[~used].view(np.uint32).any(), name
    # the trace call on the same ray
    assert np.array_equal(_bits(traced["distance"][used]), _bits(segments["distance"][used])), name
    assert np.array_equal(traced["entityIndex"][used], segments["entityIndex"][used]), name
    assert np.array_equal(_bits(traced["normal"][used]), _bits(segments["normal"][used])), name
    assert np.all(np.isposinf(segments["distance"][sky])) and not _bits(segments["normal"][sky]).any(), name
    assert np.array_equal(_bits(segments["to"][sky]), _bits((segments["direction"][sky] * f32(a.PATH_SKY_REACH)).astype(f32))), name
    info = segments["info"]
    assert np.all((info[sky] & a.PATH_INFO_MATERIAL_MASK) == 0xFFFF) and np.all(_event(info[sky]) == a.PATH_SKY) and np.all(_event(info[surface]) != a.PATH_SKY), name
    assert not _bits(segments["pad0"]).any() and not _bits(segments["pad1"]).any(), name
    # chaining
    point = (segments["from"] + (segments["distance"][..., None] * segments["direction"]).astype(f32)).astype(f32)
    assert np.array_equal(_bits(segments["to"][surface]), _bits(point[surface])), name
    nxt = segments[:, 1:]
    link = used[:, 1:]                                    # segment d + 1 exists: segment d is a surface
    normal = segments["normal"][:, :-1]
    d = nxt["direction"]
    dot = ((d[..., 0] * normal[..., 0] + d[..., 1] * normal[..., 1]).astype(f32) + d[..., 2] * normal[..., 2]).astype(f32)
    toward = np.where((dot >= 0)[..., None], normal, -normal).astype(f32)
    origin = (point[:, :-1] + (f32(0.001) * toward).astype(f32)).astype(f32)
    assert np.array_equal(_bits(nxt["from"][link]), _bits(origin[link])), name
    white = surface & np.isin(_event(info), (a.PATH_GLOSSY, a.PATH_REFLECT))
    assert np.array_equal(_bits(segments["attenuation"][white]), _bits(np.ones((int(white.sum()), 3), f32))), name
    assert np.array_equal(_bits(segments["attenuation"][sky]), _bits(np.ones((int(sky.sum()), 3), f32))), name
    # the fold, tail -> head: c = c * a + e in two roundings
    c = np.zeros((n, 3), f32)
    for k in range(depth - 1, -1, -1):
        step = ((c * segments["attenuation"][:, k]).astype(f32) + segments["emission"][:, k]).astype(f32)
        c = np.where((used[:, k] & ok)[:, None], step, c)
    assert np.array_equal(_bits(c), _bits(summaries["color"])), name
    # the material a segment names is the entity's, and IsPerfectSpecular goes with the events only such a material takes
    scene = _scene(name)
    assert np.array_equal((info[surface] & a.PATH_INFO_MATERIAL_MASK).astype(np.int64), np.asarray(scene.material_index, np.int64)[segments["entityIndex"][surface]]), name
    assert np.all((info[surface & np.isin(_event(info), (a.PATH_REFRACT, a.PATH_REFLECT))] & a.PATH_INFO_PERFECT_SPECULAR) != 0), name


@pytest.mark.parametrize("depth", [1, 2])
def test_failed_samples(depth):
    """4. traceDepth 1 and 2 on `cover`: pixels that do not reach the sky report success 0, colour +0 and segmentCount == traceDepth, and their AOVs are the batch's
    fallback AOVs."""
    a = _rt().abi
    p, out, summaries, segments, _ = _one_sample_frame("cover", depth)
    n = len(summaries)
    _check_against_batch(p, _zeros(n), out, summaries, depth)
    failed = (summaries["flags"] & a.PATH_FLAG_SUCCEEDED) == 0
    assert failed.sum() > n // 8 and (~failed).sum() > n // 8, (depth, int(failed.sum()))
    assert np.all(segments["entityIndex"][failed] >= 0) and not _bits(out["color"][failed]).any()
    assert np.array_equal(_bits(out["normal"][failed]), _bits(summaries["normal"][failed])) and np.array_equal(_bits(out["albedo"][failed]), _bits(summaries["albedo"][failed]))
    assert _bits(summaries["normal"][failed]).any(axis=1).all()                            # a surface's normal, not the default


def _accumulate(ins, records, upto=None):
    """the batch's running sums from the records of samples 0, 1, ... in order: acc += color_k where sample k exists and succeeded, in float32"""
    a = _rt().abi
    acc = {k: ins[k][:, :3].astype(f32).copy() for k in ("color", "normal", "albedo")}
    count = ins["color"][:, 3].astype(f32).copy()
    rays = np.zeros(len(count), np.int64)
    for k, (s, _) in enumerate(records):
        exists = (s["flags"] & a.PATH_FLAG_NO_SUCH_SAMPLE) == 0
        ok = exists & ((s["flags"] & a.PATH_FLAG_SUCCEEDED) != 0)
        if upto is not None:
            assert np.array_equal(exists, k < upto), k
        for key in acc:
            acc[key] = np.where(ok[:, None], (acc[key] + s[key]).astype(f32), acc[key])
        count = np.where(ok, (count + f32(1)).astype(f32), count)
        rays += np.where(exists, s["segmentCount"], 0)
    return acc, count, rays


@functools.lru_cache(maxsize=None)
def _six_sample_frame(name, noise=0, w=33, h=19):
    """case 2 (and 6, 7): sampleCountRange {6, 6}; samples k = 0 .. 6 recorded in seven calls (k = 6 does not exist), and the brightest"""
    rt = _rt()
    a = rt.abi
    n = w * h
    scene = _scene(name)
    p = rt.scenes.make_params(scene, w, h, spp=6, trace_depth=4, jitter=True, noise_color=noise, noise_texture_index=1 if noise else 0)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        if noise:
            tex = rt.scenes.NoiseTextures(row_stride=12, count=2, seed=23)                  # a row stride that is not a power of two
            ctx.upload_blue_noise(tex.blue_desc())
            ctx.upload_stb_noise(tex.stb_desc())
        out = rt.sample_batch_host(ctx, p)
        records = [ctx.record_paths(p, np.arange(n), sample_index=k) for k in range(7)]
        brightest = ctx.record_paths(p, np.arange(n), select=a.PATH_SELECT_BRIGHTEST)
    return p, out, records, brightest


def _check_six(p, out, records, what):
    a = _rt().abi
    n = len(out["scw"])
    acc, count, rays = _accumulate(_zeros(n), records[:6])
    for key in ("color", "normal", "albedo"):
        has = count > 0 if key != "color" else np.ones(n, bool)                               # (without a success the AOVs are sample 0's fallback, checked below)
        assert np.array_equal(_bits(out[key][:, :3][has]), _bits(acc[key][has])), (what, key)
    assert np.array_equal(out["color"][:, 3], count), what
    assert np.array_equal(rays.astype(f32), out["diag"][:, 0]), what
    none = count == 0
    for key in ("normal", "albedo"):
        assert np.array_equal(_bits(out[key][none]), _bits(records[0][0][key][none])), (what, key)
    for k in range(6):
        s, g = records[k]
        assert np.all(s["sampleIndex"] == k) and np.all(s["sampleCount"] == 6), (what, k)
    s, g = records[6]
    assert np.all(s["flags"] == a.PATH_FLAG_NO_SUCH_SAMPLE) and np.all(s["segmentCount"] == 0) and np.all(s["sampleCount"] == 6) and np.all(s["sampleIndex"] == 6), what
    assert not g.view(np.uint32).any(), what
    for field in ("time", "luminance", "randomEvents", "color", "normal", "albedo"):
        assert not _bits(s[field]).any(), (what, field)
    return count


@pytest.mark.parametrize("name", ["cover", "mixed"])
def test_every_sample_index(name):
    """2. sampleCountRange {6, 6}: acc = in.color.xyz, then `if success_k: acc += color_k` for k = 0 .. 5 equals out.color.xyz bit for bit (and so the AOVs), the success
    count equals out.color.w, the segment counts add up to RayCount; k = 6 gives flags bit 1 and zero segments."""
    p, out, records, _ = _six_sample_frame(name)
    count = _check_six(p, out, records, name)
    print(name, "successes per pixel", np.bincount(count.astype(int), minlength=7).tolist())
    assert (count < 6).any() and (count > 0).any(), name


@pytest.mark.parametrize("noise", [1, 2], ids=["blue", "stbn"])
def test_blue_and_spatiotemporal_blue_noise(noise):
    """7. case 2 at 17 x 9 with NoiseTextures' sets at row stride 12 and noiseTextureIndex 1"""
    p, out, records, _ = _six_sample_frame("cover", noise, 17, 9)
    _check_six(p, out, records, noise)
    white = _six_sample_frame("cover")[2][0][0]["color"]
    assert not np.array_equal(records[0][0]["color"][:40], white[:40])                          # another source, another path


@pytest.mark.parametrize("name", ["cover", "mixed"])
def test_brightest(name):
    """6. SELECT_BRIGHTEST returns the k and the records that the six SELECT_INDEX calls rank first: a NaN channel above all, then the larger luminance (a failed sample:
    +0), first among equals; a pixel whose samples all fail reports k = 0."""
    a = _rt().abi
    p, out, records, (bs, bg) = _six_sample_frame(name)
    n = len(bs)
    best = np.zeros(n, np.int64)
    best_lum = records[0][0]["luminance"].copy()
    best_nan = np.isnan(records[0][0]["color"]).any(axis=1)
    for k in range(1, 6):
        s = records[k][0]
        is_nan = np.isnan(s["color"]).any(axis=1)
        better = (is_nan & ~best_nan) | (~is_nan & ~best_nan & (s["luminance"] > best_lum))
        best = np.where(better, k, best)
        best_lum = np.where(better, s["luminance"], best_lum)
        best_nan |= is_nan
    assert np.array_equal(bs["sampleIndex"], best.astype(np.int32)), np.flatnonzero(bs["sampleIndex"] != best)[:8]
    want_s = np.stack([records[k][0] for k in range(6)])[best, np.arange(n)]
    want_g = np.stack([records[k][1] for k in range(6)])[best, np.arange(n)]
    assert np.array_equal(bs.view(np.uint32), want_s.view(np.uint32)) and np.array_equal(bg.view(np.uint32), want_g.view(np.uint32)), name
    all_fail = np.all([(records[k][0]["flags"] & a.PATH_FLAG_SUCCEEDED) == 0 for k in range(6)], axis=0)
    print(name, "brightest index", np.bincount(best, minlength=6).tolist(), "pixels without a success", int(all_fail.sum()))
    assert len(np.unique(best)) == 6, name
    if name == "mixed":                                   # (some of its pixels never reach the sky in four bounces; on `cover` every pixel of this frame does once in six)
        assert all_fail.any()
    assert np.all(bs["sampleIndex"][all_fail] == 0) and np.all(bs["flags"][all_fail] == 0)


def test_adaptive_counts():
    """3. non-zero input accumulators with weights spread over the extrema, sampleCountRange {1, 6}: summary.sampleCount is the number of samples the batch took - the
    running sum over exactly the samples k < sampleCount equals the batch - and is the header's expression of the pixel's weight."""
    rt = _rt()
    a = rt.abi
    w, h = 33, 19
    n = w * h
    scene = _scene("cover")
    lo, hi = 0.25, 1.5
    p = rt.scenes.make_params(scene, w, h, spp=1, spp_max=6, trace_depth=5, extrema=(lo, hi))
    rng = np.random.default_rng(77)
    ins = _zeros(n)
    ins["color"][:, :3] = rng.random((n, 3), dtype=f32) * 4
    ins["color"][:, 3] = rng.integers(1, 9, n).astype(f32)
    weight = (lo - 0.25 + (hi - lo + 0.5) * rng.random(n, dtype=f32)).astype(f32)              # below, between and above the extrema
    weight[::11] = 0                                                                            # w == 0: the minimum
    ins["scw"] = (weight * ins["color"][:, 3]).astype(f32)
    ins["normal"], ins["albedo"] = rng.standard_normal((n, 3)).astype(f32), rng.random((n, 3), dtype=f32)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        out = rt.sample_batch_host(ctx, p, ins)
        records = [ctx.record_paths(p, np.arange(n), ins["color"], ins["scw"], sample_index=k) for k in range(6)]
    took = records[0][0]["sampleCount"]
    for s, _ in records:
        assert np.array_equal(s["sampleCount"], took)
    wq = (ins["scw"] / ins["color"][:, 3]).astype(f32)
    nw = np.clip(((wq - f32(lo)) / (f32(hi) - f32(lo))).astype(f32), f32(0), f32(1))
    want = np.where(wq == 0, 1, np.rint((f32(1) + (nw * f32(5)).astype(f32)).astype(f32))).astype(np.int32)
    assert np.array_equal(took, want), np.flatnonzero(took != want)[:8]
    assert sorted(np.unique(took).tolist()) == [1, 2, 3, 4, 5, 6]
    acc, count, rays = _accumulate(ins, records, upto=took)
    for key in ("color", "normal", "albedo"):
        assert np.array_equal(_bits(out[key][:, :3]), _bits(acc[key])), key
    assert np.array_equal(out["color"][:, 3], count) and np.array_equal(rays.astype(f32), out["diag"][:, 0])


def _raw_call(ctx, p, words_ptr, capacity, color, scw, summaries, segments, select=0, index=0):
    rt = _rt()
    rp = rt.abi.RecordPathsParams(select, index, 0, 0)
    lst = rt.abi.PixelList(words_ptr, capacity)
    return rt.lib.load().rtowRecordPathsDevice(ctx.handle, C.byref(p), C.byref(rp), C.byref(lst), color, scw, summaries, segments, None)


def test_edges_of_the_launch():
    """8. lists of 1, 63, 64 and 65 entries; words[0] beyond the capacity; a capacity beyond words[0]; entries >= W * H (flags bit 2, never an address); capacity 0;
    outputs at odd 4-byte offsets between guard words - no guard word and no slot beyond the count changes; segments == NULL gives the same summaries."""
    rt = _rt()
    a = rt.abi
    w, h, depth = 33, 19, 6
    n = w * h
    scene = _scene("cover")
    p = rt.scenes.make_params(scene, w, h, spp=1, trace_depth=depth)
    order = np.random.default_rng(5).permutation(n).astype(np.uint32)
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        full_s, full_g = ctx.record_paths(p, order)
        color, scw = rt.DeviceBuffer(ctx, n * 16).zero(), rt.DeviceBuffer(ctx, n * 4).zero()
        for listed, capacity, stated in ((1, 1, 1), (63, 63, 63), (64, 64, 64), (65, 65, 65), (65, 65, 70), (65, 65, 0xFFFFFFFF), (61, 65, 61), (0, 65, 0), (0, 0, 9)):
            words = _Guarded(rt, ctx, 4 + max(capacity, 1), np.concatenate([np.array([stated, 0, 0, 0], np.uint32), order[:max(capacity, 1)]]))
            for with_segments in (True, False):
                sums = _Guarded(rt, ctx, max(capacity, 1) * SUMMARY_WORDS)
                segs = _Guarded(rt, ctx, max(capacity, 1) * depth * SEGMENT_WORDS)
                rt.lib.check(_raw_call(ctx, p, words.ptr, capacity, color.ptr, scw.ptr, sums.ptr, segs.ptr if with_segments else None), "rtowRecordPathsDevice")
                ctx.synchronize()
                body_s, body_g = sums.check(True), segs.check(True)
                assert np.array_equal(body_s[:listed * SUMMARY_WORDS], full_s[:listed].view(np.uint32).reshape(-1)), (listed, capacity, stated, with_segments)
                assert np.all(body_s[listed * SUMMARY_WORDS:] == GUARD), (listed, capacity, stated)
                if with_segments:
                    assert np.array_equal(body_g[:listed * depth * SEGMENT_WORDS], full_g[:listed].view(np.uint32).reshape(-1)), (listed, capacity, stated)
                    assert np.all(body_g[listed * depth * SEGMENT_WORDS:] == GUARD), (listed, capacity, stated)
                else:
                    assert np.all(body_g == GUARD)
                sums.buf.free()
                segs.buf.free()
            words.check(True)
            words.buf.free()
        # entries that are no pixel of the frame, between two that are
        entries = np.array([order[0], n, 0xFFFFFFFF, 0x80000000, order[1]], np.uint32)
        s, g = ctx.record_paths(p, entries)
        assert np.array_equal(s[[0, 4]].view(np.uint32), full_s[[0, 1]].view(np.uint32)) and np.array_equal(g[[0, 4]].view(np.uint32), full_g[[0, 1]].view(np.uint32))
        assert np.all(s["flags"][1:4] == a.PATH_FLAG_NOT_A_PIXEL) and np.array_equal(s["pixel"][1:4].view(np.uint32), entries[1:4])
        rest = s[1:4].copy()
        rest["pixel"], rest["flags"] = 0, 0
        assert not rest.view(np.uint32).any() and not g[1:4].view(np.uint32).any()
        s2, none = ctx.record_paths(p, entries, want_segments=False)
        assert none is None and np.array_equal(s2.view(np.uint32), s.view(np.uint32))
        color.free()
        scw.free()


def test_depth_64_and_a_reupload_between_two_calls():
    """8. traceDepth 64 on the mirror scene (paths between two facing mirrors) against the batch; two calls on one stream with rtowUploadScene between them, no wait:
    each records its own scene."""
    rt = _rt()
    a = rt.abi
    w, h = 33, 19
    n = w * h
    mirrors, cover = _scene("mirrors"), _scene("cover")
    p = rt.scenes.make_params(mirrors, w, h, spp=1, trace_depth=64)
    q = rt.scenes.make_params(cover, w, h, spp=1, trace_depth=7)
    pixels = np.concatenate([np.array([n, 0, 0, 0], np.uint32), np.arange(n, dtype=np.uint32)])
    with rt.Context(0) as ctx:
        ctx.upload_scene(mirrors.desc())
        out = rt.sample_batch_host(ctx, p)
        s, g = ctx.record_paths(p, np.arange(n))
        _check_against_batch(p, _zeros(n), out, s, "mirrors at depth 64")
        print("mirrors at depth 64: longest path", int(s["segmentCount"].max()), "failed", int(((s["flags"] & a.PATH_FLAG_SUCCEEDED) == 0).sum()))
        assert s["segmentCount"].max() > 8, int(s["segmentCount"].max())                    # beyond the depth every other case runs at
        ctx.upload_scene(cover.desc())
        alone = ctx.record_paths(q, np.arange(n))
        words = rt.DeviceBuffer(ctx, pixels.nbytes).upload(pixels)
        color, scw = rt.DeviceBuffer(ctx, n * 16).zero(), rt.DeviceBuffer(ctx, n * 4).zero()
        first = [rt.DeviceBuffer(ctx, n * SUMMARY_WORDS * 4), rt.DeviceBuffer(ctx, n * 64 * SEGMENT_WORDS * 4)]
        second = [rt.DeviceBuffer(ctx, n * SUMMARY_WORDS * 4), rt.DeviceBuffer(ctx, n * 7 * SEGMENT_WORDS * 4)]
        ctx.upload_scene(mirrors.desc())
        rt.lib.check(_raw_call(ctx, p, words.ptr, n, color.ptr, scw.ptr, first[0].ptr, first[1].ptr), "rtowRecordPathsDevice")
        ctx.upload_scene(cover.desc())
        rt.lib.check(_raw_call(ctx, q, words.ptr, n, color.ptr, scw.ptr, second[0].ptr, second[1].ptr), "rtowRecordPathsDevice")
        ctx.synchronize()
        assert np.array_equal(first[0].download(np.uint32, (n * SUMMARY_WORDS,)), s.view(np.uint32).reshape(-1))
        assert np.array_equal(first[1].download(np.uint32, (n * 64 * SEGMENT_WORDS,)), g.view(np.uint32).reshape(-1))
        assert np.array_equal(second[0].download(np.uint32, (n * SUMMARY_WORDS,)), alone[0].view(np.uint32).reshape(-1))
        assert np.array_equal(second[1].download(np.uint32, (n * 7 * SEGMENT_WORDS,)), alone[1].view(np.uint32).reshape(-1))
        for b in [words, color, scw] + first + second:
            b.free()


def test_refusals_touch_nothing():
    """9. a scene with a ProbabilisticVolume material and rngPolicy 1 return RTOW_ERROR_UNSUPPORTED with the outputs untouched; RTOW_ERROR_NO_SCENE before an upload; bad
    arguments are refused with a real context as without one; the calls leave rtowGetLastSampleKernelMs and the batch status of an earlier batch unchanged."""
    rt = _rt()
    a = rt.abi
    w, h, depth = 24, 16, 5
    n = w * h
    cover, volumes = _scene("cover"), _scene("volumes")
    p = rt.scenes.make_params(cover, w, h, spp=1, trace_depth=depth)
    pixels = np.concatenate([np.array([n, 0, 0, 0], np.uint32), np.arange(n, dtype=np.uint32)])
    with rt.Context(0) as ctx:
        words = rt.DeviceBuffer(ctx, pixels.nbytes).upload(pixels)
        color, scw = rt.DeviceBuffer(ctx, n * 16).zero(), rt.DeviceBuffer(ctx, n * 4).zero()
        sums, segs = _Guarded(rt, ctx, n * SUMMARY_WORDS), _Guarded(rt, ctx, n * depth * SEGMENT_WORDS)
        call = lambda params, **over: _raw_call(ctx, params, over.get("words", words.ptr), over.get("capacity", n), over.get("color", color.ptr), scw.ptr,
                                                over.get("sums", sums.ptr), over.get("segs", segs.ptr), over.get("select", 0), over.get("index", 0))
        assert call(p) == a.RTOW_ERROR_NO_SCENE
        ctx.upload_scene(volumes.desc())
        assert call(rt.scenes.make_params(volumes, w, h, spp=1, trace_depth=depth)) == a.RTOW_ERROR_UNSUPPORTED
        assert call(rt.scenes.make_params(volumes, w, h, spp=1, trace_depth=depth), segs=None) == a.RTOW_ERROR_UNSUPPORTED
        ctx.upload_scene(cover.desc())
        out = rt.sample_batch_host(ctx, p)
        ms = ctx.last_sample_kernel_ms()
        assert call(rt.scenes.make_params(cover, w, h, spp=1, trace_depth=depth, rng_policy=1)) == a.RTOW_ERROR_UNSUPPORTED
        assert call(rt.scenes.make_params(cover, w, h, spp=1, trace_depth=depth, noise_color=a.NOISE_BLUE)) == a.RTOW_ERROR_INVALID_VALUE      # no blue-noise set uploaded
        assert call(rt.scenes.make_params(cover, w, h, spp=1, trace_depth=65)) == a.RTOW_ERROR_CAPACITY
        assert call(rt.scenes.make_params(cover, w, h, spp=1, trace_depth=depth, slice_divider=2)) == a.RTOW_ERROR_INVALID_VALUE
        assert call(p, select=2) == a.RTOW_ERROR_INVALID_VALUE and call(p, select=1, index=1) == a.RTOW_ERROR_INVALID_VALUE and call(p, index=-1) == a.RTOW_ERROR_INVALID_VALUE
        assert call(p, words=None) == a.RTOW_ERROR_INVALID_VALUE and call(p, color=None) == a.RTOW_ERROR_INVALID_VALUE and call(p, sums=None) == a.RTOW_ERROR_INVALID_VALUE
        assert call(p, sums=color.ptr + 16) == a.RTOW_ERROR_INVALID_VALUE and call(p, segs=words.ptr + 4) == a.RTOW_ERROR_INVALID_VALUE
        assert call(p, segs=sums.ptr + 4 * (n * SUMMARY_WORDS - 1)) == a.RTOW_ERROR_INVALID_VALUE
        ctx.synchronize()
        sums.check(None)
        segs.check(None)
        # a good call, and one without segments (the context's own stack block): neither is a sample batch
        assert call(p) == a.RTOW_SUCCESS and call(p, segs=None) == a.RTOW_SUCCESS and call(p, capacity=0) == a.RTOW_SUCCESS
        ctx.batch_status()
        assert ctx.last_sample_kernel_ms() == ms
        s = np.frombuffer(sums.check(True).tobytes(), np.dtype(a.PATH_SUMMARY_DTYPE))
        _check_against_batch(p, _zeros(n), out, s, "after the refusals")
        for b in (words, color, scw, sums.buf, segs.buf):
            b.free()
