"""CPU: tests/shade_hits_reference.py - the numpy restatement of rtowShadeHitsDevice that the GPU tests hold the kernel to - anchored without a GPU against the
oracle's sample path.  A 48 x 32 frame of the cover scene and one of the textured scene, each at its own camera: first-hit entities from the oracle's
Raytracer.HitWorld on the view formula's rays, and the same frame rendered by the oracle's SampleBatchJob with 1 sample per pixel, SubPixelJitter off, LensRadius 0,
white noise and trace depth 1 (the setting of tests/test_gpu_trace_rays.py's comparison of the view form with the sample path's first hit).  On every comparable pixel
(shade_hits_reference.comparable: misses, and Standard first hits that are not perfectly specular and have a constant glossiness of exactly 0) the oracle's albedo AOV
equals the restatement's emission + albedo (albedo alone on a miss) as uint32 words.  At most half of a frame's pixels may be left out as not comparable."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shade_hits_reference as ref  # noqa: E402

W, H = 48, 32


def frame(rt, oracle, name, w, h):
    """(scene, desc, params, rays, first-hit entity per pixel) of one of the two frames; the GPU test imports this too"""
    scene = {"cover": rt.scenes.cover_scene, "textured": rt.scenes.textured_scene}[name]()
    desc = scene.desc()
    p = rt.scenes.make_params(scene, w, h, spp=1, trace_depth=1, jitter=False, noise_color=rt.abi.NOISE_WHITE)
    p.view.lensRadius = 0.0
    rays = ref.view_rays(p.view, w, h)
    osc = oracle.OracleScene(desc)
    try:
        ent = np.full(w * h, -1, np.int32)
        for k in range(w * h):
            hit, rec = osc.hit_world(rays["origin"][k], rays["direction"][k], 0.0)
            if hit:
                ent[k] = int(rec[7])
        sample = osc.sample_batch(p)
    finally:
        osc.close()
    return scene, desc, p, rays, ent, sample


@pytest.mark.parametrize("name", ["cover", "textured"])
def test_the_restatement_equals_the_oracles_albedo_aov_on_comparable_pixels(rt, oracle, name):
    scene, desc, p, rays, ent, sample = frame(rt, oracle, name, W, H)
    # the rays are the oracle's own camera rays (View.GetRay at the pixel centre, no lens): the restatement's view formula, bit for bit
    out, state = (C.c_float * 8)(), C.c_uint32(1)
    for k in (0, W - 1, W * H // 2 + 7, W * H - 1):
        u, v = (np.float32(k % W) + np.float32(0.5)) / np.float32(W), (np.float32(k // W) + np.float32(0.5)) / np.float32(H)
        oracle.load().oracle_kat_get_ray(C.byref(p.view), float(u), float(v), C.byref(state), out)
        assert np.array_equal(np.asarray(list(out)[3:6], np.float32).view(np.uint32), rays["direction"][k].view(np.uint32)), (name, k)
        assert np.array_equal(np.asarray(list(out)[0:3], np.float32).view(np.uint32), rays["origin"][k].view(np.uint32)), (name, k)
    got = ref.surface(oracle, scene, desc, rays, ent, p.environment)
    keep = ref.comparable(scene, ent)
    hits, misses = int((ent >= 0).sum()), int((ent < 0).sum())
    print("%s: %d hits, %d misses, %d of %d pixels comparable" % (name, hits, misses, keep.sum(), W * H))
    assert hits > 0 and misses > 0, name
    assert 2 * int((~keep).sum()) <= W * H, (name, int(keep.sum()))                     # the cap: a condition of the comparison, not a measurement
    want = ref.expected_albedo_aov(got, ent)
    have = (np.float32(0) + sample["albedo"]).astype(np.float32)                        # -0 and +0 of a fallback store read alike: what the accumulator's 0 + x does
    bad = ~ref.same_bits(have, want).all(axis=1) & keep
    assert not bad.any(), (name, np.flatnonzero(bad)[:8], have[bad][:4], want[bad][:4])
    assert (keep & (ent >= 0)).sum() > W * H // 8 and np.any(want[keep & (ent >= 0)] != 0), name
    if name == "textured":                                                               # texture coordinates and texels took part
        tex = keep & (ent >= 0) & np.any(got["texCoord"] != 0, axis=1)
        assert tex.sum() > W * H // 8 and len(np.unique(got["albedo"][tex], axis=0)) > 8, (name, int(tex.sum()))


def test_conversions_and_nan_equality_of_the_restatement():
    x = np.asarray([0.0, 0.99, -0.99, 5.7, -5.7, 3e9, -3e9, np.inf, -np.inf, np.nan], np.float32)
    assert ref.to_int(x).tolist() == [0, 0, 0, 5, -5, 2147483647, -2147483648, 2147483647, -2147483648, 0]
    a = np.asarray([np.nan, 1.0, 0.0], np.float32)
    b = np.asarray([-np.nan, 1.0, -0.0], np.float32)
    assert ref.same_bits(a, b).tolist() == [True, True, False]
    assert ref.same_bits(np.asarray([1, -1], np.int32), np.asarray([1, -2], np.int32)).tolist() == [True, False]
