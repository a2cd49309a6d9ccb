"""CPU: the numpy restatement of rtowReprojectAccumDevice (tests/reproject_reference.py) on its own - what the specification of include/rtow.h promises a
host, checked before any kernel is compared with it: an unmoved camera carries every pixel to itself, a sideways step shifts by whole columns, occluders and
other entities are rejected, points behind the previous camera carry nothing, and the maxHistory rule keeps the means."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_reference as rr  # noqa: E402

F = np.float32


def _history(n, w=1.0, seed=0):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0, 2, (n, 4)).astype(F)
    color[:, 3] = F(w)
    return {"color": color, "normal": rng.normal(size=(n, 3)).astype(F), "albedo": rng.uniform(0, 1, (n, 3)).astype(F), "scw": rng.uniform(0, 4, n).astype(F)}


def _random_view(rng, w, h):
    position = rng.uniform(-8, 8, 3)
    target = position + rng.normal(size=3) * 4 + np.array([0.0, 0.0, -6.0])
    return rr.make_view(tuple(position), tuple(target), w, h, vfov=float(rng.uniform(20, 70)), focus=float(rng.uniform(1, 10)))


@pytest.mark.parametrize("w,h", [(41, 29), (1920, 1080), (3840, 2160)])
def test_an_unmoved_camera_carries_every_pixel_to_itself(w, h):
    """previousView == the view, previousHits == hits, distances in [0.01, 1000] and a share of sky: outSource[i] == i for every pixel at depthTolerance 1e-3
    (the point o + t d is rounded in float32: |P - origin| differs from t by up to 4.4e-5 t, and the projection drifts by up to 0.14 pixel from the centre)."""
    rng = np.random.default_rng(w + h)
    n = w * h
    view = _random_view(rng, w, h)
    o, d = rr.pixel_centre_rays(view, w, h)
    t = np.exp(rng.uniform(np.log(0.01), np.log(1000.0), n)).astype(F)
    e = rng.integers(0, 500, n).astype(np.int32)
    sky = rng.random(n) < 0.25
    t[sky], e[sky] = np.inf, -1
    out, src = rr.reproject(w, h, rr.view_arrays(view), o, d, t, e, t, e, _history(n), 1e-3, 64, rr.MATCH_ENTITY)
    off = np.flatnonzero(src != np.arange(n))
    assert off.size == 0, (off.size, off[:5], src[off[:5]])
    assert np.array_equal(out["color"].view(np.uint32), _history(n)["color"].view(np.uint32))


def _plane_hits(o, d, plane_z):
    return ((F(plane_z) - o[:, 2]) / d[:, 2]).astype(F)


def test_a_sideways_step_over_a_facing_plane_shifts_by_whole_columns():
    w, h, k, depth, vfov = 64, 36, 5, 5.0, 40.0
    n = w * h
    a = rr.make_view((0.0, 0.0, depth), (0.0, 0.0, 0.0), w, h, vfov=vfov, focus=depth)
    va = rr.view_arrays(a)
    column = float(np.linalg.norm(va["horizontal"].astype(np.float64))) / w          # focus == depth: the image plane lies in the world plane z = 0
    step = va["right"].astype(np.float64) * (k * column)
    b = rr.make_view((float(step[0]), float(step[1]), depth + float(step[2])), (float(step[0]), float(step[1]), float(step[2])), w, h, vfov=vfov, focus=depth)
    oa, da = rr.pixel_centre_rays(a, w, h)
    ob, db = rr.pixel_centre_rays(b, w, h)
    zeros = np.zeros(n, np.int32)
    _, src = rr.reproject(w, h, va, ob, db, _plane_hits(ob, db, 0.0), zeros, _plane_hits(oa, da, 0.0), zeros, _history(n), 0.01, 64, rr.MATCH_ENTITY)
    src = src.reshape(h, w)
    cols = np.arange(w)[None, :] + np.zeros((h, 1), np.int64)
    want = np.where(cols + k < w, np.arange(n).reshape(h, w) + k, -1)                # the new pixel (col, row) sees what (col + k, row) saw; k columns enter the frame
    assert np.array_equal(src, want), (src[0], want[0])
    assert (src[:, w - k:] == -1).all() and (src[:, : w - k] >= 0).all()


def _still(w=48, h=30, seed=3):
    rng = np.random.default_rng(seed)
    view = _random_view(rng, w, h)
    o, d = rr.pixel_centre_rays(view, w, h)
    n = w * h
    t = rng.uniform(1, 50, n).astype(F)
    e = rng.integers(0, 9, n).astype(np.int32)
    return w, h, n, rr.view_arrays(view), o, d, t, e, rng


def test_occluders_reject_by_depth_and_other_entities_only_when_matching():
    w, h, n, pv, o, d, t, e, rng = _still()
    nearer = rng.random(n) < 0.3
    other = ~nearer & (rng.random(n) < 0.3)
    pt = np.where(nearer, t * F(0.5), t).astype(F)                                  # something stood in front of the point in the previous view
    pe = np.where(other, e + 1, e).astype(np.int32)                                 # the same depth, another entity
    for flags in (0, rr.MATCH_ENTITY):
        _, src = rr.reproject(w, h, pv, o, d, t, e, pt, pe, _history(n), 0.01, 64, flags)
        assert (src[nearer] == -1).all()
        assert (src[other] == (-1 if flags else np.arange(n)[other])).all()
        assert np.array_equal(src[~nearer & ~other], np.arange(n)[~nearer & ~other])
    sky_now, sky_then = np.full(n, -1, np.int32), np.where(nearer, 0, -1).astype(np.int32)
    _, src = rr.reproject(w, h, pv, o, d, np.full(n, np.inf, F), sky_now, t, sky_then, _history(n), 0.01, 64, rr.MATCH_ENTITY)
    assert (src[nearer] == -1).all() and np.array_equal(src[~nearer], np.arange(n)[~nearer])      # sky carries sky only


def test_points_behind_the_previous_camera_carry_nothing():
    w, h, n, pv, o, d, t, e, rng = _still()
    behind = rng.random(n) < 0.5
    t2 = np.where(behind, -t, t).astype(F)                                          # o + t d on the far side of the (unmoved) camera: s < 0
    _, src = rr.reproject(w, h, pv, o, d, t2, e, t, e, _history(n), 1.0, 64, 0)
    assert (src[behind] == -1).all() and np.array_equal(src[~behind], np.arange(n)[~behind])
    on_plane = np.zeros(n, F)                                                       # t = 0: P is the camera itself, s == 0 is not > 0
    _, src = rr.reproject(w, h, pv, o, d, on_plane, e, on_plane, e, _history(n), 1.0, 64, 0)
    assert (src == -1).all()


def test_the_max_history_rule():
    w, h, n, pv, o, d, t, e, rng = _still()
    cap = 64
    prev = _history(n)
    weights = np.array([1, 2, 63, 64, 65, 100, 1000, 1e6], F)
    prev["color"][:, 3] = weights[rng.integers(0, weights.size, n)]
    prev["color"][:, :3] *= prev["color"][:, 3:4]                                   # sums over w samples
    out, src = rr.reproject(w, h, pv, o, d, t, e, t, e, prev, 0.01, cap, rr.MATCH_ENTITY)
    assert np.array_equal(src, np.arange(n))
    over = prev["color"][:, 3] > cap
    assert over.any() and (~over).any()
    for k in prev:                                                                  # w <= cap: all 11 floats bit for bit
        assert np.array_equal(out[k][~over].view(np.uint32), prev[k][~over].view(np.uint32)), k
    assert (out["color"][over, 3].view(np.uint32) == np.array(cap, F).view(np.uint32)).all()       # w becomes the cap exactly
    pw, ow = prev["color"][over, 3].astype(np.float64), float(cap)
    for k, x, y in (("color", prev["color"][over, :3], out["color"][over, :3]), ("normal", prev["normal"][over], out["normal"][over]),
                    ("albedo", prev["albedo"][over], out["albedo"][over]), ("scw", prev["scw"][over, None], out["scw"][over, None])):
        before, after = x.astype(np.float64) / pw[:, None], y.astype(np.float64) / ow
        # two float32 roundings (k = cap / w, then x * k), half an ulp each: the mean moves by at most one ulp (2^-23 relative)
        assert (np.abs(after - before) <= np.abs(before) * 2.0 ** -23).all(), k


def test_unusable_history_is_not_carried():
    w, h, n, pv, o, d, t, e, rng = _still()
    prev = _history(n, w=8.0)
    kind = rng.integers(0, 8, n)
    for k, (channel, value) in enumerate(((0, np.nan), (1, np.inf), (2, -np.inf), (3, np.nan), (3, np.inf))):
        prev["color"][kind == k, channel] = value
    prev["color"][kind == 5, 3] = 0.5
    prev["color"][kind == 6, 3] = 0.0
    out, src = rr.reproject(w, h, pv, o, d, t, e, t, e, prev, 0.01, 64, rr.MATCH_ENTITY)
    bad = kind <= 6
    assert (src[bad] == -1).all() and np.array_equal(src[~bad], np.arange(n)[~bad])
    for k in prev:
        assert (out[k][bad].view(np.uint32) == 0).all(), k                          # +0, all 11 floats
        assert np.array_equal(out[k][~bad].view(np.uint32), prev[k][~bad].view(np.uint32)), k
    prev["normal"][:, 0] = np.nan                                                   # only the colour's four channels decide
    _, src = rr.reproject(w, h, pv, o, d, t, e, t, e, prev, 0.01, 64, rr.MATCH_ENTITY)
    assert np.array_equal(src[~bad], np.arange(n)[~bad])
