"""CPU: the numpy restatement of rtowReprojectAccumBilinearDevice (tests/reproject_bilinear_reference.py) against facts of its own - what the specification of
include/rtow.h promises whatever the kernel does - and the coverage of the generated cases the GPU test runs (tests/reproject_bilinear_cases.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reproject_bilinear_cases as bc  # noqa: E402
import reproject_bilinear_reference as rb  # noqa: E402
import reproject_reference as rr  # noqa: E402

F = np.float32
W, H = 48, 32


def _sky_pair(seed, w=W, h=H):
    """two views a small step apart and an all-sky frame in both: every tap inside the image passes step 3, so the accumulators alone decide"""
    rng = np.random.default_rng(seed)
    a = rr.make_view((0.3, 1.2, 6.0), (0.0, 0.5, 0.0), w, h)
    b = rr.make_view((0.35, 1.25, 5.9), (0.02, 0.5, 0.0), w, h)
    o, d = rr.pixel_centre_rays(b, w, h)
    n = w * h
    sky_t, sky_e = np.full(n, np.inf, F), np.full(n, -1, np.int32)
    return rng, rr.view_arrays(a), o, d, sky_t, sky_e


def _accumulators(mean, count, rng):
    """sums of `count` samples whose mean is `mean` (n, 3) in every buffer"""
    n = count.size
    c = count.astype(F)
    return {"color": np.concatenate([mean * c[:, None], c[:, None]], axis=1).astype(F), "normal": (mean * c[:, None]).astype(F),
            "albedo": (mean * c[:, None]).astype(F), "scw": (mean[:, 0] * c).astype(F)}


def _run(va, o, d, t, e, prev, max_history=1000, tol=0.01, flags=1, moments=None, max_batches=None, w=W, h=H):
    return rb.reproject_bilinear(w, h, va, o, d, t, e, t, e, prev, tol, max_history, flags, moments, max_batches)


def test_the_restated_steps_are_those_of_the_nearest_restatement(rt):
    """project(), the nearest tap and matches() give reproject_reference.source_pixels, for every configuration"""
    for k, cfg in enumerate(bc.CONFIGS):
        flags, tol, mh = cfg
        case = bc.make_bilinear_case(41, 29, bc.seed_of(41, 29, k), mh, 16)
        w, h = case["w"], case["h"]
        inside, fx, fy, r = rb.project(w, h, case["va"], case["o"], case["d"], case["t"], case["e"])
        q = np.where(inside, np.where(inside, fy, 0).astype(np.int64) * w + np.where(inside, fx, 0).astype(np.int64), 0)
        ok = inside & rb.matches(q, case["e"], r, case["pt"], case["pe"], tol, flags)
        want = rr.source_pixels(w, h, case["va"], case["o"], case["d"], case["t"], case["e"], case["pt"], case["pe"], tol, flags)
        assert np.array_equal(np.where(ok, q, -1), want), cfg


def test_a_constant_mean_comes_back_whatever_the_counts_and_the_valid_taps(rt):
    """About ten float32 roundings of 2^-24 each lie between the mean and the output divided by its count: 1e-6 relative."""
    rng, va, o, d, t, e = _sky_pair(1)
    n = W * H
    mean = np.broadcast_to(np.array([0.7, 1.9, 0.31], F), (n, 3))
    count = rng.integers(1, 50, n)
    count[rng.random(n) < 0.3] = 0                                       # unusable taps: any set of valid taps occurs
    out, src, _, valid = _run(va, o, d, t, e, _accumulators(mean, count, rng))
    taps_valid = valid.sum(0)
    assert set(np.unique(taps_valid)) == {0, 1, 2, 3, 4}
    got = src >= 0
    assert np.array_equal(got, taps_valid > 0)
    cw = out["color"][got, 3].astype(np.float64)
    for key in ("color", "normal", "albedo"):
        back = out[key][got, :3].astype(np.float64) / cw[:, None]
        assert np.abs(back / mean[got].astype(np.float64) - 1).max() <= 1e-6, key
    assert np.abs(out["scw"][got].astype(np.float64) / cw / 0.7 - 1).max() <= 1e-6 + 2.0 ** -24   # 0.7f itself is rounded
    for key in rb.KEYS:
        assert (out[key][~got] == 0).all() and not np.signbit(out[key][~got]).any()


def test_a_linear_mean_comes_back_as_the_ramp_at_the_reprojected_point(rt):
    """All four taps valid: the blend of the taps' means is the ramp at (fx - 0.5, fy - 0.5), within 1e-5 of the ramp's range."""
    rng, va, o, d, t, e = _sky_pair(2)
    n = W * H
    qx, qy = np.tile(np.arange(W), H).astype(np.float64), np.repeat(np.arange(H), W).astype(np.float64)
    coef = np.array([[0.01, 0.02, 0.5], [-0.015, 0.01, 1.5], [0.02, -0.005, 0.4]])          # positive on the frame
    ramp = lambda x, y: np.stack([c[0] * x + c[1] * y + c[2] for c in coef], axis=1)
    mean = ramp(qx, qy)
    span = (mean.max(0) - mean.min(0)).max()
    out, src, _, valid = _run(va, o, d, t, e, _accumulators(mean.astype(F), rng.integers(1, 50, n), rng))
    four = valid.all(0)
    assert four.mean() > 0.5
    inside, fx, fy, _ = rb.project(W, H, va, o, d, t, e)
    want = ramp(fx[four].astype(np.float64) - 0.5, fy[four].astype(np.float64) - 0.5)
    got = out["color"][four, :3].astype(np.float64) / out["color"][four, 3:4].astype(np.float64)
    assert np.abs(got - want).max() <= 1e-5 * span, np.abs(got - want).max() / span


def test_color_w_is_the_smallest_capped_count_of_the_valid_taps(rt):
    rng, va, o, d, t, e = _sky_pair(3)
    n = W * H
    count = rng.integers(0, 40, n)
    prev = _accumulators(np.ones((n, 3), F), count, rng)
    for max_history in (1, 7, 1000):
        out, src, _, valid = _run(va, o, d, t, e, prev, max_history=max_history)
        inside, fx, fy, _ = rb.project(W, H, va, o, d, t, e)
        q, _, _ = rb.taps(W, H, inside, fx, fy)
        capped = np.where(valid, np.minimum(count[q], max_history), 10 ** 6).min(0)
        got = src >= 0
        assert np.array_equal(out["color"][got, 3], capped[got].astype(F))
        assert np.array_equal(out["color"][:, 3], np.floor(out["color"][:, 3])) and out["color"][:, 3].max() <= max_history
        assert (out["color"][~got, 3] == 0).all()


@pytest.mark.parametrize("w,h", [(8, 8), (41, 29), (96, 54)])
def test_what_the_nearest_call_carries_is_carried_and_a_lone_nearest_tap_is_copied_bit_for_bit(rt, w, h):
    lone_seen = 0
    for k, cfg in enumerate(bc.CONFIGS):
        flags, tol, mh = cfg
        case = bc.make_bilinear_case(w, h, bc.seed_of(w, h, k), mh, 16)
        near, near_src = rr.reproject(w, h, case["va"], case["o"], case["d"], case["t"], case["e"], case["pt"], case["pe"], case["prev"], tol, mh, flags)
        out, src, _, valid = bc.reference(case, flags, tol, mh)
        assert (src[near_src >= 0] >= 0).all(), cfg                        # the containment
        assert (src >= 0).sum() >= (near_src >= 0).sum()
        lone = (near_src >= 0) & (valid.sum(0) == 1)
        lone_seen += int(lone.sum())
        assert np.array_equal(src[lone], near_src[lone])
        for key in rb.KEYS:
            assert np.array_equal(out[key][lone].view(np.uint32), near[key][lone].view(np.uint32)), (cfg, key)
    assert lone_seen > 0


def test_the_nearest_pixel_is_a_tap_of_weight_at_least_a_quarter(rt):
    rng = np.random.default_rng(5)
    for w, h in ((1, 1), (7, 3), (1920, 1080), (1 << 22, 1)):
        fx, fy = (rng.random(4096) * w).astype(F), (rng.random(4096) * h).astype(F)
        fx[:4], fy[:4] = [0, 0.5, np.nextafter(F(w), F(0)), w / 2], [0, np.nextafter(F(h), F(0)), 0.5, h / 2]
        inside = (fx < w) & (fy < h)
        q, b, usable = rb.taps(w, h, inside, fx, fy)
        nearest = fy.astype(np.int64) * w + fx.astype(np.int64)
        is_nearest = usable & (q == nearest[None, :])
        assert (is_nearest.sum(0)[inside] == 1).all(), (w, h)
        assert (np.where(is_nearest, b, 1).min(0) >= 0.25).all(), (w, h)


def test_a_tap_with_a_non_finite_colour_never_reaches_an_output(rt):
    rng, va, o, d, t, e = _sky_pair(6)
    n = W * H
    prev = _accumulators(rng.uniform(0.1, 2, (n, 3)).astype(F), rng.integers(1, 30, n), rng)
    bad = rng.random(n) < 0.25
    prev["color"][bad, rng.integers(0, 4, int(bad.sum()))] = rng.choice([np.nan, np.inf, -np.inf], int(bad.sum()))
    moments = np.stack([rng.uniform(0, 2, n), rng.uniform(0, 4, n), rng.integers(1, 9, n)], axis=1).astype(F)
    out, src, out_m, valid = _run(va, o, d, t, e, prev, moments=moments, max_batches=4)
    inside, fx, fy, _ = rb.project(W, H, va, o, d, t, e)
    q, _, _ = rb.taps(W, H, inside, fx, fy)
    assert not (valid & bad[q]).any() and bad[q].any()
    for key in rb.KEYS:
        assert np.isfinite(out[key]).all(), key
    assert np.isfinite(out_m).all()
    assert not bad[src[src >= 0]].any()


def test_the_moments_rules(rt):
    rng, va, o, d, t, e = _sky_pair(7)
    n = W * H
    prev = _accumulators(np.ones((n, 3), F), rng.integers(1, 30, n), rng)
    mean = rng.uniform(0.2, 2, n)
    cnt = rng.choice(np.array([0, 0.5, 1, 2, 5, 9, np.nan]), n, p=[0.25, 0.1, 0.15, 0.15, 0.15, 0.1, 0.1])
    with np.errstate(all="ignore"):
        moments = np.stack([mean * cnt, 1.5 * mean * cnt, cnt], axis=1).astype(F)
    max_batches = 4
    out, src, out_m, valid = _run(va, o, d, t, e, prev, moments=moments, max_batches=max_batches)
    inside, fx, fy, _ = rb.project(W, H, va, o, d, t, e)
    q, b, _ = rb.taps(W, H, inside, fx, fy)
    with np.errstate(all="ignore"):
        part = valid & np.isfinite(moments[q]).all(2) & (moments[q][:, :, 2] >= 1)
    taking = part.sum(0)
    assert set(np.unique(taking)) == {0, 1, 2, 3, 4}
    none = taking == 0
    assert (out_m[none] == 0).all() and not np.signbit(out_m[none]).any() and (none & (src >= 0)).any()    # carried colour, no moments
    one = taking == 1
    only = q[np.argmax(part, axis=0), np.arange(n)][one]
    m = moments[only]
    small = m[:, 2] <= max_batches
    assert np.array_equal(out_m[one][small].view(np.uint32), m[small].view(np.uint32))                       # a copy bit for bit
    k = F(max_batches) / m[~small, 2]
    assert np.array_equal(out_m[one][~small], np.stack([m[~small, 0] * k, m[~small, 1] * k, np.full(k.size, max_batches, F)], axis=1))
    several = taking > 1
    assert np.array_equal(out_m[several, 2], np.where(part, np.minimum(moments[q][:, :, 2], max_batches), np.inf).min(0)[several].astype(F))
    back = out_m[several, 0].astype(np.float64) / out_m[several, 2]
    lo = np.where(part, mean[q], np.inf).min(0)[several]
    hi = np.where(part, mean[q], -np.inf).max(0)[several]
    assert (back >= lo * (1 - 1e-6)).all() and (back <= hi * (1 + 1e-6)).all()                              # a convex blend of the taps' means
    assert np.abs(out_m[several, 1].astype(np.float64) / out_m[several, 0] / 1.5 - 1).max() <= 1e-6          # s2 = 1.5 s1 at every tap


def test_the_generated_cases_cover_every_number_of_valid_taps(rt):
    """The two conditions the GPU test relies on, with the restatement alone: over the configurations of one size every number of valid taps from 0 to 4 occurs
    (sizes from 8 x 8 up), and at 96 x 54 each holds at least 2 % of the pixels; taps of weight 0 exist, and so do pixels whose moments come from no, one and
    several taps."""
    for w, h in bc.SIZES:
        if w * h < 64 and (w, h) != (9, 7):
            continue
        total, zero_b, taking = np.zeros(5), 0, np.zeros(5)
        for k, cfg in enumerate(bc.CONFIGS):
            flags, tol, mh = cfg
            mb = bc.MAX_BATCHES[k % 2]
            case = bc.make_bilinear_case(w, h, bc.seed_of(w, h, k), mh, mb)
            _, _, _, valid = bc.reference(case, flags, tol, mh, mb)
            total += np.bincount(valid.sum(0), minlength=5)
            zero_b += bc.zero_weight_taps(case)
        share = total / total.sum()
        print("bilinear cases %dx%d: share of pixels with 0..4 valid taps %s, taps of weight 0: %d" % (w, h, np.round(share, 4), zero_b))
        assert (total > 0).all(), ((w, h), total)
        assert zero_b > 0, (w, h)
        if (w, h) == (96, 54):
            assert share.min() >= 0.02, share
