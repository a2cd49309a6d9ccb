"""CPU: tests/temporal_moments_reference.py (the numpy restatement of rtowReprojectMomentsDevice and rtowEstimateMomentsDevice) held to facts that do not come from
it - known answers, the consequences the header states, its guide weight against rtowUpsampleDevice's restatement - and the coverage condition of the GPU
comparison, which needs no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_variance_reference as dv  # noqa: E402
import temporal_moments_reference as tm  # noqa: E402
import upsample_reference as ur  # noqa: E402

F = np.float32


def _flat(w, h, entity=2, distance=3.0, normal=(0, 0, 1)):
    n = w * h
    return np.full(n, distance, F), np.full(n, entity, np.int32), np.tile(np.asarray(normal, F), (n, 1))


def _colour(lum_values, samples=4.0):
    """grey colours of the given mean luminance (grey: lum = the value up to rounding), as sums over `samples`"""
    l = np.asarray(lum_values, F).reshape(-1)
    return np.stack([l * F(samples)] * 3 + [np.full(l.size, samples, F)], axis=1).astype(F)


def test_a_frame_of_constant_luminance_has_zero_variance():
    w, h = 19, 11
    color = _colour(np.full(w * h, 0.75))
    out, filled, wanted = tm.estimate_moments(w, h, color, _flat(w, h), None, 4, 2, 2, 0.05, 1)
    assert filled.all() and wanted.all()
    assert (out[:, 2] == 2).all()
    v0 = dv.initial_variance(out, np.ones((w * h, 3), F), flags=0)
    assert (v0 == 0).all()
    l = dv.lum(color[:, :3] / color[:, 3:])
    assert np.array_equal(out[:, 0], l + l)                               # W = taps exactly, S1 = taps * l up to rounding that the division undoes for 0.75


def test_with_49_taps_only_full_fully_accepted_windows_are_filled():
    w, h = 16, 12
    rng = np.random.default_rng(3)
    color = _colour(rng.uniform(0.2, 1.5, w * h))
    t, e, nrm = _flat(w, h)
    e[5 * w + 12] = 4                                                      # one foreign pixel: no window that holds it is fully accepted
    out, filled, _ = tm.estimate_moments(w, h, color, (t, e, nrm), None, 4, 49, 0, 0.05, 1)
    want = np.zeros((h, w), bool)
    want[3:h - 3, 3:w - 3] = True
    want[2:9, 9:16] = False
    assert np.array_equal(filled.reshape(h, w).astype(bool), want)
    assert (out[~want.reshape(-1)] == 0).all()                             # unchanged: the zeros of a NULL inMoments


def test_a_luminance_step_on_an_entity_edge_is_each_side_alone():
    w, h = 14, 9
    left = np.tile(np.arange(w) < 7, h)
    rng = np.random.default_rng(5)
    l = np.where(left, 0.2, 3.0) + rng.uniform(0, 0.05, w * h)
    color = _colour(l)
    t, e, nrm = _flat(w, h)
    e[~left] = 3
    both, filled, _ = tm.estimate_moments(w, h, color, (t, e, nrm), None, 4, 2, 2, 0.05, 1)
    assert filled.all()
    for side, cols in ((left, slice(0, 7)), (~left, slice(7, 14))):
        sub = color.reshape(h, w, 4)[:, cols].reshape(-1, 4)
        alone, f2, _ = tm.estimate_moments(7, h, sub, _flat(7, h), None, 4, 2, 2, 0.05, 1)
        assert f2.all()
        assert np.array_equal(both[side].view(np.uint32), alone.view(np.uint32))
    mixed, _, _ = tm.estimate_moments(w, h, color, (t, e, nrm), None, 4, 2, 2, 0.05, 0)      # without the flag the step leaks into the variance
    v_edge = dv.initial_variance(mixed, np.ones((w * h, 3), F), 0).reshape(h, w)[4, 6]
    v_kept = dv.initial_variance(both, np.ones((w * h, 3), F), 0).reshape(h, w)[4, 6]
    assert v_edge > 100 * v_kept


def test_unqualified_invalid_and_sparse_pixels_are_unchanged():
    w, h = 9, 9
    color = _colour(np.full(w * h, 0.5))
    color[40, 3] = 0                                                       # the centre pixel has no sample: L invalid
    m = np.zeros((w * h, 3), F)
    m[:, 2] = 1
    m[0] = (5.0, 7.0, 4.0)                                                 # qualifies for nothing: n >= minBatches
    m[1] = (np.nan, 1.0, np.nan)                                           # a NaN n is estimated
    out, filled, wanted = tm.estimate_moments(w, h, color, _flat(w, h), m, 4, 2, 2, 0.05, 1)
    assert not wanted[0] and not filled[0] and np.array_equal(out[0], m[0])
    assert wanted[1] and filled[1] and out[1, 2] == 2
    assert wanted[40] and not filled[40] and np.array_equal(out[40], m[40])
    t, e, nrm = _flat(w, h)
    e[:] = np.arange(w * h)                                                # every pixel its own entity: one tap each
    out, filled, _ = tm.estimate_moments(w, h, color, (t, e, nrm), m, 4, 2, 2, 0.05, 1)
    assert not filled.any() and np.array_equal(out.view(np.uint32), m.view(np.uint32))


def test_the_cap_keeps_the_mean():
    prev = np.array([[6.0, 9.5, 4.0], [48.0, 100.0, 32.0], [3.0, 5.0, 16.0], [1.5, 2.0, 17.0]], F)
    out = tm.reproject_moments(np.array([0, 1, 2, 3], np.int32), prev, 16)
    assert np.array_equal(out[0], prev[0]) and np.array_equal(out[2], prev[2])          # at or below the cap: bit for bit
    assert np.array_equal(out[1], np.array([24.0, 50.0, 16.0], F))                     # k = 1/2 exactly
    assert out[3, 2] == 16
    np.testing.assert_allclose(out[3, 0] / out[3, 2], prev[3, 0] / prev[3, 2], rtol=3e-7)
    np.testing.assert_allclose(out[3, 1] / out[3, 2], prev[3, 1] / prev[3, 2], rtol=3e-7)


def test_sources_outside_the_frame_and_invalid_moments_give_zeros():
    prev = np.array([[1.0, 1.0, 1.0], [np.nan, 1.0, 2.0], [1.0, np.inf, 2.0], [1.0, 1.0, np.nan], [1.0, 1.0, 0.5], [2.0, 3.0, 2.0]], F)
    src = np.array([-1, 6, 1, 2, 3, 4], np.int32)
    out = tm.reproject_moments(src, prev, 8)
    assert np.array_equal(out.view(np.uint32), np.zeros((6, 3), np.uint32))            # +0, not -0
    src = np.array([5, 0, -2 ** 31, 2 ** 31 - 1, 5, 0], np.int32)
    out = tm.reproject_moments(src, prev, 8)
    assert np.array_equal(out[[0, 1, 4, 5]], prev[[5, 0, 5, 0]]) and (out[[2, 3]] == 0).all()


def test_the_guide_weight_accepts_what_rtowUpsampleDevices_restatement_accepts():
    """At equal sizes the upsampling restatement reads src pixel p for dst pixel p with bilinear weight 1: with the src guides shifted by one pixel, its stage A answers
    exactly where g(p, p + 1) > 0."""
    w, h = 48, 27
    for seed, (sharp, tol, flags) in enumerate([(4, 0.05, 1), (0, 1.0, 0), (8, 0.01, 1), (2, 0.0, 0)]):
        case = ur.make_case(w, h, w, h, 40 + seed)
        dt, de, dn = case["dst_hits"]
        shift = lambda a: np.roll(a.reshape(h, w, *a.shape[1:]), -1, axis=1).reshape(a.shape)
        st, se, sn = shift(dt), shift(de), shift(dn)
        color = np.ones((w * h, 3), F)
        _, stage, _ = ur.upsample(w, h, w, h, ur.GUIDED, sharp, tol, flags & 1, color, (st, se, sn), None, (dt, de, dn))
        g = tm.guide_weight(de, dt, dn, se, st, sn, sharp, tol, flags & 1)
        assert np.array_equal(stage == 0, g > 0)
        assert 0.05 < (g > 0).mean() < 0.98


@pytest.mark.parametrize("w,h", [s for s in tm.SIZES if s[0] * s[1] > 64])
def test_the_generated_cases_exercise_every_outcome(w, h):
    """What keeps agreement on "unchanged" from hiding a dead kernel in tests/test_gpu_temporal_moments.py: with minTaps 2 every case larger than 8 x 8 has filled
    pixels, qualifying pixels left unchanged and pixels that do not qualify."""
    case = tm.make_case(w, h, tm.case_seed(w, h))
    for cfg in tm.CONFIGS:
        if cfg[1] != 2:
            continue
        _, filled, wanted = tm.reference(case, cfg)
        cov = tm.coverage(filled, wanted)
        assert min(cov) >= 3, (cfg, cov)
        _, f_null, w_null = tm.reference(case, cfg, None)
        assert w_null.all() and tm.coverage(f_null, w_null)[0] >= 3 and tm.coverage(f_null, w_null)[1] >= 1, cfg
    m1, p = tm.one_pixel_qualifies(case, tm.CONFIGS[0])
    _, f1, w1 = tm.reference(case, tm.CONFIGS[0], m1)
    assert w1.sum() == 1 and w1[p]
    _, f0, w0 = tm.reference(case, tm.CONFIGS[0], tm.no_pixel_qualifies(case, tm.CONFIGS[0]))
    assert not w0.any() and not f0.any()
