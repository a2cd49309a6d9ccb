"""CPU: the consequences include/rtow.h states for rtowRectifyHistoryDevice, held on the numpy restatement (tests/rectify_history_reference.py), and the condition on the
generated cases that keeps the GPU comparison (tests/test_gpu_rectify_history.py) from passing vacuously: every outcome on at least 5 % of the pixels, and a tile
without a valid history next to one with some."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_history_reference as rh  # noqa: E402

F = np.float32
OUT = ("color", "normal", "albedo", "scw", "moments", "keep")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    return {(w, h): rh.make_case(w, h, rh.case_seed(w, h)) for w, h in rh.SIZES}


@pytest.fixture(scope="module")
def results(cases):
    return {(size, k): rh.reference(case, cfg) for size, case in cases.items() for k, cfg in enumerate(rh.CONFIGS)}


def test_huge_tolerances_copy_everything_bit_for_bit(cases):
    for size, case in cases.items():
        for sigma, rel in ((1e18, 0.0), (0.0, 1e18), (1e18, 1e18)):
            got = rh.rectify(case["w"], case["h"], case["history"], case["fresh"], case["hits"], case["moments"], 3, 2, 2, 0.05, sigma, rel, 1)
            assert not (got["outcome"] >= rh.CUT).any(), (size, sigma, rel)
            for key in rh.KEYS:
                assert np.array_equal(_bits(got[key[0]]).ravel(), _bits(case["history"][key[0]]).ravel()), (size, key)
            assert np.array_equal(_bits(got["moments"]), _bits(case["moments"])) and (got["keep"] == 1).all()
            assert got["stats"][0] == got["stats"][1] and got["stats"][2] == got["stats"][3] == 0
    # relativeTolerance alone cannot keep a pixel whose neighbourhood mean is zero, sigmaScale alone one whose neighbourhood does not vary: only the 2^-20 is left
    big = [s for s in cases if s[0] * s[1] >= 256]
    assert any(rh.reference(cases[s], rh.CONFIGS[0])["stats"][1] > 0 for s in big)


def test_holes_stay_holes_and_unjudged_pixels_keep_their_bits(cases, results):
    for (size, k), got in results.items():
        case = cases[size]
        hole = case["hole"]
        assert (got["outcome"][hole] == rh.UNJUDGED).all()
        for key in OUT[:5]:
            assert (_bits(got[key]).reshape(case["n"], -1)[hole] == 0).all(), (size, k, key)       # +0, every float
        assert (got["keep"][hole] == 1).all()
        same = got["outcome"] <= rh.KEPT
        for key, _ in rh.KEYS:
            assert np.array_equal(_bits(got[key]).reshape(case["n"], -1)[same], _bits(case["history"][key]).reshape(case["n"], -1)[same]), (size, k, key)
        assert np.array_equal(_bits(got["moments"])[same], _bits(case["moments"])[same]) and (got["keep"][same] == 1).all()
        dropped = got["outcome"] == rh.DROPPED
        for key in OUT:
            assert (_bits(got[key]).reshape(case["n"], -1)[dropped] == 0).all(), (size, k, key)


def test_a_cut_pixel_has_an_integral_smaller_count_and_its_old_mean(cases, results):
    seen = 0
    for (size, k), got in results.items():
        case = cases[size]
        cut = got["outcome"] == rh.CUT
        seen += int(cut.sum())
        old, new = case["history"]["color"][cut].astype(np.float64), got["color"][cut].astype(np.float64)
        assert (new[:, 3] == np.trunc(new[:, 3])).all() and (new[:, 3] >= 1).all() and (new[:, 3] < old[:, 3]).all(), (size, k)
        keep = got["keep"][cut].astype(np.float64)
        assert ((keep > 0) & (keep < 1)).all()
        # k = newW / h.w is one rounding off, x * k another, so the mean moves by at most a few units in the last place
        assert np.allclose(new[:, :3] / new[:, 3:4], old[:, :3] / old[:, 3:4], rtol=4 * 2.0 ** -23, atol=0), (size, k)
        m_old, m_new = case["moments"][cut].astype(np.float64), got["moments"][cut].astype(np.float64)
        ok = np.isfinite(m_old).all(axis=1) & (m_old[:, 2] > 0)
        assert np.allclose(m_new[ok, 0] / m_new[ok, 2], m_old[ok, 0] / m_old[ok, 2], rtol=4 * 2.0 ** -23, atol=0), (size, k)
    assert seen > 100


def test_judged_is_the_sum_of_the_three_counts(results):
    for (size, k), got in results.items():
        s = got["stats"]
        assert s[0] == s[1] + s[2] + s[3] and s[0] == (got["outcome"] != rh.UNJUDGED).sum() and s[0] <= size[0] * size[1], (size, k)


def test_in_place_equals_out_of_place(cases):
    """The pass reads history and moments at its own pixel only: running it in place - every output the matching input - is running it pixel by pixel in any order,
    each pixel seeing its own old values.  Restated: the pixels rectified one half of the frame after the other, the second half reading buffers the first half has
    already overwritten, give the bits of the whole frame at once."""
    for size in ((65, 5), (131, 9)):
        case = cases[size]
        n = case["n"]
        for cfg in (rh.CONFIGS[0], rh.CONFIGS[4]):
            want = rh.reference(case, cfg)
            live = {k: v.copy() for k, v in case["history"].items()}
            live_m = case["moments"].copy()
            order = np.random.default_rng(3).permutation(n)
            for part in (order[: n // 2], order[n // 2:]):
                got = rh.rectify(case["w"], case["h"], live, case["fresh"], case["hits"], live_m, *cfg)
                for key, _ in rh.KEYS:
                    live[key][part] = got[key][part]
                live_m[part] = got["moments"][part]
            for key, _ in rh.KEYS:
                assert np.array_equal(_bits(live[key]).ravel(), _bits(want[key]).ravel()), (size, key)
            assert np.array_equal(_bits(live_m), _bits(want["moments"]))


def test_null_moments_change_nothing_else(cases):
    case = cases[(70, 10)]
    a, b = rh.reference(case, rh.CONFIGS[0]), rh.reference(case, rh.CONFIGS[0], moments=False)
    assert b["moments"] is None
    for key in ("color", "normal", "albedo", "scw", "keep", "stats"):
        assert np.array_equal(_bits(a[key]).ravel(), _bits(b[key]).ravel()) if key != "stats" else np.array_equal(a[key], b[key])


def test_every_outcome_covers_five_percent_of_the_random_cases(cases, results):
    """The condition the GPU comparison rests on: under the configurations rh.COVERED every case of at least 256 pixels has at least 5 % of its pixels unjudged, kept,
    cut and dropped, and so have the pixels of all configurations taken together; minTaps = (2 r + 1)^2 leaves interior pixels unjudged, T = 2^-20 cuts or drops."""
    total = np.zeros(4)
    pixels = 0
    for (size, k), got in results.items():
        if size[0] * size[1] < 256:
            continue
        s = rh.shares(got["outcome"])
        total += np.array(s) * cases[size]["n"]
        pixels += cases[size]["n"]
        if k in rh.COVERED:
            assert min(s) >= 0.05, (size, k, s)
    assert (total / pixels >= 0.05).all(), total / pixels
    # minTaps at its maximum: a judgement needs every tap, and one fresh pixel in six is invalid
    assert all(rh.shares(results[(size, 3)]["outcome"])[0] > 0.5 for size in cases if size[0] * size[1] >= 256)
    for size in cases:                                                 # both tolerances zero: a judged pixel is kept only within 2^-10 of the neighbourhood mean
        s = results[(size, 4)]["stats"]
        assert s[1] <= s[0] // 20


def test_a_tile_without_history_lies_next_to_one_with_some(cases):
    for size in ((65, 5), (70, 10), (131, 9)):
        without, with_ = rh.tiles_without_and_with_history(cases[size])
        assert (1, 0) in without and (0, 0) in with_, (size, without)
    assert rh.tiles_without_and_with_history(cases[(64, 4)]) == ([], [(0, 0)])
    empty = rh.make_case(70, 10, 5, holes="all")
    assert rh.tiles_without_and_with_history(empty)[1] == []
    got = rh.reference(empty, rh.CONFIGS[0])
    assert (got["stats"] == 0).all() and (got["keep"] == 1).all() and (_bits(got["color"]) == 0).all()


def test_the_inputs_hold_what_the_specification_singles_out(cases):
    case = cases[(131, 9)]
    c, f = case["history"]["color"], case["fresh"]
    t, e, nrm = case["hits"]
    assert np.isnan(c).any() and np.isinf(c).any() and np.isnan(f).any() and np.isinf(f).any()
    for wv in (0, 0.5, 1):
        assert (c[:, 3] == wv).any() and (f[:, 3] == wv).any(), wv
    assert (e < 0).any() and ((e >= 0) & (nrm == 0).all(axis=1)).any() and np.isnan(t).any()
