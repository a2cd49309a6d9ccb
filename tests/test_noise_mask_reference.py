"""CPU: tests/noise_mask_reference.py (the numpy restatement of rtowNoiseMaskDevice) held to facts that do not come from the restatement itself: the histogram
accounts for every known pixel, a budget bounds the known qualifying pixels - with errors exactly on bin edges, in the first and in the last bin -, the dilated mask
is a brute-force OR, dilate 0 is the qualifying set, and a triple that is not finite or has n < 2 never reaches a bin."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_mask_reference as nm  # noqa: E402

F = np.float32


def _cases():
    for w, h in ((65, 5), (130, 9), (96, 54)):
        yield w, h, nm.make_moments(w, h, nm.case_seed(w, h))
    yield 70, 6, nm.power_of_two_bands(70, 6)


def test_histogram_sums_to_known_and_counts_add_up():
    for w, h, m in _cases():
        for flags in (0, nm.ABSOLUTE):
            r = nm.noise_mask(w, h, m, 0.01, 2.0 ** -6, 1, 0, flags)
            assert int(r["histogram"].sum()) == r["known"] and r["known"] + r["unknown"] == w * h
            assert r["known"] > 0 and (r["unknown"] > 0 or m[:, 2].min() >= 2)
            known = r["error"] >= 0
            assert np.array_equal(r["error"][~known], np.full(int((~known).sum()), -1, F)) and np.isfinite(r["error"]).all()
            assert r["maxError"] == r["error"][known].max()
            # the bins are what the specification says they hold
            g = r["error"][known].astype(np.float64)
            b = nm.bin_of(r["error"][known])
            inner = (b > 0) & (b < 63)
            assert (g[inner] >= 2.0 ** (b[inner] - 31)).all() and (g[inner] < 2.0 ** (b[inner] - 30)).all()
            assert (g[b == 0] < 2.0 ** -30).all() and (g[b == 63] >= 2.0 ** 32).all()


def test_bin_edges():
    g = np.array([0, 2.0 ** -149, 2.0 ** -31, np.nextafter(F(2.0 ** -30), F(0)), 2.0 ** -30, 1, np.nextafter(F(2), F(0)), 2.0 ** 31, np.nextafter(F(2.0 ** 32), F(0)),
                  2.0 ** 32, 2.0 ** 100, 3.4e38], F)
    assert nm.bin_of(g).tolist() == [0, 0, 0, 0, 1, 31, 31, 62, 62, 63, 63, 63]
    assert [float(nm.bin_lower_bound(b)) for b in (0, 1, 31, 63)] == [0.0, 2.0 ** -30, 1.0, 2.0 ** 32]


@pytest.mark.parametrize("flags", [0, nm.ABSOLUTE, nm.UNKNOWN_QUALIFIES, nm.ABSOLUTE | nm.UNKNOWN_QUALIFIES])
def test_a_budget_bounds_the_known_qualifying_pixels(flags):
    """random moments, and errors exactly on powers of two with bands in bin 0 (2^-40, 2^-31) and bin 63 (2^32, 2^40)"""
    for w, h, m in _cases():
        n = w * h
        g = nm.filtered_error(w, h, nm.own_error(m, bool(flags & nm.ABSOLUTE), 2.0 ** -6))
        if m[0, 0] == 0 and flags & nm.ABSOLUTE:                   # the bands: the construction holds
            inside = g.reshape(h, w)[1:-1, 1::4]
            assert (np.log2(inside.astype(np.float64)) % 1 == 0).all()
            assert (nm.bin_of(g) == 0).any() and (nm.bin_of(g) == 63).any()
        seen = set()
        for budget in (1, 2, n // 16, n // 4, n // 2, n - 1, n, 2 * n):
            for threshold in (2.0 ** -60, 0.01, 2.0 ** 20):
                r = nm.noise_mask(w, h, m, threshold, 2.0 ** -6, 0, budget, flags, g=g)
                known = r["error"] >= 0
                assert int((r["qualifies"] & known).sum()) <= r["R"], (w, h, budget, threshold)
                assert r["qualifying"] <= max(budget, r["unknown"] if flags & nm.UNKNOWN_QUALIFIES else 0)
                assert r["threshold"] >= F(threshold)
                seen.add(float(r["threshold"]))
        assert len(seen) >= 4, seen                                # the budget did move the threshold


def test_the_dilated_mask_is_a_brute_force_or():
    for w, h, m in _cases():
        for radius in (0, 1, 2, 3):
            r = nm.noise_mask(w, h, m, 0.05, 2.0 ** -6, radius, 0, nm.UNKNOWN_QUALIFIES if radius & 1 else 0)
            q = r["qualifies"].reshape(h, w)
            want = np.zeros((h, w), np.uint8)
            for y in range(h):
                for x in range(w):
                    want[y, x] = q[max(0, y - radius): y + radius + 1, max(0, x - radius): x + radius + 1].any()
            assert np.array_equal(r["mask"].reshape(h, w), want), (w, h, radius)
            assert 0 < r["qualifying"] < w * h and r["masked"] == int(want.sum())
            if radius == 0:
                assert np.array_equal(r["mask"], r["qualifies"].astype(np.uint8))
            else:
                assert r["masked"] > r["qualifying"]


def test_non_finite_and_short_triples_are_unknown_and_reach_no_bin():
    bad = [(np.nan, 1, 4), (1, np.nan, 4), (1, 1, np.nan), (np.inf, 1, 4), (1, np.inf, 4), (1, 1, np.inf), (-np.inf, 1, 4), (np.inf, np.inf, np.inf),
           (np.nan, np.nan, np.nan), (1, 1, 0), (1, 1, 1), (1, 1, 1.5), (1, 1, -2)]
    w, h = len(bad), 1
    for flags in (0, nm.ABSOLUTE):
        m = np.array(bad, F)
        assert (nm.own_error(m, bool(flags), 0.5) == -1).all()
        r = nm.noise_mask(w, h, m, 0.01, 0.5, 0, 0, flags)
        assert r["known"] == 0 and r["unknown"] == w and r["histogram"].sum() == 0 and r["maxError"] == 0 and (r["error"] == -1).all()
        assert r["qualifying"] == 0
        assert nm.noise_mask(w, h, m, 0.01, 0.5, 0, 0, flags | nm.UNKNOWN_QUALIFIES)["qualifying"] == w
        # one good pixel between them is filtered over itself alone: g == e
        m[5] = (2, 3, 4)
        r = nm.noise_mask(w, h, m, 0.01, 0.5, 0, 0, flags)
        e = F(F(3) - F(2) * F(0.5)) / F(12)
        want = e if flags else e / F(F(0.25) + F(0.25))
        assert r["known"] == 1 and r["error"][5] == want and r["histogram"][nm.bin_of(np.array([want], F))[0]] == 1
    # a relative error without a floor over a mean of zero is 0 / 0: unknown
    assert nm.own_error(np.array([(0, 0, 4)], F), False, 0.0)[0] == -1 and nm.own_error(np.array([(0, 0, 4)], F), False, 0.5)[0] == 0


def test_a_budget_no_bin_can_meet_gives_an_infinite_threshold():
    m = nm.power_of_two_bands(32, 4)
    r = nm.noise_mask(32, 4, m, 0.01, 0.0, 0, 3, nm.ABSOLUTE)      # the last bin alone holds more than 3 pixels
    assert r["histogram"][63] > 3 and np.isinf(r["threshold"]) and r["qualifying"] == 0
    short = np.zeros((8, 3), F)
    r = nm.noise_mask(8, 1, short, 0.01, 0.0, 0, 3, nm.UNKNOWN_QUALIFIES)      # nothing known: every tail is 0 <= R, b* = 0
    assert r["threshold"] == F(0.01) and r["qualifying"] == 8 and r["R"] == 0
