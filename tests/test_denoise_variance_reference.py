"""CPU: known answers of tests/denoise_variance_reference.py, the numpy restatement the GPU tests hold rtowAccumulateMomentsDevice and rtowDenoiseVarianceDevice to."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402
import denoise_variance_reference as dv  # noqa: E402

F = np.float32


def _flat(w, h):
    n = w * h
    nrm = np.tile(np.array([0, 0, 1], F), (n, 1))
    a = np.full((n, 3), 0.5, F)
    return nrm, a


def test_unit_variance_under_the_plain_b3_kernel():
    """Equal normals and albedo, colorSigma 0, v0 = 1 everywhere: an interior pixel's weights are h(i) h(j), they sum to 1, and the variance out is the sum
    of their squares, (2/256 + 2/16 + 9/64)^2 = 0.2734375^2, exactly."""
    w, h = 9, 9
    nrm, a = _flat(w, h)
    c = np.random.default_rng(0).uniform(0, 1, (w * h, 3)).astype(F)
    (c1, v1), = dv.denoise_variance_levels(w, h, c, nrm, a, None, 1, 4, 0.0, 0.5, 0, v0=np.ones(w * h, F))
    assert v1[4, 4] == F(0.2734375) * F(0.2734375) == F(0.07476806640625)
    assert v1[2:7, 2:7].min() == v1[2:7, 2:7].max()                       # every pixel whose 25 taps lie inside the image
    assert v1[0, 0] > v1[4, 4]                                            # at the border fewer taps average: less variance reduction
    assert np.array_equal(c1.view(np.uint32), dr.denoise_levels(w, h, c, nrm, a, 1, 4, 0.0, 0.5, 0)[0].view(np.uint32))


def test_moments_of_identical_batches_give_zero_variance():
    n = 5
    c = np.zeros((n, 4), F)
    c[:, :3] = [[0.5, 0.25, 1.0], [1, 1, 1], [0, 0, 0], [2, 4, 8], [0.125, 0.5, 0.75]]
    c[:, 3] = 1
    m = dv.accumulate_moments([c, c, c, c])
    assert np.array_equal(m[:, 2], np.full(n, 4, F))
    l = dv.lum(c[:, :3])
    assert np.array_equal(m[:, 0], ((l + l) + l) + l)
    v0 = dv.initial_variance(m, np.ones((n, 3), F), 0)
    assert np.array_equal(v0, np.zeros(n, F)) and not np.signbit(v0).any()          # +0: s2 - s1 * mean cancels to <= 0 and is clamped
    # the same sums scaled by the sample count: the mean is what counts (c.xyz / c.w)
    c2 = c.copy()
    c2 *= F(4)
    assert np.array_equal(dv.accumulate_moments([c2, c2, c2, c2]), m)


def test_fewer_than_two_batches_is_unknown():
    c = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 1, -2], [1, 1, 1, np.nan], [np.inf, 1, 1, 1], [np.nan, 1, 1, 2]], F)
    m = dv.accumulate_moments([c])
    assert np.array_equal(m[:, 2], np.array([1, 0, 0, 0, 0, 0], F))        # w = 0, w < 0, NaN w and a non-finite luminance are skipped
    assert np.array_equal(m[1:], np.zeros((5, 3), F))
    v0 = dv.initial_variance(m, np.ones((6, 3), F), 0)
    assert np.array_equal(v0, np.full(6, -1, F))
    # n = 2 is the first known count: two luminances 1 and 3 have variance of the mean ((1-2)^2 + (3-2)^2) / (2 * 1) = 1
    m2 = np.array([[4, 10, 2]], F)
    assert dv.initial_variance(m2, np.ones((1, 3), F), 0)[0] == F(1)
    # demodulation divides by the squared luminance of the albedo; an albedo below 2^-10 leaves the variance as it is
    a = np.array([[0.5, 0.5, 0.5]], F)
    la = dv.lum(a)[0]
    assert dv.initial_variance(m2, a, 1)[0] == F(1) / (la * la)
    assert dv.initial_variance(m2, np.full((1, 3), 2.0 ** -12, F), 1)[0] == F(1)
    # huge and NaN moments: a non-finite estimate is unknown, a NaN difference clamps to 0
    odd = np.array([[0, np.inf, 2], [np.nan, 1, 3], [1, np.nan, 3], [1, 1, np.nan], [1, 1, np.inf], [0, 3e38, 2]], F)
    v = dv.initial_variance(odd, np.ones((6, 3), F), 0)
    assert v[0] == -1 and v[1] == 0 and v[2] == 0 and v[3] == -1 and v[4] == 0 and v[5] == F(3e38) / F(2)


def test_no_colour_term_is_the_plain_filter_at_color_sigma_zero():
    """colorSigma == 0: the colour of every level equals tests/denoise_reference.py's at colorSigma 0, bit for bit, whatever the moments say; and with every
    n < 2 the same holds for colorSigma > 0 (no pixel has a variance, so no pixel has a colour term)."""
    rng = np.random.default_rng(3)
    w, h = 23, 17
    n = w * h
    c = rng.uniform(0, 3, (n, 3)).astype(F)
    c[rng.integers(0, n, 5), 1] = np.nan
    nrm = rng.normal(size=(n, 3)).astype(F)
    nrm[rng.random(n) < 0.6] = nrm[0]
    nrm[rng.random(n) < 0.1] = 0
    a = rng.uniform(0, 1, (n, 3)).astype(F)
    moments = np.stack([rng.uniform(0, 8, n), rng.uniform(0, 40, n), rng.integers(0, 6, n)], axis=1).astype(F)
    for flags in (0, 1):
        plain = dr.denoise_levels(w, h, c, nrm, a, 4, 2, 0.0, 0.3, flags)
        got = dv.denoise_variance_levels(w, h, c, nrm, a, moments, 4, 2, 0.0, 0.3, flags)
        for k in range(4):
            assert np.array_equal(got[k][0].view(np.uint32), plain[k].view(np.uint32)), (flags, k)
        few = moments.copy()
        few[:, 2] = rng.integers(0, 2, n)
        got = dv.denoise_variance_levels(w, h, c, nrm, a, few, 4, 2, 3.0, 0.3, flags)
        for k in range(4):
            assert np.array_equal(got[k][0].view(np.uint32), plain[k].view(np.uint32)), (flags, k)
            assert (got[k][1] == -1).all()
    # and the colour term does something when it is on
    on = dv.denoise_variance_levels(w, h, c, nrm, a, moments, 4, 2, 3.0, 0.3, 1)
    assert not np.array_equal(on[3][0].view(np.uint32), dr.denoise_levels(w, h, c, nrm, a, 4, 2, 0.0, 0.3, 1)[3].view(np.uint32))
