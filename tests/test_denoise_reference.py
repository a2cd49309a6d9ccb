"""CPU: properties of the numpy restatement of rtowDenoiseDevice (tests/denoise_reference.py), which the GPU tests hold the kernel to bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import denoise_reference as dr  # noqa: E402

F = np.float32


def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


@pytest.mark.parametrize("flags", [0, dr.DEMODULATE_ALBEDO])
@pytest.mark.parametrize("iterations", [1, 3, 5, 8])
def test_a_constant_image_stays_constant(flags, iterations):
    """Every weight is positive and every tap has the centre's colour, so acc / wsum = c * (wsum / wsum) up to the rounding of the sums: at most 25 taps per
    level, each sum within a few ulps.  Stated bound: 8 ulps from the input after any number of levels (measured: 3)."""
    w, h = 23, 17
    n = w * h
    c = np.tile(F([0.3, 1.7, 0.05]), (n, 1))
    nrm = np.tile(F([0.0, 0.6, 0.8]), (n, 1))
    alb = np.tile(F([0.5, 0.25, 0.75]), (n, 1))
    out = dr.denoise_reference(w, h, c, nrm, alb, iterations, 4, 0.5, 0.5, flags)
    assert np.isfinite(out).all()
    assert _ulps(out, c).max() <= 8


def test_without_colour_and_albedo_terms_uniform_normals_give_the_b3_spline_blur():
    """Both sigmas 0, every normal the same unit vector (n.n = 1 exactly: (0, 0, 1)): every tap weight is h(i) h(j) - one level is the plain B3 spline
    blur, normalised over the taps inside the image.  Restated independently: a separable weight mask, summed in the same tap order."""
    rng = np.random.default_rng(3)
    w, h = 19, 13
    n = w * h
    c = rng.uniform(0, 4, (n, 3)).astype(F)
    nrm = np.tile(F([0, 0, 1]), (n, 1))
    alb = rng.uniform(0, 1, (n, 3)).astype(F)
    for step, k in ((1, 1), (2, 2), (4, 3)):
        got = dr.denoise_levels(w, h, c, nrm, alb, k, 8, 0.0, 0.0, 0)[-1]
        prev = c.reshape(h, w, 3) if k == 1 else dr.denoise_levels(w, h, c, nrm, alb, k - 1, 8, 0.0, 0.0, 0)[-1]
        want = np.empty_like(prev)
        for y in range(h):
            for x in range(w):
                acc, ws = np.zeros(3, F), F(0)
                for j in range(-2, 3):
                    for i in range(-2, 3):
                        qy, qx = y + j * step, x + i * step
                        if 0 <= qy < h and 0 <= qx < w:
                            wt = dr.H[i + 2] * dr.H[j + 2]
                            acc = acc + wt * prev[qy, qx]
                            ws = ws + wt
                want[y, x] = acc / ws
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), step


def test_perpendicular_normals_give_zero_weight_across_an_edge():
    """Two planes meeting at a vertical edge with normals (1, 0, 0) and (0, 1, 0): n.n' = 0, so wn = 0 for every tap across the edge and no colour
    crosses it, at any level: changing every colour right of the edge leaves every output left of it bit-identical."""
    rng = np.random.default_rng(4)
    w, h, edge = 40, 12, 17
    n = w * h
    c = rng.uniform(0, 2, (n, 3)).astype(F)
    nrm = np.zeros((h, w, 3), F)
    nrm[:, :edge] = (1, 0, 0)
    nrm[:, edge:] = (0, 1, 0)
    alb = rng.uniform(0.2, 1, (n, 3)).astype(F)
    for sharp in (0, 4):
        whole = dr.denoise_reference(w, h, c, nrm.reshape(-1, 3), alb, 5, sharp, 0.5, 0.5, dr.DEMODULATE_ALBEDO).reshape(h, w, 3)
        c2 = c.reshape(h, w, 3).copy()
        c2[:, edge:] = rng.uniform(0, 50, (h, w - edge, 3))
        other = dr.denoise_reference(w, h, c2.reshape(-1, 3), nrm.reshape(-1, 3), alb, 5, sharp, 0.5, 0.5, dr.DEMODULATE_ALBEDO).reshape(h, w, 3)
        assert np.array_equal(whole[:, :edge].view(np.uint32), other[:, :edge].view(np.uint32))
        assert not np.array_equal(whole[:, edge:], other[:, edge:])


def test_a_nan_tap_changes_only_its_own_pixel():
    """A colour with a NaN channel passes through at its own pixel and is skipped as a tap (nothing added: not 0 * NaN, which would poison the sums).
    The pixel gets an exactly-zero normal among non-zero ones, so its neighbours give it weight 0 whatever its colour: with and without the NaN, every
    other pixel is bit-identical."""
    rng = np.random.default_rng(5)
    w, h = 21, 15
    n = w * h
    c = rng.uniform(0, 2, (n, 3)).astype(F)
    nrm = np.tile(F([0, 0, 1]), (n, 1))
    alb = rng.uniform(0.2, 1, (n, 3)).astype(F)
    p = 7 * w + 9
    nrm[p] = 0                                                     # exactly-zero normal next to non-zero ones: wn = 0 both ways
    a = dr.denoise_reference(w, h, c, nrm, alb, 1, 4, 0.5, 0.5, 0)
    c2 = c.copy()
    c2[p, 1] = np.nan
    b = dr.denoise_reference(w, h, c2, nrm, alb, 1, 4, 0.5, 0.5, 0)
    others = np.arange(n) != p
    assert np.array_equal(a[others].view(np.uint32), b[others].view(np.uint32))
    assert np.isnan(b[p, 1]) and np.array_equal(b[p, [0, 2]], c[p, [0, 2]])   # passes through unchanged


def test_a_nan_tap_is_skipped_not_weighted():
    """With uniform normals the non-finite pixel IS a neighbour: every other pixel's output equals the explicit sums over its taps without that one."""
    rng = np.random.default_rng(6)
    w, h = 9, 7
    n = w * h
    c = rng.uniform(0, 2, (n, 3)).astype(F)
    nrm = np.tile(F([0, 0, 1]), (n, 1))
    alb = np.ones((n, 3), F)
    p = 3 * w + 4
    c[p, 0] = np.inf
    out = dr.denoise_reference(w, h, c, nrm, alb, 1, 0, 0.0, 0.0, 0).reshape(h, w, 3)
    img = c.reshape(h, w, 3)
    for y in range(h):
        for x in range(w):
            if y * w + x == p:
                assert np.array_equal(out[y, x], img[y, x])
                continue
            acc, ws = np.zeros(3, F), F(0)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    qy, qx = y + j, x + i
                    if 0 <= qy < h and 0 <= qx < w and qy * w + qx != p:
                        wt = dr.H[i + 2] * dr.H[j + 2]
                        acc = acc + wt * img[qy, qx]
                        ws = ws + wt
            assert np.array_equal(out[y, x].view(np.uint32), (acc / ws).view(np.uint32)), (x, y)


def test_demodulation_rule_and_exact_binary_weights():
    assert [float(x) for x in dr.H] == [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16] and float(dr.H[2] * dr.H[2]) == 9 / 64
    c = F([[2.0, 2.0, 2.0]])
    a = F([[0.5, 2.0 ** -10, 2.0 ** -11]])
    assert dr.demodulate(c, a).tolist() == [[4.0, 2048.0, 2.0]]
    assert dr.remodulate(F([[4.0, 2048.0, 2.0]]), a).tolist() == [[2.0, 2.0, 2.0]]
