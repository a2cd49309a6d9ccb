"""CPU: tests/upsample_reference.py (the numpy restatement of rtowUpsampleDevice's specification, include/rtow.h) held to facts that do not come from it: the point
pixel in exact rationals, k x k replication, the identity, GUIDED with uniform guides == BILINEAR, linear ramps, edges that hold exactly, sky and surface kept
apart - and the coverage condition of the random inputs tests/test_gpu_upsample.py runs the kernel on."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import upsample_reference as ur  # noqa: E402

F = np.float32
# (src, dst) sizes of one axis: 1, primes, non-integer ratios, ratios above 1, and the ends of the allowed range both ways
AXIS_PAIRS = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 10), (13, 37), (37, 13), (97, 101), (101, 97), (540, 1080), (1080, 540), (641, 1920), (1920, 641),
              (16383, 16384), (16384, 16383), (1, 16384), (16384, 1), (16384, 16384), (16381, 16384), (3, 16384)]


def _uniform_hits(n, entity=2, distance=3.0, normal=(0.0, 0.0, 1.0)):
    return np.full(n, distance, F), np.full(n, entity, np.int32), np.tile(np.array(normal, F), (n, 1))


@pytest.mark.parametrize("src,dst", AXIS_PAIRS)
def test_positions_in_exact_rationals(src, dst):
    """px = floor((X + 0.5) / dst * src); x0 = floor((X + 0.5) / dst * src - 0.5) and fx the fraction left, the texel pair and weight of a bilinear read at the pixel
    centre - all three for every X, in exact rationals; fx is that fraction rounded to float32 once."""
    point, x0, fx = ur.axis_positions(src, dst)
    assert point.dtype == np.int64 and fx.dtype == F
    for X in range(dst):
        u = (Fraction(X) + Fraction(1, 2)) / dst * src
        assert int(point[X]) == u.numerator // u.denominator
        s = u - Fraction(1, 2)
        fl = s.numerator // s.denominator                       # Python's // floors
        assert int(x0[X]) == fl and -1 <= fl <= src - 1
        frac = s - fl
        assert 0 <= frac < 1 and abs(Fraction(float(fx[X])) - frac) <= Fraction(1, 2 ** 25)       # within half an ulp of a float32 below 1
    assert point.min() >= 0 and point.max() <= src - 1


@pytest.mark.parametrize("k", [1, 2, 3, 5])
def test_an_integer_ratio_replicates_each_pixel_in_point_mode(k):
    sw, sh = 7, 5
    c = np.random.default_rng(k).uniform(0, 2, (sw * sh, 3)).astype(F)
    c[3] = (np.nan, np.inf, -0.0)
    out, stage, _ = ur.upsample(sw, sh, sw * k, sh * k, ur.POINT, 0, 0.0, 0, c)
    want = np.repeat(np.repeat(c.reshape(sh, sw, 3), k, axis=0), k, axis=1).reshape(-1, 3)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and (stage == 2).all()


def test_the_same_size_returns_the_source_bit_for_bit():
    """srcW == dstW, srcH == dstH, no demodulation: fx = fy = 0, so stage A is the one tap (x0, y0) = p with weight (1 * 1) * g, and r = (g * c) / g.  POINT and BILINEAR
    (g = 1) return the source bit for bit wherever it is finite, and so does GUIDED wherever g of the pixel with itself is exactly 1 (sky, or a normal whose dot with
    itself is 1: here the axes); for other unit normals g is 1 to a few ulp and (g * c) / g is c to 1 ulp.  Non-finite colours pass through stage C."""
    w, h = 23, 11
    n = w * h
    rng = np.random.default_rng(3)
    c = rng.uniform(0, 5, (n, 3)).astype(F)
    c[5, 1], c[77, 0] = np.nan, np.inf                            # stage C hands these through
    t, e = rng.uniform(1, 9, n).astype(F), rng.integers(-1, 4, n).astype(np.int32)
    axes = np.array([(1, 0, 0), (0, -1, 0), (0, 0, 1)], F)[rng.integers(0, 3, n)]
    axes[e < 0] = 0
    hits = (t, e, axes)
    finite = np.isfinite(c).all(axis=1)
    for mode, sharp, flags in ((ur.POINT, 0, 0), (ur.BILINEAR, 0, 0), (ur.GUIDED, 0, 0), (ur.GUIDED, 8, ur.MATCH_ENTITY)):
        out, stage, _ = ur.upsample(w, h, w, h, mode, sharp, 0.0, flags, c, hits, None, hits, None)
        assert np.array_equal(out.view(np.uint32), c.view(np.uint32)), mode
        if mode != ur.POINT:
            assert (stage[finite] == 0).all() and (stage[~finite] == 2).all()
    rough = rng.normal(size=(n, 3))
    rough = (rough / np.linalg.norm(rough, axis=1)[:, None]).astype(F)
    rough[e < 0] = 0
    out, stage, _ = ur.upsample(w, h, w, h, ur.GUIDED, 1, 0.0, 0, c, (t, e, rough), None, (t, e, rough), None)
    assert (stage[finite] == 0).all() and np.array_equal(out[~finite].view(np.uint32), c[~finite].view(np.uint32))
    assert (np.abs(out[finite] - c[finite]) <= np.spacing(c[finite])).all()


@pytest.mark.parametrize("src,dst", [((9, 7), (18, 14)), ((13, 7), (37, 29)), ((16, 9), (11, 5))])
def test_guided_with_uniform_guides_is_bilinear(src, dst):
    ns, nd = src[0] * src[1], dst[0] * dst[1]
    rng = np.random.default_rng(ns)
    c, sa, da = rng.uniform(0, 3, (ns, 3)).astype(F), rng.uniform(0.1, 1, (ns, 3)).astype(F), rng.uniform(0.1, 1, (nd, 3)).astype(F)
    c[4, 2] = np.nan
    for flags in (0, ur.DEMODULATE_ALBEDO):
        b, bs, _ = ur.upsample(*src, *dst, ur.BILINEAR, 0, 0.0, flags, c, None, sa, None, da)
        for sharp, tol, match in ((0, 0.0, 0), (8, 0.05, ur.MATCH_ENTITY)):
            g, gs, _ = ur.upsample(*src, *dst, ur.GUIDED, sharp, tol, flags | match, c, _uniform_hits(ns), sa, _uniform_hits(nd), da)
            same = bs == 0                                   # where bilinear answered, guided gives its bits; where it did not (the NaN under all weight), B may
            assert np.array_equal(g[same].view(np.uint32), b[same].view(np.uint32)) and (gs[same] == 0).all()
            assert (gs[~same] >= 1).all()


def test_bilinear_reproduces_a_linear_ramp_in_the_interior():
    """colour = a + b x + c y at the src pixel centres: wherever all four taps are inside the image a bilinear read returns the ramp at the dst pixel centre, to 2 ulp
    of the frame's largest value.  In ulps of the single result the specified arithmetic (fx, 1 - fx, the weight, four products, three sums of each kind and the
    quotient, each rounded once) is exact at a ratio of 2 and up to 2.5 ulp off at the two other ratios, where fx itself is rounded; that figure is printed."""
    for (sw, sh), (dw, dh) in (((16, 12), (32, 24)), ((13, 7), (37, 29)), ((40, 30), (27, 19))):
        X, Y = np.tile(np.arange(sw), sh), np.repeat(np.arange(sh), sw)
        coef = np.array([(0.5, 0.125, 0.25), (1.0, 0.0625, 0.5), (2.0, 0.25, 0.03125)])
        c = np.stack([a + b * X + g * Y for a, b, g in coef], axis=1).astype(F)            # exact in float32: small dyadic numbers
        out, stage, _ = ur.upsample(sw, sh, dw, dh, ur.BILINEAR, 0, 0.0, 0, c)
        _, x0, _ = ur.axis_positions(sw, dw)
        _, y0, _ = ur.axis_positions(sh, dh)
        DX, DY = np.tile(np.arange(dw), dh), np.repeat(np.arange(dh), dw)
        inside = (x0[DX] >= 0) & (x0[DX] + 1 <= sw - 1) & (y0[DY] >= 0) & (y0[DY] + 1 <= sh - 1)
        assert inside.sum() > dw * dh // 2 and (stage == 0).all()
        sx, sy = (DX + 0.5) * sw / dw - 0.5, (DY + 0.5) * sh / dh - 0.5
        want = np.stack([a + b * sx + g * sy for a, b, g in coef], axis=1)
        err = np.abs(out[inside].astype(np.float64) - want[inside])
        print("ramp %dx%d -> %dx%d: %.3f ulp of the result at worst" % (sw, sh, dw, dh, (err / np.spacing(out[inside]).astype(np.float64)).max()))
        assert err.max() <= 2 * float(np.spacing(F(c.max())))


def _two_regions(w, h, edge, right):
    """guides of a frame split at column `edge` (in units of this frame's pixels): entity 1 left; right: another entity on the same plane, or sky"""
    col = np.tile(np.arange(w), h)
    t, e, n = _uniform_hits(w * h, entity=1)
    if right == "sky":
        e[col >= edge], t[col >= edge], n[col >= edge] = -1, np.inf, 0
    else:
        e[col >= edge] = 5
    return (t, e, n), col >= edge


@pytest.mark.parametrize("right", ["entity", "sky"])
def test_an_entity_edge_holds_exactly(right):
    """Changing every src colour right of the edge leaves every dst pixel whose guides lie left of it bit-identical, and the other way round: with MATCH_ENTITY no tap
    crosses, in stage A or B, and stage C is never needed because each region is at least 4 src pixels wide (some tap of the 4 x 4 block is always on the pixel's side).
    The planes are the same (distance, normal): only the entity - or the sky test - separates them, at any tolerance."""
    (sw, sh), (dw, dh) = (24, 10), (60, 25)
    s_edge, d_edge = 9, 20                                      # 9 / 24 = 0.375, 20 / 60 = 0.333: the dst columns 20 (taps 7, 8) and 21 lie beyond both inner taps' side
    rng = np.random.default_rng(17)
    c = rng.uniform(0, 2, (sw * sh, 3)).astype(F)
    src_hits, s_right = _two_regions(sw, sh, s_edge, right)
    dst_hits, d_right = _two_regions(dw, dh, d_edge, right)
    c_right, c_left = c.copy(), c.copy()
    c_right[s_right] = rng.uniform(50, 100, (int(s_right.sum()), 3))
    c_left[~s_right] = rng.uniform(50, 100, (int((~s_right).sum()), 3))
    for tol in (0.0, 0.05, 1e30):
        run = lambda col: ur.upsample(sw, sh, dw, dh, ur.GUIDED, 4, tol, ur.MATCH_ENTITY, col, src_hits, None, dst_hits, None)
        base, stage, _ = run(c)
        assert (stage <= 1).all() and (stage == 1).any()              # stage B holds the edge too
        x, _, _ = run(c_right)
        y, _, _ = run(c_left)
        assert np.array_equal(x[~d_right].view(np.uint32), base[~d_right].view(np.uint32)) and (x[d_right] >= 50).all()
        assert np.array_equal(y[d_right].view(np.uint32), base[d_right].view(np.uint32)) and (y[~d_right] >= 50).all()


def test_sky_and_surface_never_mix():
    """Sky src pixels are blue (0, 0, 1 .. 2), surface src pixels red (1 .. 2, 0, 0): in GUIDED mode, whatever the other parameters, a dst sky pixel answered by stage A
    or B has no red and a dst surface pixel no blue.  (Stage C copies the point pixel: it is the stage that admits there was nothing to take.)"""
    case = ur.make_case(48, 27, 96, 54, 5)
    se, de = case["src_hits"][1], case["dst_hits"][1]
    rng = np.random.default_rng(1)
    c = np.zeros((se.size, 3), F)
    c[se < 0, 2] = rng.uniform(1, 2, int((se < 0).sum()))
    c[se >= 0, 0] = rng.uniform(1, 2, int((se >= 0).sum()))
    for sharp, tol, flags in ((0, 1e30, 0), (4, 0.05, ur.MATCH_ENTITY), (8, 0.0, 0)):
        out, stage, _ = ur.upsample(48, 27, 96, 54, ur.GUIDED, sharp, tol, flags, c, case["src_hits"], None, case["dst_hits"], None)
        ab = stage <= 1
        sky, surf = ab & (de < 0), ab & (de >= 0)
        assert sky.sum() > 100 and surf.sum() > 1000
        assert (out[sky, 0] == 0).all() and (out[sky, 2] >= 1).all()
        assert (out[surf, 2] == 0).all() and (out[surf, 0] >= 1).all()


def _guided(configs):
    return [cfg for cfg in configs if cfg[0] == ur.GUIDED]


@pytest.mark.parametrize("src,dst", [p for p in ur.SIZE_PAIRS + [ur.LARGE_PAIR] if p[1][0] * p[1][1] >= ur.COVERAGE_MIN_PIXELS])
def test_the_generated_cases_cover_every_stage_and_rejection(src, dst):
    """What tests/test_gpu_upsample.py asserts again before it believes a comparison: in every GUIDED case of at least 1000 dst pixels each stage answers at least 2 % of
    the pixels and each rejection cause (the entity cause where MATCH_ENTITY makes it one) rejects a tap in at least 1 % of them."""
    case = ur.make_case(*src, *dst, ur.case_seed(src, dst))
    for cfg in _guided(ur.LARGE_CONFIGS if (src, dst) == ur.LARGE_PAIR else ur.CONFIGS):
        _, stage, rejected = ur.reference(case, *cfg)
        cov = ur.coverage(stage, rejected, cfg[3])
        print(src, dst, cfg, cov)
        assert ur.coverage_ok(cov), (src, dst, cfg, cov)


def test_the_generated_cases_carry_the_special_values():
    case = ur.make_case(48, 27, 96, 54, ur.case_seed((48, 27), (96, 54)))
    c = case["src_color"]
    assert np.isnan(c).any() and np.isposinf(c).any() and np.isneginf(c).any()
    for alb in (case["src_albedo"], case["dst_albedo"]):
        for val in (0.0, 2.0 ** -11, 2.0 ** -10):
            assert (alb == F(val)).any(), val
    se, de = case["src_hits"][1], case["dst_hits"][1]
    assert (se < 0).any() and (de < 0).any() and (se >= 100).any() and (de >= 300).any()
    sn, dn = case["src_hits"][2], case["dst_hits"][2]
    dots = sn[:-1] @ np.array([0, 0, 1], F)
    assert (dots > 0.9).any() and (dots < -0.9).any()
