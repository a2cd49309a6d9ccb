"""CPU: the numpy restatements of tests/postpass_reference.py equal the C++ oracle bit for bit on every case that tests/test_gpu_postpass_edges.py sends to the device,
and every case contains what it is named for (decided from the oracle and the restatement, never from a kernel)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import postpass_reference as pp  # noqa: E402

F, U = np.float32, np.uint32
FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]                 # (debugMode, ldrAlbedo)


def _same(got, want, what):
    for name, g, w in zip(("color", "normal", "albedo"), got, want):
        bad = np.flatnonzero((pp.bits(g).reshape(-1, 3) != pp.bits(w).reshape(-1, 3)).any(1))
        assert bad.size == 0, (what, name, bad[:5], g[bad[:3]], w[bad[:3]])


@pytest.mark.parametrize("w,h", pp.COMBINE_SHAPES)
def test_the_combine_restatement_is_the_oracle(oracle, w, h):
    for case in pp.combine_cases(w, h):
        for debug, ldr in FLAGS:
            want = oracle.combine(w, h, case["color"], case["normal"], case["albedo"], debug_mode=bool(debug), ldr_albedo=bool(ldr))
            _same(pp.combine(w, h, case["color"], case["normal"], case["albedo"], bool(debug), bool(ldr)), want, (case["name"], debug, ldr))


def _counts(case):
    return pp.truncate(case["color"][:, 3]).reshape(case["h"], case["w"])


@pytest.mark.parametrize("w,h", [s for s in pp.COMBINE_SHAPES if s != (1, 1)])
def test_every_combine_case_contains_what_it_is_named_for(oracle, w, h):
    cases = {c["pattern"]: c for c in pp.combine_cases(w, h)}
    assert sorted(cases) == sorted(pp.PATTERNS)
    n = w * h
    magenta, black = F([1, 0, 1]), F([0, 0, 0])
    seen_w, seen_counts, nan_sampled, nan_empty, seen_kinds = set(), set(), 0, 0, np.zeros(11, np.int64)
    for pattern, case in cases.items():
        own = _counts(case)
        plain = oracle.combine(w, h, case["color"], case["normal"], case["albedo"])[0].reshape(h, w, 3)
        debug = oracle.combine(w, h, case["color"], case["normal"], case["albedo"], debug_mode=True)[0].reshape(h, w, 3)
        row, count = pp.walk(w, h, case["color"])
        assert ((debug == magenta).all(2) == (own == 0)).all(), "debug mode: magenta exactly where the pixel itself has no samples, no borrowing"
        if pattern == "row0":
            assert (own[0] != 0).all() and (own[1:] == 0).all() and (row == 0).all()                 # every other pixel borrows across its whole column
            poisoned = np.isnan(case["color"][:w, :3]).any(1)
            assert (poisoned.any() or w == 1) and not poisoned.all()
            assert (plain[:, poisoned] == black).all() and (plain[:, ~poisoned] != black).any(2).all(), "a look-around that lands on a NaN pixel gives black"
        if pattern == "last_row":
            assert (own[-1] != 0).all() and (own[:-1] == 0).all()
            assert (count[:-1] == 0).all() and (plain[:-1] == black).all(), "nothing below to borrow from: every walk leaves the image"
        if pattern == "rows_mod2":
            assert ((own != 0) == (np.arange(h)[:, None] % 2 == 0)).all()
            if h > 1:
                assert (row[1] == 0).all() and (count[1] == own[0]).all()
            if (w, h) == (257, 3):
                assert ((w + np.arange(w)) // 256 != np.arange(w) // 256).sum() >= 255, "row 1 reads row 0 from another workgroup of 256 pixels"
        if pattern == "empty_columns":
            assert (own[:, ::3] == 0).all() and (count[:, ::3] == 0).all() and (plain[:, ::3] == black).all(), "a column with no samples anywhere"
            if w > 1:
                assert (own[:, 1] != 0).any()
        # what is drawn per pixel: counted over the five frames of the shape
        final = count.reshape(n)
        seen_w |= set(case["color"][:, 3].tolist())
        seen_counts |= set(final.tolist())
        sampled, zero = case["color"][own.reshape(n) != 0], case["color"][own.reshape(n) == 0]
        nan_sampled, nan_empty = nan_sampled + int(np.isnan(sampled[:, :3]).any()), nan_empty + int(np.isnan(zero[:, :3]).any())
        with np.errstate(all="ignore"):
            length = pp.squared_length(case["normal"] / np.maximum(final, 1).astype(F)[:, None])
        kinds = [length == 0, length == pp.FLT_MIN, length == np.nextafter(pp.FLT_MIN, F(1)), (length > 0) & (length < pp.FLT_MIN), np.isinf(length), np.isnan(length)]
        out = oracle.combine(w, h, case["color"], case["normal"], case["albedo"])
        assert (out[1][length == pp.FLT_MIN] == 0).all() and (out[1][length == np.nextafter(pp.FLT_MIN, F(1))] != 0).any(1).all(), "FLT_MIN is not above the threshold, its neighbour is"
        assert (out[1][~(length > pp.FLT_MIN)] == 0).all() and (out[1][np.isinf(length)] == 0).all()
        alb, ldr = out[2], oracle.combine(w, h, case["color"], case["normal"], case["albedo"], ldr_albedo=True)[2]
        kinds += [alb == 1, alb == np.nextafter(F(1), F(2)), alb > 2, np.isnan(alb), alb < 0]
        seen_kinds = seen_kinds + np.array([int(k.sum()) for k in kinds])
        assert (ldr[np.isnan(alb)] == 1).all() and (ldr[alb > 1] == 1).all() and np.array_equal(pp.bits(ldr[alb <= 1]), pp.bits(alb[alb <= 1])), "min(x, 1): a NaN becomes 1"
    assert (seen_kinds >= 3).all(), ("normals at the threshold of normalizesafe (0, FLT_MIN, one ulp above, denormal, +inf, NaN), albedos round 1 (1, one ulp above, 3, NaN, -1)", seen_kinds)
    assert seen_w >= set(np.concatenate([pp.W_SAMPLED, pp.W_EMPTY]).tolist()) and seen_counts >= {0, 1, 2, -3, 2 ** 24, 2 ** 30}, "every w of the lists, borrowed ones included"
    assert nan_sampled >= 1 and nan_empty >= 1, "NaN in r, g or b of pixels with and without samples"


def test_the_single_pixel_cases_cover_the_lists(oracle):
    cases = pp.single_pixel_cases()
    assert {float(c["color"][0, 3]) for c in cases} >= set(np.concatenate([pp.W_SAMPLED, pp.W_EMPTY]).tolist())
    assert {c["normal"].tobytes() for c in cases} >= {pp.NORMAL_EDGES[k:k + 1].tobytes() for k in range(len(pp.NORMAL_EDGES))}
    assert {c["albedo"][0, :1].tobytes() for c in cases} >= {pp.ALBEDO_EDGES[k:k + 1].tobytes() for k in range(len(pp.ALBEDO_EDGES))}
    by_name = {c["name"]: c for c in cases}
    c = by_name["1x1-w4"]                                 # w = -3: the colour is divided by -3, the guides by 1
    assert c["color"][0, 3] == -3
    color, normal, albedo = oracle.combine(1, 1, c["color"], c["normal"], c["albedo"])
    assert np.array_equal(color[0], c["color"][0, :3] / F(-3)) and np.array_equal(albedo[0], c["albedo"][0]) and np.array_equal(normal[0], F([0, 0.6, -0.8]))
    for name, want in (("1x1-w9", [0, 0, 0]), ("1x1-nan-sampled", [0, 0, 0]), ("1x1-nan-empty", [0, 0, 0])):      # w = 0.9 is no samples
        c = by_name[name]
        assert np.array_equal(oracle.combine(1, 1, c["color"], c["normal"], c["albedo"])[0][0], F(want)), name
    c = by_name["1x1-nan-empty"]
    assert np.array_equal(oracle.combine(1, 1, c["color"], c["normal"], c["albedo"], debug_mode=True)[0][0], F([1, 0, 1])), "no samples is asked before NaN"
    c = by_name["1x1-nan-sampled"]
    assert np.array_equal(oracle.combine(1, 1, c["color"], c["normal"], c["albedo"], debug_mode=True)[0][0], F([0, 1, 1]))


@pytest.fixture(scope="module")
def operands(oracle):
    return pp.finalize_operands(oracle)


def _byte(oracle, v):
    frame = np.zeros((v.size, 3), F)
    frame[:, 0] = v
    return oracle.finalize(frame, np.zeros_like(frame), np.zeros_like(frame))[0][:, 0]


def test_the_finalize_operands_sit_on_every_byte_step(oracle, operands):
    first = pp.first_floats_of_each_byte(oracle)
    at = first.astype(U).view(F)
    below = (first - 1).astype(U).view(F)
    assert np.array_equal(_byte(oracle, at), np.arange(1, 256)) and np.array_equal(_byte(oracle, below), np.arange(0, 255)), "the first float of byte k, and the last of k - 1"
    assert np.all(np.diff(first) > 16), "the 17 floats round one step do not reach the next"
    got = _byte(oracle, operands)
    assert set(got.tolist()) == set(range(256)), "the threshold case hits all 256 byte values"
    near = operands[:255 * 17].reshape(255, 17)
    assert np.array_equal(pp.bits(near[:, 8]), first.astype(U)) and np.all(np.diff(pp.bits(near).astype(np.int64), axis=1) == 1)
    b = got[:255 * 17].reshape(255, 17)
    k = np.arange(1, 256)[:, None]
    assert (b[:, 7:8] == k - 1).all() and (b[:, 8:9] == k).all() and ((b == k - 1) | (b == k)).all()
    # the oracle's pow is not monotone from float to float (at step 182 a float of byte 182 lies below two of byte 181): a bisection finds a crossing, and the floats
    # round it are where a table of thresholds and a pow can disagree - hence all 17
    assert ((b[:, :8] == k - 1).all(1) & (b[:, 8:] == k).all(1)).sum() >= 250
    special = operands[255 * 17:]
    assert np.isnan(special).any() and np.isinf(special).sum() == 2 and (special < 0).any() and ((special != 0) & (np.abs(special) < pp.FLT_MIN)).any()
    assert np.signbit(special[special == 0]).tolist() == [False, True]


def test_the_finalize_frame_places_every_operand_in_nine_positions(oracle, operands):
    color, normal, albedo = pp.finalize_frame(operands)
    nrm, exact = pp.normal_of(operands)
    n = operands.size
    assert color.shape == normal.shape == albedo.shape == (n, 3)
    for j in range(3):
        assert np.array_equal(pp.bits(np.roll(color[:, j], j)), pp.bits(operands)) and np.array_equal(pp.bits(np.roll(albedo[:, j], 3 + j)), pp.bits(operands))
        lane = np.roll(normal[:, j], 6 + j)
        with np.errstate(all="ignore"):
            back = (lane * F(0.5) + F(0.5)).astype(F)
        assert np.array_equal(pp.bits(back[exact]), pp.bits(operands[exact])), "the normal lane's operand is the float itself, exactly"
        assert (lane[~exact] == 0).all()
    assert exact.mean() > 0.4 and exact[:255 * 17].reshape(255, 17).any(1).sum() > 200, "most steps keep operands in the normal lane"
    # w = 1: combine is the identity on colour (where no channel is NaN) and on albedo, so the fused pass converts these very operands
    c4 = np.concatenate([color, np.ones((n, 1), F)], 1)
    cc, cn, ca = oracle.combine(n, 1, c4, normal, albedo)
    clean = ~np.isnan(color).any(1)
    assert np.array_equal(pp.bits(cc[clean]), pp.bits(color[clean])) and np.array_equal(pp.bits(ca), pp.bits(albedo)) and (cc[~clean] == 0).all()


def _cases():
    return [pp.metrics_frame(n) for n in pp.METRICS_COUNTS] + pp.metrics_edge_cases()


@pytest.fixture(scope="module")
def metrics_cases():
    return {c["name"]: c for c in _cases()}


def test_the_metrics_restatement_is_the_oracle(oracle, metrics_cases):
    for name, c in metrics_cases.items():
        for diag in (c["diag"], np.ascontiguousarray(c["diag"][:, :1])):
            want = pp.record_of(oracle.reduce_metrics(diag, c["color"], c["scw"]))
            assert pp.reduce_metrics(diag, c["color"], c["scw"]).tobytes() == want.tobytes(), (name, diag.shape[1], want)


def test_every_metrics_case_contains_what_it_is_named_for(oracle, metrics_cases):
    rec = {name: pp.record_of(oracle.reduce_metrics(c["diag"], c["color"], c["scw"]))[0] for name, c in metrics_cases.items()}
    assert sorted(c["n"] for name, c in metrics_cases.items() if name.startswith("frame-")) == pp.METRICS_COUNTS
    for c in metrics_cases.values():
        assert np.isnan(c["diag"][:, 1:]).all(), "junk behind each count"
    r = rec["rays-wrap-negative"]
    assert 2 ** 31 < r["totalRayCount64"] < 2 ** 32 and r["totalRayCount"] == r["totalRayCount64"] - 2 ** 32 < 0 and r["totalSamples"] == r["totalSamples64"]
    r = rec["samples-wrap-negative"]
    assert 2 ** 31 < r["totalSamples64"] < 2 ** 32 and r["totalSamples"] == r["totalSamples64"] - 2 ** 32 < 0 and r["totalRayCount"] == r["totalRayCount64"]
    r = rec["rays-wrap-positive"]
    assert r["totalRayCount64"] > 2 ** 32 and r["totalRayCount"] != r["totalRayCount64"] and r["totalRayCount"] == r["totalRayCount64"] - 2 ** 32 > 0
    assert r["totalSamples"] == r["totalSamples64"] and metrics_cases["rays-wrap-positive"]["diag"][:, 0].max() == 2e9
    r = rec["samples-wrap-positive"]
    assert r["totalSamples64"] > 2 ** 32 and r["totalSamples"] == r["totalSamples64"] - 2 ** 32 > 0 and r["totalRayCount"] == r["totalRayCount64"]
    assert r["sampleCountExtrema"][1] == 2 * 10 ** 9
    r = rec["both-wrap"]
    assert r["totalRayCount"] == r["totalRayCount64"] - 2 ** 32 and r["totalSamples"] == r["totalSamples64"] - 2 ** 33 < 0 and r["totalRayCount"] != r["totalSamples"]
    assert (metrics_cases["negative-rays"]["diag"][:, 0] < 0).sum() > 100 and rec["negative-rays"]["totalRayCount64"] < 0
    for name in ("all-weights-nan-1", "all-weights-nan-257"):
        assert np.isnan(pp.weights(metrics_cases[name]["color"], metrics_cases[name]["scw"])).all()
        assert rec[name]["sampleCountWeightExtrema"].tolist() == [np.inf, -np.inf] and rec[name]["sampleCountExtrema"].tolist() == [0, 0]
    c = metrics_cases["one-finite-weight"]
    w = pp.weights(c["color"], c["scw"])
    assert np.isfinite(w).sum() == 1 and np.isnan(w).sum() == 256 and rec["one-finite-weight"]["sampleCountWeightExtrema"].tolist() == [F(2.5 / 8)] * 2
    c = metrics_cases["nan-and-inf-weights"]
    assert np.isnan(c["scw"]).sum() > 50 and np.isinf(c["scw"]).sum() > 50
    r = rec["nan-and-inf-weights"]["sampleCountWeightExtrema"]
    assert np.isfinite(r[0]) and r[1] == np.inf
    c = metrics_cases["empty-pixels-with-weight"]
    empty = c["color"][:, 3] == 0
    assert empty.sum() > 50 and (c["scw"][empty] > 0).all() and rec["empty-pixels-with-weight"]["sampleCountWeightExtrema"][1] == np.inf
    assert rec["empty-pixels-with-weight"]["sampleCountExtrema"][0] == 0
    # the frames: every kind of pixel from 255 pixels on
    for n in pp.METRICS_COUNTS[1:]:
        c = metrics_cases["frame-%d" % n]
        w = pp.weights(c["color"], c["scw"])
        assert (c["diag"][:, 0] < 0).any() and np.isnan(c["scw"]).any() and np.isnan(w).any() and np.isinf(w).any() and (c["color"][:, 3] == 0).any(), n
    # one pixel: 2047 of the 2048 partial results are the start value of the fold
    c, r = metrics_cases["frame-1"], rec["frame-1"]
    assert c["n"] == 1 and r["sampleCountExtrema"][0] == r["sampleCountExtrema"][1] == r["totalSamples"] > 0 and r["sampleCountWeightExtrema"][0] == r["sampleCountWeightExtrema"][1]
    # beyond one round of the grid: without the tail every field of the record is another
    c = metrics_cases["frame-%d" % pp.METRICS_COUNTS[-1]]
    g = pp.GRID_LANES
    assert c["n"] > g
    whole, head = rec[c["name"]], pp.record_of(oracle.reduce_metrics(c["diag"][:g], c["color"][:g], c["scw"][:g]))[0]
    for field in ("totalRayCount", "totalSamples", "totalRayCount64", "totalSamples64"):
        assert whole[field] != head[field], field
    for field in ("sampleCountWeightExtrema", "sampleCountExtrema"):
        assert whole[field][0] != head[field][0] and whole[field][1] != head[field][1], field


def test_the_largest_frame_is_beyond_the_grid_of_the_reduction():
    """reduce_metrics_kernel runs kMetricsBlocks workgroups of 256 lanes: the largest pixel count sends 257 lanes round their loop a second time"""
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracing-in-one-weekend_amd", "csrc", "rtow_kernels.h")).read()
    blocks = re.search(r"constexpr int kMetricsBlocks = (\d+);", header)
    assert blocks and int(blocks.group(1)) * 256 == pp.GRID_LANES and pp.METRICS_COUNTS[-1] == pp.GRID_LANES + 257


def test_wrap32_and_truncate():
    assert pp.wrap32(2 ** 31) == -2 ** 31 and pp.wrap32(2 ** 32 + 5) == 5 and pp.wrap32(-2 ** 31 - 1) == 2 ** 31 - 1 and pp.wrap32(-7) == -7
    assert pp.truncate(F([0.9, 1.9, -0.5, -3.7, 2.0 ** 30, -0.0])).tolist() == [0, 1, 0, -3, 2 ** 30, 0]
    for bad in (np.nan, np.inf, 2.0 ** 31, -2.0 ** 31):
        with pytest.raises(AssertionError):
            pp.truncate(F([bad]))
