"""Synthetic inputs for the tests of rtowReprojectAccumBilinearDevice, shared by the CPU test that checks their coverage with the restatement alone and the GPU
test that runs them: tests/test_gpu_reproject.py's make_case (two views a small step apart, a plane, random hits, misses, sky, points behind the camera, rays on
the image-plane edges, accumulators with every kind of sample count and non-finite channels) with a mix of sample counts that leaves every number of valid taps
common, plus moments, rays whose reprojected point has a whole gx or gy (a tap of weight 0), and rays within half a pixel of each image border (x0 = -1,
x0 + 1 = W).  A helper of the tests, not a test."""
import numpy as np

import reproject_bilinear_reference as rb
import reproject_reference as rr
from test_gpu_reproject import CONFIGS, make_case  # noqa: F401

F = np.float32
SIZES = [(1, 1), (2, 2), (8, 8), (9, 7), (41, 29), (96, 54), (257, 3)]
MAX_BATCHES = (1, 16)


def _fx_fy(case, d):
    """(fx, fy) of sky rays with directions d (m, 3) through the restatement's steps 1 and 2"""
    m = d.shape[0]
    inside, fx, fy, _ = rb.project(case["w"], case["h"], case["va"], np.zeros((m, 3), F), d, np.full(m, np.inf, F), np.full(m, -1, np.int32))
    return inside, fx, fy


def _aim(case, u, v):
    """direction of the ray through (u, v) of the previous view's image plane"""
    va = case["va"]
    return ((va["lowerLeftCorner"] + F(u) * va["horizontal"]) + F(v) * va["vertical"]).astype(F)


def _aim_whole(case, axis, target, other):
    """A direction whose fx (axis 0) or fy (axis 1) is exactly target + 0.5, so that gx or gy is whole: the plane coordinate is scanned ulp by ulp around its
    solution until the float32 chain of steps 1 and 2 lands on the value.  None if no neighbour does."""
    size = (case["w"], case["h"])[axis]
    centre = np.array([(target + 0.5) / size], F).view(np.int32)[0]
    coords = (centre + np.arange(-256, 257)).astype(np.int32).view(F)
    d = np.stack([_aim(case, c, other) if axis == 0 else _aim(case, other, c) for c in coords])
    inside, fx, fy = _fx_fy(case, d)
    hit = np.flatnonzero(inside & ((fx, fy)[axis] == F(target + 0.5)))
    return d[hit[0]] if hit.size else None


def make_bilinear_case(w, h, seed, max_history, max_batches, variant=0):
    """make_case plus: 30 % of the accumulators unusable (so that one, two and three valid taps are as common as four), moments, aimed sky rays (see the module's
    text) whose taps' previous pixels are made sky, so that those taps can be valid."""
    case = make_case(w, h, seed, max_history, variant)
    rng = np.random.default_rng(seed + 977)
    n = case["n"]
    prev = case["prev"]
    dead = rng.random(n) < 0.30
    half = dead & (rng.random(n) < 0.5)
    for k in rb.KEYS:
        prev[k][dead] = 0
    prev["color"][half, 3] = F(0.5)
    mb = float(max_batches)
    counts = np.array([0, 0.5, 1, 2, mb, mb + 1, np.nan], F)
    msel = counts[rng.choice(7, n, p=[0.08, 0.08, 0.2, 0.2, 0.2, 0.2, 0.04])]
    mean = rng.uniform(0, 2, n)
    with np.errstate(all="ignore"):
        case["moments"] = np.stack([mean * msel, (mean * mean + rng.uniform(0, 1, n)) * msel, msel], axis=1).astype(F)
    case["moments"][rng.integers(0, n, max(1, n // 53)), rng.integers(0, 2, max(1, n // 53))] = np.inf
    aimed = []
    if n >= 48:
        for axis in (0, 1):
            size = (w, h)[axis]
            for target in sorted({0, size // 2, size - 2}):
                d = _aim_whole(case, axis, target, float(rng.uniform(0.2, 0.8)))
                if d is not None:
                    aimed.append(d)
        for u, v in ((0.25 / w, 0.4), (1 - 0.25 / w, 0.6), (0.3, 0.25 / h), (0.7, 1 - 0.25 / h), (0.25 / w, 0.25 / h), (1 - 0.25 / w, 1 - 0.25 / h)):
            aimed.append(_aim(case, u, v))
        at = rng.choice(n, len(aimed), replace=False)
        for i, d in zip(at, aimed):
            case["d"][i], case["t"][i], case["e"][i] = d, np.inf, -1
        case["rays"]["direction"] = case["d"]
        inside, fx, fy, _ = rb.project(w, h, case["va"], case["o"][at], case["d"][at], case["t"][at], case["e"][at])
        q, _, usable = rb.taps(w, h, inside, fx, fy)
        sky = np.unique(q[usable])
        case["pe"][sky], case["pt"][sky] = -1, np.inf
    case["aimed"] = len(aimed)
    return case


def reference(case, flags, tol, max_history, max_batches=None):
    m = case["moments"] if max_batches is not None else None
    return rb.reproject_bilinear(case["w"], case["h"], case["va"], case["o"], case["d"], case["t"], case["e"], case["pt"], case["pe"], case["prev"], tol, max_history,
                                 flags, m, max_batches)


def seed_of(w, h, k, variant=0):
    return 1000 * w + 10 * h + k + 65537 * variant


def zero_weight_taps(case):
    """how many taps inside the image have weight exactly 0"""
    inside, fx, fy, _ = rb.project(case["w"], case["h"], case["va"], case["o"], case["d"], case["t"], case["e"])
    q, b, usable = rb.taps(case["w"], case["h"], inside, fx, fy)
    return int((inside[None, :] & (b == 0)).sum())
