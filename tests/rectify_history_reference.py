"""numpy float32 restatement of rtowRectifyHistoryDevice (include/rtow.h): a pixel's carried history against the mean and the variance of the fresh samples
in its guide-weighted neighbourhood - kept, cut down to trunc(h.w / r) samples, or dropped.  Vectorised over pixels with the tap loop in the specification's order
(j outer, i inner); every operation is one float32 operation of the specification - no contraction, correctly rounded division, no sqrt / exp / pow - so the result
is the kernel's, bit for bit.  It shares nothing with the product and nothing with the other restatements: the luminance and the guide weight are written out here.
Also the generator of the random inputs the CPU and GPU tests share.  A helper of the tests, not a test."""
import numpy as np

F = np.float32
MATCH_ENTITY = 1
UNJUDGED, KEPT, CUT, DROPPED = 0, 1, 2, 3
KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))


def lum(x, y, z):
    return (F(0.2126) * x + F(0.7152) * y) + F(0.0722) * z


def guide_weight(e, t, n, e2, t2, n2, normal_sharpness, depth_tolerance, match):
    """g(p, q): e, t, n the pixel's guides, e2, t2, n2 the tap's (arrays of one shape; n, n2 with a last axis of 3)"""
    tol = F(depth_tolerance)
    sky = e < 0
    near = np.abs(t2 - t) <= tol * t                                   # NaN fails
    d = (n[..., 0] * n2[..., 0] + n[..., 1] * n2[..., 1]) + n[..., 2] * n2[..., 2]
    d = np.where(d > 0, d, F(0)).astype(F)
    for _ in range(normal_sharpness):
        d = d * d
    compared = ~sky & (e2 >= 0) & ~(bool(match) & (e2 != e)) & near
    return np.where(sky, np.where(e2 < 0, F(1), F(0)), np.where(compared, d, F(0))).astype(F)


def luminance(color):
    """L(q): (l, valid) over an array of float4 colour sums"""
    c = np.ascontiguousarray(color, F)
    w = c[..., 3]
    l = lum(c[..., 0] / w, c[..., 1] / w, c[..., 2] / w).astype(F)
    return l, (w > 0) & np.isfinite(l)                                 # a NaN w fails w > 0


def rectify(width, height, history, fresh, hits, moments, radius, min_taps, normal_sharpness, depth_tolerance, sigma_scale, relative_tolerance, flags):
    """rtowRectifyHistoryDevice.  history: {"color" (n, 4), "normal" (n, 3), "albedo" (n, 3), "scw" (n,)}; fresh (n, 4); hits = (distance, entityIndex, normal);
    moments (n, 3) or None.  -> {"color", "normal", "albedo", "scw", "moments" (or None), "keep" (n,), "stats" (4,) uint32: judged, kept, cut, dropped,
    "outcome" (n,): UNJUDGED / KEPT / CUT / DROPPED}"""
    h, w = height, width
    n = h * w
    with np.errstate(all="ignore"):
        hc = np.ascontiguousarray(history["color"], F).reshape(n, 4)
        hw = hc[:, 3]
        lh = lum(hc[:, 0] / hw, hc[:, 1] / hw, hc[:, 2] / hw).astype(F)
        history_valid = np.isfinite(hc).all(axis=1) & (hw >= 1) & np.isfinite(lh)
        t, e, nrm = hits
        t = np.ascontiguousarray(t, F).reshape(h, w)
        e = np.ascontiguousarray(e, np.int32).reshape(h, w)
        nrm = np.ascontiguousarray(nrm, F).reshape(h, w, 3)
        l, valid = luminance(np.ascontiguousarray(fresh, F).reshape(h, w, 4))
        W, S1, S2 = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
        taps = np.zeros((h, w), np.int32)
        match = bool(flags & MATCH_ENTITY)
        for j in range(-radius, radius + 1):
            for i in range(-radius, radius + 1):
                y0, y1, x0, x1 = max(0, -j), min(h, h - j), max(0, -i), min(w, w - i)
                if y0 >= y1 or x0 >= x1:
                    continue                                           # every tap of this offset lies outside the image
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + j, y1 + j), slice(x0 + i, x1 + i))
                if i == 0 and j == 0:
                    wgt = np.ones(l[P].shape, F)                       # the centre: w = 1, no guide consulted (its own L is checked below)
                else:
                    wgt = guide_weight(e[P], t[P], nrm[P], e[Q], t[Q], nrm[Q], normal_sharpness, depth_tolerance, match)
                lq = l[Q]
                take = valid[Q] & (wgt > 0)                            # skipped taps add nothing (not + 0)
                W[P] = np.where(take, W[P] + wgt, W[P])
                S1[P] = np.where(take, S1[P] + wgt * lq, S1[P])
                S2[P] = np.where(take, S2[P] + wgt * (lq * lq), S2[P])
                taps[P] += take
        mu, b = (S1 / W).reshape(n), (S2 / W).reshape(n)
        judged = history_valid & valid.reshape(n) & (taps.reshape(n) >= min_taps) & np.isfinite(mu) & np.isfinite(b)
        var = b - mu * mu
        var = np.where(var > 0, var, F(0)).astype(F)
        K2, R2 = F(sigma_scale) * F(sigma_scale), F(relative_tolerance) * F(relative_tolerance)
        d = lh - mu
        T = (K2 * var + R2 * (mu * mu)) + F(2.0 ** -20)
        r = (d * d) / T
        outside = judged & (r > 1)                                     # a NaN r keeps
        m = hw / r
        new_w = np.trunc(m).astype(F)
        cut = outside & (new_w >= 1)
        dropped = outside & ~cut
        k = (new_w / hw).astype(F)
    outcome = np.full(n, UNJUDGED, np.int32)
    outcome[judged] = KEPT
    outcome[cut] = CUT
    outcome[dropped] = DROPPED
    out = {}
    with np.errstate(all="ignore"):
        for key, width_ in KEYS + ((("moments", 3),) if moments is not None else ()):
            src = np.ascontiguousarray(moments if key == "moments" else history[key], F).reshape(n, width_)
            res = src.copy()                                           # unchanged pixels keep their bits
            res[cut] = (src[cut] * k[cut, None]).astype(F)
            res[dropped] = F(0)
            out[key] = res
        out["color"][cut, 3] = new_w[cut]
    out["scw"] = out["scw"].reshape(n)
    if moments is None:
        out["moments"] = None
    keep = np.ones(n, F)
    keep[cut] = k[cut]
    keep[dropped] = F(0)
    out["keep"] = keep
    counts = [int((outcome == o).sum()) for o in (KEPT, CUT, DROPPED)]
    out["stats"] = np.array([sum(counts)] + counts, np.uint32)
    out["outcome"] = outcome
    return out


# ---- the random inputs of the GPU tests (and of their coverage condition, which is checked on the CPU) ----
# one pixel, smaller than a halo, exactly one tile, a tile plus a column and a row, several tiles with ragged edges
SIZES = [(1, 1), (3, 2), (64, 4), (65, 5), (70, 10), (131, 9)]
# (radius, minTaps, normalSharpness, depthTolerance, sigmaScale, relativeTolerance, flags): every radius with MATCH_ENTITY on and off; minTaps 2, 12 of 25 and 49 of 49;
# sharpness 0 and 8; depth tolerance 0; both band terms alone, and both zero (T = 2^-20: nearly every judged pixel is cut or dropped)
CONFIGS = [(1, 2, 2, 0.05, 1.0, 0.125, 1), (2, 12, 0, 0.25, 2.0, 0.0, 0), (3, 2, 8, 0.0, 0.0, 0.5, 1), (3, 49, 0, 1.0, 1.0, 0.125, 0), (2, 4, 4, 0.05, 0.0, 0.0, 1),
           (1, 3, 0, 1.0, 1.5, 0.25, 0)]
# the configurations under which every case of at least 256 pixels shows every outcome on 5 % of its pixels (tests/test_rectify_history_reference.py)
COVERED = (0, 1, 2, 5)
TILE_W, TILE_H = 64, 4


def case_seed(w, h):
    return 2003 * w + 29 * h


def make_case(w, h, seed, holes="tile"):
    """Inputs of one call.  Guides as the temporal-moments cases: a few rectangular entity regions (entities 0..4) with sky blocks (-1, +inf, zero normal), per region a
    base distance and normal with a little curvature; pixels far off, normals of exactly zero on surfaces, a few NaN distances.  Fresh colour: sums over w = 1 .. 4
    samples of the region's colour with 30 % noise, with w = 0, 0.5, NaN and negative and non-finite channels.  History: sample counts 0 (a hole: all 11 floats and the
    moments zero), 0.5, 1, 2, 7, 64; its mean the region's colour times a factor near 1 (kept), 1.5 to 2.5 (cut where the count is large, dropped where it is
    small) or 4 to 10 (dropped unless the count is large); NaN and infinite channels.  holes: "tile" makes the 64 x 4 tile at (64, 0) - the second of the bottom row,
    whatever part of it the frame has - a tile of holes next to tiles with history; "all" makes every pixel a hole."""
    rng = np.random.default_rng(seed)
    n = w * h
    bx, by = max(1, min(4, w // 8)), max(1, min(3, h // 4))
    nc = bx * by
    ent = rng.integers(0, 5, nc)
    ent[rng.random(nc) < 0.2] = -1
    if nc == 1:
        ent[0] = -1 if seed % 5 == 0 else 2
    dist = rng.choice(np.array([1.0, 2.0, 4.0, 8.0]), nc)
    axes = np.array([(0, 0, 1), (1, 0, 0), (0, 1, 0), (0.6, 0, 0.8), (0, -0.8, 0.6)], np.float64)
    nrm = axes[rng.integers(0, len(axes), nc)]
    X, Y = np.tile(np.arange(w), h), np.repeat(np.arange(h), w)
    cell = np.minimum((Y * by) // h, by - 1) * bx + np.minimum((X * bx) // w, bx - 1)
    e = ent[cell].astype(np.int32)
    t = dist[cell].astype(F)
    nn = nrm[cell] + rng.normal(0, 0.05, (n, 3))
    nn = (nn / np.linalg.norm(nn, axis=1)[:, None]).astype(F)
    t = np.where(rng.random(n) < 0.5, t, (t * (1 + rng.uniform(-0.04, 0.04, n))).astype(F)).astype(F)
    pick = lambda share: rng.random(n) < share
    far = pick(0.04)
    t[far] = t[far] * F(16)
    t[pick(0.01)] = np.nan
    nn[pick(0.05)] = 0                                                 # a surface whose normal is exactly zero: n.n' = 0
    sky = e < 0
    t[sky], nn[sky] = np.inf, 0
    base = rng.uniform(0.2, 2.0, (nc, 3))[cell]
    cw = rng.integers(1, 5, n).astype(F)
    fresh = np.concatenate([np.abs(base * (1 + 0.3 * rng.normal(size=(n, 3)))) * cw[:, None], cw[:, None]], axis=1).astype(F)
    fresh[pick(0.04), 3] = 0
    fresh[pick(0.03), 3] = 0.5
    fresh[pick(0.02), 3] = np.nan
    fresh[pick(0.02), 3] = -1
    for val in (np.inf, -np.inf, np.nan):
        idx = np.flatnonzero(pick(0.015))
        fresh[idx, rng.integers(0, 3, idx.size)] = val
    hw = rng.choice(np.array([0, 0.5, 1, 2, 7, 64], F), n, p=[0.1, 0.04, 0.08, 0.12, 0.26, 0.4])
    kind = rng.random(n)
    factor = np.where(kind < 0.35, rng.uniform(0.95, 1.05, n), np.where(kind < 0.8, rng.uniform(1.5, 2.5, n), rng.uniform(4, 10, n)))
    color = np.concatenate([base * factor[:, None] * hw[:, None], hw[:, None]], axis=1).astype(F)
    normal = (nn * hw[:, None] + rng.normal(0, 0.01, (n, 3))).astype(F)
    albedo = (rng.uniform(0.1, 0.9, (nc, 3))[cell] * hw[:, None]).astype(F)
    scw = (rng.uniform(0, 1, n) * hw).astype(F)
    cnt = np.minimum(hw, 16).astype(F)                                 # batches carried
    mean = lum(*(base * factor[:, None]).astype(F).T)
    moments = np.stack([mean * cnt, (mean * mean + F(0.01)) * cnt, cnt], axis=1).astype(F)
    for val in (np.inf, -np.inf, np.nan):
        idx = np.flatnonzero(pick(0.015))
        color[idx, rng.integers(0, 4, idx.size)] = val                 # an invalid history
        idx = np.flatnonzero(pick(0.01))
        normal[idx, rng.integers(0, 3, idx.size)] = val                # carried as it is: copied, or multiplied by k
        idx = np.flatnonzero(pick(0.01))
        moments[idx, rng.integers(0, 3, idx.size)] = val
    hole = hw == 0
    if holes == "tile":
        hole |= (X >= TILE_W) & (X < 2 * TILE_W) & (Y < TILE_H)
    elif holes == "all":
        hole[:] = True
    color[hole], normal[hole], albedo[hole], scw[hole], moments[hole] = 0, 0, 0, 0, 0
    return {"w": w, "h": h, "n": n, "history": {"color": color, "normal": normal, "albedo": albedo, "scw": scw}, "fresh": fresh, "hits": (t, e, nn),
            "moments": moments, "hole": hole}


def reference(case, cfg, moments=True):
    return rectify(case["w"], case["h"], case["history"], case["fresh"], case["hits"], case["moments"] if moments else None, *cfg)


def shares(outcome):
    """the share of the pixels with each outcome: (unjudged, kept, cut, dropped)"""
    return tuple(float((outcome == o).mean()) for o in (UNJUDGED, KEPT, CUT, DROPPED))


def tiles_without_and_with_history(case):
    """(tiles of the 64 x 4 grid none of whose pixels has a valid history, tiles with one) - the kernel's early-out decision, restated"""
    w, h = case["w"], case["h"]
    with np.errstate(all="ignore"):
        c = case["history"]["color"]
        lh = lum(c[:, 0] / c[:, 3], c[:, 1] / c[:, 3], c[:, 2] / c[:, 3])
        valid = (np.isfinite(c).all(axis=1) & (c[:, 3] >= 1) & np.isfinite(lh)).reshape(h, w)
    without, with_ = [], []
    for ty in range(0, h, TILE_H):
        for tx in range(0, w, TILE_W):
            (with_ if valid[ty:ty + TILE_H, tx:tx + TILE_W].any() else without).append((tx // TILE_W, ty // TILE_H))
    return without, with_
