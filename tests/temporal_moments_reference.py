"""numpy float32 restatement of rtowReprojectMomentsDevice and rtowEstimateMomentsDevice (include/rtow.h): the luminance moments gathered through
rtowReprojectAccumDevice's source map with a history cap, and the 7 x 7 guide-weighted estimate for pixels without a history.  Vectorised over pixels with the tap
loop in the specification's order (j outer, i inner); every operation is one float32 operation of the specification - no contraction, correctly rounded division, no
sqrt / exp / pow - so the result is the kernels', bit for bit.  The guide weight is rtowUpsampleDevice's rule (tests/upsample_reference.py keeps its copy inside
`upsample`; tests/test_temporal_moments_reference.py holds this one to it).  Also the generator of the random inputs the CPU and GPU tests share.  A helper of the
tests, not a test."""
import numpy as np

from denoise_variance_reference import lum

F = np.float32
MATCH_ENTITY = 1
RADIUS = 3


def reproject_moments(source, previous, max_batches):
    """rtowReprojectMomentsDevice: source (n,) int32, previous (n, 3) float32 -> (n, 3)"""
    source = np.ascontiguousarray(source, np.int32).reshape(-1)
    prev = np.ascontiguousarray(previous, F).reshape(-1, 3)
    n = source.size
    out = np.zeros((n, 3), F)
    inside = (source >= 0) & (source.astype(np.int64) < n)
    m = prev[np.where(inside, source, 0)]
    cap = F(max_batches)
    with np.errstate(all="ignore"):
        valid = inside & np.isfinite(m).all(axis=1) & (m[:, 2] >= 1)
        over = valid & (m[:, 2] > cap)
        k = cap / m[:, 2]
        scaled = np.stack([m[:, 0] * k, m[:, 1] * k, np.full(n, cap, F)], axis=1).astype(F)
    out[valid] = m[valid]                                  # bit for bit
    out[over] = scaled[over]
    return out


def guide_weight(e, t, n, e2, t2, n2, normal_sharpness, depth_tolerance, match):
    """g(p, q) of rtowUpsampleDevice's specification: e, t, n the pixel's guides, e2, t2, n2 the other pixel's (arrays of one shape; n, n2 with a last axis of 3)"""
    tol = F(depth_tolerance)
    with np.errstate(all="ignore"):
        sky = e < 0
        near = np.abs(t2 - t) <= tol * t                   # NaN fails
        d = (n[..., 0] * n2[..., 0] + n[..., 1] * n2[..., 1]) + n[..., 2] * n2[..., 2]
        d = np.where(d > 0, d, F(0)).astype(F)
        for _ in range(normal_sharpness):
            d = d * d
        compared = ~sky & (e2 >= 0) & ~(bool(match) & (e2 != e)) & near
        return np.where(sky, np.where(e2 < 0, F(1), F(0)), np.where(compared, d, F(0))).astype(F)


def luminance(color):
    """L(q): (l, valid) over an array of float4 colours"""
    c = np.ascontiguousarray(color, F)
    with np.errstate(all="ignore"):
        w = c[..., 3]
        l = lum(c[..., :3] / w[..., None]).astype(F)
        return l, (w > 0) & np.isfinite(l)                 # a NaN w fails w > 0


def estimate_moments(width, height, color, hits, in_moments, min_batches, min_taps, normal_sharpness, depth_tolerance, flags):
    """rtowEstimateMomentsDevice -> (outMoments (n, 3) float32, outFilled (n,) uint8, wanted (n,) bool: the pixels whose n is not >= minBatches).
    hits = (distance, entityIndex, normal); in_moments (n, 3) or None = zeros."""
    h, w = height, width
    c = np.ascontiguousarray(color, F).reshape(h, w, 4)
    t, e, nrm = hits
    t = np.ascontiguousarray(t, F).reshape(h, w)
    e = np.ascontiguousarray(e, np.int32).reshape(h, w)
    nrm = np.ascontiguousarray(nrm, F).reshape(h, w, 3)
    m = np.zeros((h * w, 3), F) if in_moments is None else np.ascontiguousarray(in_moments, F).reshape(h * w, 3).copy()
    with np.errstate(all="ignore"):
        wanted = ~(m[:, 2] >= F(min_batches)).reshape(h, w)                # a NaN n is estimated
    l, valid = luminance(c)
    W, S1, S2 = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
    taps = np.zeros((h, w), np.int32)
    match = bool(flags & MATCH_ENTITY)
    with np.errstate(all="ignore"):
        for j in range(-RADIUS, RADIUS + 1):
            for i in range(-RADIUS, RADIUS + 1):
                y0, y1, x0, x1 = max(0, -j), min(h, h - j), max(0, -i), min(w, w - i)
                if y0 >= y1 or x0 >= x1:
                    continue                                               # every tap of this offset lies outside the image
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + j, y1 + j), slice(x0 + i, x1 + i))
                if i == 0 and j == 0:
                    wgt = np.ones(l[P].shape, F)                           # the centre: w = 1, no guide consulted (its own L is checked below)
                else:
                    wgt = guide_weight(e[P], t[P], nrm[P], e[Q], t[Q], nrm[Q], normal_sharpness, depth_tolerance, match)
                lq = l[Q]
                take = valid[Q] & (wgt > 0)                                # skipped taps add nothing (not + 0)
                W[P] = np.where(take, W[P] + wgt, W[P])
                S1[P] = np.where(take, S1[P] + wgt * lq, S1[P])
                S2[P] = np.where(take, S2[P] + wgt * (lq * lq), S2[P])
                taps[P] += take
        a, b = S1 / W, S2 / W
        filled = wanted & valid & (taps >= min_taps) & np.isfinite(a) & np.isfinite(b)
        est = np.stack([a + a, b + b, np.full((h, w), F(2))], axis=-1).astype(F).reshape(h * w, 3)
    filled = filled.reshape(-1)
    out = m.copy()                                                         # unchanged pixels keep their bits
    out[filled] = est[filled]
    return out, filled.astype(np.uint8), wanted.reshape(-1)


# ---- the random inputs of the GPU tests (and of their coverage condition, which is checked on the CPU) ----
SIZES = [(1, 1), (3, 2), (7, 7), (8, 8), (64, 4), (65, 5), (70, 10), (41, 29), (257, 3), (96, 54)]
# (minBatches, minTaps, normalSharpness, depthTolerance, flags): sharpness 0 and 8, tolerance 0, the flag on and off, minTaps 2 and 49
CONFIGS = [(4, 2, 2, 0.05, 1), (2, 49, 0, 0.25, 0), (8, 2, 8, 0.0, 1), (4, 8, 0, 0.05, 0), (3, 2, 4, 1.0, 1)]
EXACT_TOLERANCE = 0.25         # exact in float32: the generator puts pixels at |t' - t| == 0.25 t exactly, which CONFIGS[1] accepts and a smaller tolerance rejects


def case_seed(w, h):
    return 1009 * w + 17 * h


def make_case(w, h, seed):
    """Inputs of one rtowEstimateMomentsDevice call.  Guides: a few large rectangular entity regions (entities 0..4) with sky blocks (-1, +inf, zero normal), per
    region a base distance and normal with a little curvature; single pixels at exactly (1 + 0.25) times the region's distance (a power-of-two base keeps the product
    exact), single pixels far off, normals of exactly zero on surfaces, a few NaN distances.  Colours: sums over w = 1 .. 4 samples, with w = 0, a NaN w, a negative w
    and non-finite channels.  Moments: n in {0, 1, 2, 3, 4, 8, 20} with plausible sums, and NaN / inf entries."""
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
    jitter = rng.random(n)
    t = np.where(jitter < 0.5, t, (t * (1 + rng.uniform(-0.04, 0.04, n))).astype(F)).astype(F)        # half the surface pixels sit at the base distance exactly
    pick = lambda share: rng.random(n) < share
    at_tol = pick(0.06)
    t[at_tol] = (dist[cell][at_tol] * 1.25).astype(F)                      # exactly at the tolerance of a neighbour at the base distance
    far = pick(0.04)
    t[far] = t[far] * F(16)
    t[pick(0.01)] = np.nan
    nn[pick(0.05)] = 0                                                     # a surface whose normal is exactly zero: n.n' = 0
    sky = e < 0
    t[sky], nn[sky] = np.inf, 0
    cw = rng.integers(1, 5, n).astype(F)
    base = rng.uniform(0.1, 2.0, (nc, 3))[cell] * (1 + 0.3 * rng.normal(size=(n, 3)))
    color = np.concatenate([np.abs(base) * cw[:, None], cw[:, None]], axis=1).astype(F)
    color[pick(0.06), 3] = 0
    color[pick(0.03), 3] = np.nan
    color[pick(0.02), 3] = -1
    for val in (np.inf, -np.inf, np.nan):
        idx = np.flatnonzero(pick(0.02))
        color[idx, rng.integers(0, 3, idx.size)] = val
    cnt = rng.choice(np.array([0, 1, 2, 3, 4, 8, 20], F), n, p=[0.2, 0.1, 0.1, 0.1, 0.2, 0.15, 0.15])
    mean = rng.uniform(0.1, 2.0, n)
    moments = np.stack([mean * cnt, (mean * mean + 0.01) * cnt, cnt], axis=1).astype(F)
    for val in (np.nan, np.inf):
        idx = np.flatnonzero(pick(0.02))
        moments[idx, rng.integers(0, 3, idx.size)] = val
    return {"w": w, "h": h, "n": n, "color": color, "hits": (t, e, nn), "moments": moments}


def reference(case, cfg, moments="given"):
    min_batches, min_taps, sharp, tol, flags = cfg
    m = case["moments"] if isinstance(moments, str) else moments
    return estimate_moments(case["w"], case["h"], case["color"], case["hits"], m, min_batches, min_taps, sharp, tol, flags)


def no_pixel_qualifies(case, cfg):
    """the early-out variant: every n is at least minBatches (sums as given, NaN / inf sums stay: only n decides)"""
    m = case["moments"].copy()
    m[:, 2] = F(cfg[0]) + (np.arange(case["n"]) % 3).astype(F)
    return m


def one_pixel_qualifies(case, cfg):
    """exactly one pixel of one tile qualifies: the pixel in the middle of the frame whose colour has a valid luminance (the first pixel if there is none)"""
    m = no_pixel_qualifies(case, cfg)
    _, valid = luminance(case["color"])
    order = np.argsort(np.abs(np.arange(case["n"]) - case["n"] // 2), kind="stable")
    good = order[valid[order]]
    p = int(good[0]) if good.size else 0
    m[p, 2] = F(0)
    return m, p


def coverage(filled, wanted):
    """(filled pixels, qualifying pixels left unchanged, pixels that do not qualify)"""
    filled = filled.astype(bool)
    return int(filled.sum()), int((wanted & ~filled).sum()), int((~wanted).sum())


def make_gather_case(n, seed, max_batches):
    """Inputs of one rtowReprojectMomentsDevice call: sources mixing valid indices, -1, INT32_MIN, n, n + 1 and INT32_MAX; moments with n in {0, 0.5, 1,
    maxBatches, maxBatches + 1, 1e6} and NaN / inf entries"""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, n).astype(np.int64)
    kind = rng.random(n)
    odd = np.array([-1, -2 ** 31, n, n + 1, 2 ** 31 - 1], np.int64)
    bad = kind < 0.3
    src[bad] = odd[rng.integers(0, len(odd), int(bad.sum()))]
    if n >= 5:
        src[:5] = odd                                                      # every kind, whatever the draw
        src[5:6] = n - 1
    mb = float(max_batches)
    cnt = np.array([0, 0.5, 1, mb, mb + 1, 1e6], F)[np.arange(n) % 6]
    rng.shuffle(cnt)
    mean = rng.uniform(0.1, 2.0, n)
    prev = np.stack([mean * cnt, (mean * mean + 0.01) * cnt, cnt], axis=1).astype(F)
    for val in (np.nan, np.inf, -np.inf):
        idx = np.flatnonzero(rng.random(n) < 0.05)
        prev[idx, rng.integers(0, 3, idx.size)] = val
    return src.astype(np.int32), prev
