"""numpy float32 restatement of rtowNoiseMaskDevice (include/rtow.h): the pixel's own error from the luminance moments, its 3 x 3 tent filter over the known
in-image taps, the histogram over binades, the budget's threshold in integers, the qualifying set and its dilation.  Every float operation is one float32 operation of
the specification, in its order; counts and the threshold choice are Python integers.  The GPU tests compare the kernel with this bit for bit."""
import numpy as np

F = np.float32
ABSOLUTE, UNKNOWN_QUALIFIES = 1, 2
BINS = 64
UNKNOWN = F(-1)
TILE_W, TILE_H = 64, 4


def own_error(moments, absolute, luminance_floor):
    """e(q) -> (n,) float32, -1 where unknown"""
    m = np.ascontiguousarray(moments, F).reshape(-1, 3)
    s1, s2, n = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(all="ignore"):
        usable = np.isfinite(m).all(1) & (n >= F(2))
        mean = s1 / n
        d = s2 - s1 * mean
        d = np.where(d > 0, d, F(0)).astype(F)
        v = d / (n * (n - F(1)))
        if absolute:
            e = v
        else:
            f2 = F(luminance_floor) * F(luminance_floor)
            e = v / (mean * mean + f2)
        known = usable & np.isfinite(e)
    return np.where(known, e, UNKNOWN).astype(F)


def filtered_error(width, height, e):
    """g(p) -> (n,) float32, -1 where unknown"""
    plane = np.full((height + 2, width + 2), UNKNOWN, F)
    plane[1:-1, 1:-1] = e.reshape(height, width)
    num, den = np.zeros((height, width), F), np.zeros((height, width), F)
    with np.errstate(all="ignore"):
        for j in (-1, 0, 1):
            for i in (-1, 0, 1):
                eq = plane[1 + j: 1 + j + height, 1 + i: 1 + i + width]
                tap = eq >= 0
                w = F(0.5 if i == 0 else 0.25) * F(0.5 if j == 0 else 0.25)
                num = np.where(tap, num + w * eq, num).astype(F)
                den = np.where(tap, den + w, den).astype(F)
        g = num / den
        known = (plane[1:-1, 1:-1] >= 0) & np.isfinite(g)
    return np.where(known, g, UNKNOWN).astype(F).reshape(-1)


def bin_of(g):
    """bin(g) of known errors (g >= 0, finite) -> int64"""
    bits = np.ascontiguousarray(g, F).view(np.uint32).astype(np.int64)
    return np.clip((bits >> 23) - 96, 0, BINS - 1)


def bin_lower_bound(b):
    """L(b) as float32"""
    return F(0) if b == 0 else F(2.0 ** (b - 31))


def pick_threshold(histogram, unknown, error_threshold, max_qualifying, flags):
    """T of the specification (float32) and R (None without a budget)"""
    if max_qualifying == 0:
        return F(error_threshold), None
    u = int(unknown) if flags & UNKNOWN_QUALIFIES else 0
    r = max_qualifying - u if max_qualifying > u else 0
    best = None
    for b in range(BINS):
        if sum(int(x) for x in histogram[b:]) <= r:
            best = b
            break
    if best is None:
        return F(np.inf), r
    return max(F(error_threshold), bin_lower_bound(best)), r


def dilate(width, height, qualifies, radius):
    """OR over the in-image Chebyshev neighbourhood, by shifted copies"""
    q = qualifies.reshape(height, width)
    plane = np.zeros((height + 2 * radius, width + 2 * radius), bool)
    plane[radius: radius + height, radius: radius + width] = q
    out = np.zeros((height, width), bool)
    for j in range(2 * radius + 1):
        for i in range(2 * radius + 1):
            out |= plane[j: j + height, i: i + width]
    return out.reshape(-1)


def noise_mask(width, height, moments, error_threshold, luminance_floor, dilate_radius, max_qualifying, flags, g=None):
    """rtowNoiseMaskDevice -> dict: mask (n,) uint8, error (n,) float32, qualifies (n,) bool, known, unknown, qualifying, masked, threshold, maxError, histogram (64,),
    R, and words: the 72 uint32 of RtowNoiseStats.  g: filtered_error of the same moments and error kind, when the caller has it already."""
    n = width * height
    if g is None:
        g = filtered_error(width, height, own_error(moments, bool(flags & ABSOLUTE), luminance_floor))
    known = g >= 0
    histogram = np.bincount(bin_of(g[known]), minlength=BINS).astype(np.uint32)
    unknown = int(n - known.sum())
    t, r = pick_threshold(histogram, unknown, error_threshold, max_qualifying, flags)
    qualifies = np.where(known, g >= t, bool(flags & UNKNOWN_QUALIFIES))
    mask = dilate(width, height, qualifies, dilate_radius)
    max_error = F(g[known].max()) if known.any() else F(0)
    words = np.zeros(72, np.uint32)
    words[:4] = int(known.sum()), unknown, int(qualifies.sum()), int(mask.sum())
    words[4:6] = np.array([t, max_error], F).view(np.uint32)
    words[8:] = histogram
    return {"mask": mask.astype(np.uint8), "error": g, "qualifies": qualifies, "known": int(known.sum()), "unknown": unknown, "qualifying": int(qualifies.sum()),
            "masked": int(mask.sum()), "threshold": t, "maxError": max_error, "histogram": histogram, "R": r, "words": words}


# ---------------------------------------------------------------- inputs

SIZES = [(1, 1), (1, 9), (9, 1), (63, 3), (64, 4), (65, 5), (130, 9), (96, 54)]


def case_seed(w, h):
    return 1000 * w + h


def make_moments(w, h, seed):
    """Moments of batches of a plausible frame - n in 2..16, means over five decades, relative deviations from 1e-4 to 3 - seeded with what the kernel can get wrong:
    unknown pixels (n < 2) on the image border and in the corners of the 64 x 4 tiles, runs of zero variance, huge n (n (n - 1) overflows), triples with NaN and
    +-inf in each member, means of zero (a relative error over F2 alone), and sums large and small enough for the first and the last bin."""
    rng = np.random.default_rng(seed)
    n = w * h
    cx, cy = np.tile(np.arange(w), h), np.repeat(np.arange(h), w)
    count = rng.integers(2, 17, n).astype(F)
    mean = np.exp(rng.uniform(np.log(1e-3), np.log(1e2), n))
    rel = np.exp(rng.uniform(np.log(1e-4), np.log(3.0), n))
    s1 = count * mean
    s2 = count * (mean * mean) * (1 + rel * rel)
    m = np.stack([s1, s2, count], axis=1).astype(F)
    pick = lambda share: rng.random(n) < share
    border = (cx == 0) | (cy == 0) | (cx == w - 1) | (cy == h - 1)
    corner = ((cx % TILE_W == 0) | (cx % TILE_W == TILE_W - 1)) & ((cy % TILE_H == 0) | (cy % TILE_H == TILE_H - 1))
    short = (border & pick(0.4)) | (corner & pick(0.5)) | pick(0.03)
    m[short, 2] = rng.choice(np.array([0, 0.5, 1, 1.5, -3], F), int(short.sum()))
    flat = pick(0.05)                                                 # zero variance: s2 == s1 * (s1 / n) exactly
    m[flat] = (1, 0.25, 4)
    huge = pick(0.03)
    m[huge, 2] = rng.choice(np.array([1e6, 3e19, 3e38], F), int(huge.sum()))
    dark = pick(0.03)
    m[dark, 0] = 0
    top = pick(0.02)
    m[top, 1] = rng.choice(np.array([1e30, 3e38, 2.0 ** 40], F), int(top.sum()))
    low = pick(0.02)
    with np.errstate(all="ignore"):
        m[low, 1] = (m[low, 0] * (m[low, 0] / m[low, 2]) * F(1 + 2.0 ** -20)).astype(F)
    for value in (np.nan, np.inf, -np.inf):
        at = np.flatnonzero(pick(0.01))
        m[at, rng.integers(0, 3, at.size)] = value
    if n >= 64:                                                       # whatever the dice gave: one of each near the origin, next to a tile corner
        m[0] = (np.nan, 1, 4)
        m[1] = (1, 1, 1)
        m[w - 1] = (2, np.inf, 4)
    return m


def power_of_two_bands(w, h, exponents=(-40, -31, -30, -1, 0, 31, 32, 40), band=4):
    """ABSOLUTE errors that sit exactly on bin edges: column bands of `band` pixels whose e is 2^k exactly - (s1, s2, n) = (0, 2^(k+1), 2) gives mean 0, d = s2,
    v = 2^k - so that g is 2^k exactly inside a band (every tap equal) and a mixture across a border"""
    cx = np.tile(np.arange(w), h)
    k = np.asarray(exponents)[(cx // band) % len(exponents)]
    m = np.zeros((w * h, 3), F)
    m[:, 1] = np.ldexp(F(1), k + 1).astype(F)
    m[:, 2] = 2
    return m
