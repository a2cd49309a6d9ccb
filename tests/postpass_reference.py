"""Numpy restatements of rtowCombineDevice and rtowReduceMetricsDevice as include/rtow.h and the reference's jobs (JOBS/CombineJob.cs:29-71, JOBS/ReduceMetricsJob.cs:22-45)
specify them, and the builders of every input of tests/test_gpu_postpass_edges.py.  float32 with every operation rounded on its own, Python integers for the sums.  Nothing
here reads the product's kernels.  tests/test_postpass_reference.py holds the restatements to the C++ oracle bit for bit on every built case and checks that each case
contains what it is named for; the GPU file compares the device with the oracle on the same cases.

The domain.  `(int) x` of a float is defined in C++ only where the truncated value fits an int; beyond that the CPU oracle is undefined (x86 returns INT32_MIN) while the
device conversion saturates, so no comparison there means anything.  Every color.w and every ray count built here is finite with a magnitude below 2^31 (`truncate`
asserts it); NaN or infinite color.w is outside the documented domain of both passes and is not tested.  The weight extrema of the metrics fold from (+inf, -inf) with
math.min / math.max, which skip a NaN second operand: the result does not depend on the order as long as no weight is -0 next to a +0, and the builders make none."""
import numpy as np

F = np.float32
U = np.uint32
FLT_MIN = F(2.0 ** -126)
NAN, INF = F(np.nan), F(np.inf)

RECORD = np.dtype([("totalRayCount", "<i4"), ("totalSamples", "<i4"), ("sampleCountWeightExtrema", "<f4", (2,)), ("sampleCountExtrema", "<i4", (2,)),
                   ("totalRayCount64", "<i8"), ("totalSamples64", "<i8")])      # RtowMetrics: 40 bytes, no padding
assert RECORD.itemsize == 40


def bits(x):
    return np.ascontiguousarray(x, F).view(U)


def truncate(x):
    """(int) x inside the domain: toward zero, so 0.9 and -0.5 are 0 and -3.7 is -3"""
    x = np.asarray(x, F)
    assert np.all(np.isfinite(x) & (np.abs(x) < F(2.0 ** 31))), "outside the domain of the float -> int conversion"
    return np.trunc(x).astype(np.int64)


# ---------------------------------------------------------------- combine
def walk(width, height, color4, debug_mode=False):
    """Per pixel: the row whose accumulated colour the pixel ends up holding and that pixel's sample count.  A pixel without samples looks at the pixel one row below
    (index - width), and so on, until one has samples or the index leaves the image; in debug mode nobody looks around."""
    own = truncate(np.asarray(color4, F).reshape(height, width, 4)[..., 3])
    row = np.repeat(np.arange(height)[:, None], width, 1)
    count = own.copy()
    if not debug_mode:
        for r in range(1, height):                       # the walk of row r - 1 ended where the walk of an empty pixel of row r ends
            empty = own[r] == 0
            row[r] = np.where(empty, row[r - 1], r)
            count[r] = np.where(empty, count[r - 1], own[r])
    return row, count


def combine(width, height, color4, normal, albedo, debug_mode=False, ldr_albedo=False):
    """(color, normal, albedo) as float32 (n, 3)"""
    n = width * height
    c = np.asarray(color4, F).reshape(height, width, 4)
    row, count = walk(width, height, c, debug_mode)
    held = c[row, np.arange(width)[None, :]].reshape(n, 4)
    count = count.reshape(n)
    with np.errstate(all="ignore"):
        mean = held[:, :3] / count.astype(F)[:, None]
        no_samples, nan_colour = (F([1, 0, 1]), F([0, 1, 1])) if debug_mode else (F([0, 0, 0]), F([0, 0, 0]))
        color = np.where(np.isnan(held).any(1)[:, None], nan_colour[None, :], mean)
        color = np.where((count == 0)[:, None], no_samples[None, :], color).astype(F)      # the count is asked first
        denom = np.maximum(count, 1).astype(F)[:, None]
        alb = np.asarray(albedo, F).reshape(n, 3) / denom
        if ldr_albedo:
            alb = np.where(alb < F(1), alb, F(1))        # math.min(x, 1) = IsNaN(1) || x < 1 ? x : 1: a NaN becomes 1
        v = np.asarray(normal, F).reshape(n, 3) / denom
        length = squared_length(v)
        unit = v * (F(1) / np.sqrt(length))[:, None]     # normalizesafe: rsqrt(dot(v, v)) * v where the dot exceeds FLT_MIN, else 0
        nrm = np.where((length > FLT_MIN)[:, None], unit, F(0))
    return color, nrm.astype(F), alb.astype(F)


def squared_length(v):
    with np.errstate(all="ignore"):
        return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


COMBINE_SHAPES = [(1, 1), (1, 37), (37, 1), (257, 3), (64, 9)]
PATTERNS = ("row0", "last_row", "rows_mod2", "empty_columns", "scattered")
W_SAMPLED = F([1, 2, 3, 1.9, -3, 2.0 ** 24, 2.0 ** 30, 7])      # (int) w != 0
W_EMPTY = F([0, 0.9, -0.5, -0.0])                               # (int) w == 0
NORMAL_EDGES = F([[0, 0, 0],
                  [2.0 ** -63, 0, 0],                           # squared length FLT_MIN exactly: not above the threshold
                  [2.0 ** -63, 1.5 * 2.0 ** -75, 0],            # 2^-126 + 2^-149: one ulp above it
                  [0, 2.0 ** -70, 0],                           # a denormal squared length
                  [1e-40, -1e-42, 0],                           # denormal components: the squares underflow to 0
                  [1e30, -1e30, 3e29],                          # the dot overflows to +inf: rsqrt 0, a signed zero per component
                  [np.nan, 1, 0], [0, 0, np.nan],
                  [0, -3, 4]])
ALBEDO_EDGES = F([1.0, np.nextafter(F(1), F(2)), 3.0, np.nan, -1.0])


def has_samples(pattern, width, height, rng):
    rows, cols = np.repeat(np.arange(height), width), np.tile(np.arange(width), height)
    if pattern == "row0":
        return rows == 0
    if pattern == "last_row":
        return rows == height - 1
    if pattern == "rows_mod2":
        return rows % 2 == 0
    if pattern == "empty_columns":
        return (cols % 3 != 0) & (rng.random(width * height) < 0.5)
    return rng.random(width * height) < 0.7


def combine_case(width, height, pattern, seed):
    """One frame of accumulators.  Which pixels have samples follows `pattern`; their w, the NaNs in r / g / b, and the normals and albedos at the edges of
    normalizesafe and of the LDR clamp are drawn per pixel."""
    rng = np.random.default_rng(seed)
    n = width * height
    sampled = has_samples(pattern, width, height, rng)
    w = np.where(sampled, W_SAMPLED[rng.integers(0, len(W_SAMPLED), n)], W_EMPTY[rng.integers(0, len(W_EMPTY), n)]).astype(F)
    scale = np.maximum(np.abs(w), F(1))
    color = np.concatenate([rng.uniform(0, 2, (n, 3)) * scale[:, None], w[:, None]], 1).astype(F)
    poisoned = rng.random(n) < 0.15                      # NaN in r, g or b: in pixels that others borrow from, and in pixels without samples
    if pattern == "row0":
        poisoned[:width] = np.arange(width) % 2 == 1     # every other column borrows a NaN pixel across all its rows
    color[poisoned, rng.integers(0, 3, int(poisoned.sum()))] = NAN
    normal = (rng.normal(size=(n, 3)) * scale[:, None]).astype(F)
    albedo = (rng.uniform(0, 1.2, (n, 3)) * scale[:, None]).astype(F)
    # the edge values are what is left AFTER the division by the (possibly borrowed) count, so they go where that count is a power of two or below 2: there
    # edge * count / count is the edge again, bit for bit.  (1e30 is not scaled: it would overflow before the division, and its dot overflows either way.)
    denom = np.maximum(walk(width, height, color)[1].reshape(n), 1)
    exact = np.flatnonzero(denom & (denom - 1) == 0)
    at, kind = exact[::2], np.arange(len(exact[::2])) % len(NORMAL_EDGES)
    normal[at] = NORMAL_EDGES[kind] * np.where(kind == 5, 1, denom[at]).astype(F)[:, None]
    at, kind = exact[1::2], np.arange(len(exact[1::2]))
    albedo[at, kind % 3] = ALBEDO_EDGES[kind % len(ALBEDO_EDGES)] * denom[at].astype(F)
    other = np.flatnonzero((denom & (denom - 1) != 0) & (rng.random(n) < 0.5))      # divided by 3 or 7: near the edges, not on them
    normal[other] = NORMAL_EDGES[rng.integers(0, len(NORMAL_EDGES), other.size)]
    albedo[other, rng.integers(0, 3, other.size)] = ALBEDO_EDGES[rng.integers(0, len(ALBEDO_EDGES), other.size)]
    return {"name": "%dx%d-%s" % (width, height, pattern), "w": width, "h": height, "pattern": pattern, "color": color, "normal": normal, "albedo": albedo}


def single_pixel_cases():
    """1 x 1: nothing to draw from, so one frame per w, per normal and per albedo of the lists"""
    cases = []

    def add(name, w, normal, albedo, rgb=(0.25, 0.5, 2.0)):
        cases.append({"name": "1x1-" + name, "w": 1, "h": 1, "pattern": "single", "color": F([[rgb[0], rgb[1], rgb[2], w]]), "normal": F([normal]), "albedo": F([albedo])})
    for k, w in enumerate(np.concatenate([W_SAMPLED, W_EMPTY])):
        add("w%d" % k, w, (0.0, 3.0, -4.0), (0.5, 0.25, 2.0))
    for k, e in enumerate(NORMAL_EDGES):
        add("normal%d" % k, (0, 1)[k % 2], e, (0.5, 0.25, 2.0))
    for k, e in enumerate(ALBEDO_EDGES):
        add("albedo%d" % k, 1, (1.0, 0.0, 0.0), (e, 0.5, e))
    add("nan-sampled", 2, (0.0, 0.0, 1.0), (0.5, 0.5, 0.5), (0.5, np.nan, 0.5))
    add("nan-empty", 0, (0.0, 0.0, 1.0), (0.5, 0.5, 0.5), (np.nan, 0.5, 0.5))
    return cases


def combine_cases(width, height):
    if (width, height) == (1, 1):
        return single_pixel_cases()
    return [combine_case(width, height, p, 7919 * width + 31 * height + k) for k, p in enumerate(PATTERNS)]


# ---------------------------------------------------------------- finalize
def first_floats_of_each_byte(oracle):
    """For k = 1..255 the bit pattern of a float in [0, 2] whose byte (oracle.finalize) is at least k while its predecessor's is below k: a bisection over bit
    patterns, all steps at once.  (Where the oracle's pow is not monotone from float to float this is one of the crossings, which is why the callers take its neighbours.)"""
    def byte(patterns):
        v = np.asarray(patterns, np.int64).astype(U).view(F)
        frame = np.zeros((v.size, 3), F)
        frame[:, 0] = v
        return oracle.finalize(frame, np.zeros_like(frame), np.zeros_like(frame))[0][:, 0].astype(np.int64)
    k = np.arange(1, 256)
    lo, hi = np.zeros(255, np.int64), np.full(255, int(bits(F(2))[0]), np.int64)      # byte(lo) < k <= byte(hi); 1.0 itself need not reach 255
    assert byte(lo[:1])[0] == 0 and byte(hi[:1])[0] == 255
    while np.any(hi - lo > 1):
        mid = (lo + hi) // 2
        up = byte(mid) >= k
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    return hi


def finalize_operands(oracle):
    """The 17 floats within 8 ulp of every byte step, then zeros, negatives, denormals, FLT_MIN, 1 and its neighbours, a huge value, infinities and NaN"""
    first = first_floats_of_each_byte(oracle)
    near = (first[:, None] + np.arange(-8, 9)[None, :]).reshape(-1).astype(U).view(F)
    special = F([0.0, -0.0, -1.0, 1e-45, 1e-40, -1e-40, 2.0 ** -126, 1.0, np.nextafter(F(1), F(2)), np.nextafter(F(1), F(0)), 1e30, np.inf, -np.inf, np.nan])
    return np.concatenate([near, special]).astype(F)


def normal_of(operands):
    """The normal whose finalize operand n * 0.5 + 0.5 is the given float, and where that holds exactly"""
    v = np.asarray(operands, F)
    with np.errstate(all="ignore"):
        nrm = (F(2) * v - F(1)).astype(F)
        back = (nrm * F(0.5) + F(0.5)).astype(F)
    return nrm, bits(back) == bits(v)


def finalize_frame(operands):
    """Every operand once in each of the nine channel positions: pixel i holds operands i .. i + 8 (cyclically) in colour, albedo, normal order.  An operand that does
    not survive n = 2 v - 1 -> n * 0.5 + 0.5 is replaced in the normal lane only, by the normal 0 (operand 0.5)."""
    v = np.asarray(operands, F)
    nrm, exact = normal_of(v)
    nrm = np.where(exact, nrm, F(0)).astype(F)
    at = lambda j: (np.arange(v.size) + j) % v.size
    color = np.stack([v[at(j)] for j in (0, 1, 2)], 1)
    albedo = np.stack([v[at(j)] for j in (3, 4, 5)], 1)
    normal = np.stack([nrm[at(j)] for j in (6, 7, 8)], 1)
    return color, normal, albedo


# ---------------------------------------------------------------- metrics
GRID_LANES = 2048 * 256                                  # lanes of the reduction's grid: a larger frame sends lanes round their loop again
METRICS_COUNTS = [1, 255, 257, 4096, GRID_LANES + 257]


def wrap32(x):
    """what an int32 holds after adding up to x with wrap-around"""
    return (int(x) + 2 ** 31) % 2 ** 32 - 2 ** 31


def weights(color4, scw):
    with np.errstate(all="ignore"):
        return (np.asarray(scw, F).reshape(-1) / truncate(np.asarray(color4, F)[:, 3]).astype(F)).astype(F)


def reduce_metrics(diag, color4, scw):
    """The record as a RECORD scalar array of one element; diag is (n, 1) or (n, 4), the ray count first"""
    rays, counts = truncate(np.asarray(diag, F)[:, 0]), truncate(np.asarray(color4, F)[:, 3])
    w = weights(color4, scw)
    assert not np.any((bits(w) == U(0x80000000))), "a -0 weight: the extrema would depend on the order of the fold"
    out = np.zeros(1, RECORD)
    out["totalRayCount64"], out["totalSamples64"] = int(rays.sum()), int(counts.sum())
    out["totalRayCount"], out["totalSamples"] = wrap32(rays.sum()), wrap32(counts.sum())
    out["sampleCountWeightExtrema"] = [np.fmin.reduce(w, initial=INF), np.fmax.reduce(w, initial=-INF)]      # a NaN weight moves nothing
    cf = counts.astype(F)
    out["sampleCountExtrema"] = [int(cf.min()), int(cf.max())]
    return out


def record_of(m):
    """an abi.Metrics (ctypes) as a RECORD array"""
    return np.frombuffer(bytes(m), RECORD).copy()


def _metrics(name, rays, counts, scw, seed):
    rng = np.random.default_rng(seed)
    n = len(rays)
    diag = np.full((n, 4), NAN, F)                       # three junk floats behind each count (the stride-16 layout); the stride-4 layout is diag[:, :1]
    diag[:, 0] = rays
    rgb = rng.uniform(0, 40, (n, 3))
    rgb[rng.random(n) < 0.1] = np.nan                    # only w is read
    color = np.concatenate([rgb, np.asarray(counts, F).reshape(n, 1)], 1).astype(F)
    assert np.array_equal(color[:, 3].astype(np.int64), np.asarray(counts, np.int64)) and np.array_equal(diag[:, 0].astype(np.int64), np.asarray(rays, np.int64)), "float32-exact counts"
    return {"name": name, "n": n, "diag": diag, "color": color, "scw": np.asarray(scw, F)}


def metrics_frame(n, seed=0):
    """A frame as a host sees it, with every kind of pixel: a few negative ray counts, pixels without samples whose weight is 0 (0 / 0: skipped) or positive (+inf),
    NaN and +inf in sampleCountWeight.  Beyond one round of the grid, the tail holds what decides every field of the record."""
    rng = np.random.default_rng(1000 + n + seed)
    rays = rng.integers(0, 3000, n)
    counts = rng.integers(1, 300, n)
    scw = rng.uniform(1, 50, n).astype(F)
    if n == 1:
        return _metrics("frame-1", rays, counts, scw, n)
    pick = lambda k: rng.choice(n, max(1, min(k, n // 8)), replace=False)
    rays[pick(5)] = -rng.integers(1, 50, 1)
    empty = pick(n // 7)
    counts[empty] = 0
    scw[empty[::2]] = 0                                  # 0 / 0
    scw[pick(3)] = NAN
    scw[pick(2)] = INF
    if n > GRID_LANES:
        tail = GRID_LANES + np.array([0, 1, 100, 255, 256])
        rays[tail[0]], rays[tail[1]] = -70000, 123456792
        counts[tail[2]], scw[tail[2]] = 100000, F(1e-3)  # the largest count and the smallest weight
        counts[tail[3]], scw[tail[3]] = 1, F(1e6)        # the largest finite weight
        scw[np.isinf(scw)] = 1.0
        counts[:GRID_LANES] = np.maximum(counts[:GRID_LANES], 1)      # the only +inf and the only empty pixel are in the tail, too
        scw[:GRID_LANES] = np.maximum(scw[:GRID_LANES], F(1))         # (a NaN stays a NaN)
        counts[tail[4]], scw[tail[4]] = 0, F(3.0)
    return _metrics("frame-%d" % n, rays, counts, scw, n)


def metrics_edge_cases():
    n = 4096
    rng = np.random.default_rng(77)
    small = lambda: rng.integers(0, 3000, n)
    some = lambda: rng.integers(1, 300, n)
    scw = lambda: rng.uniform(1, 50, n).astype(F)
    cases = []
    # the sums pass 2^31 (int32 negative) and 2^32 (positive again), rays and samples independently; every count is a float32-exact integer below 2^31
    big = lambda total: (np.full(n, total // n) + rng.integers(-1000, 1000, n)) // 64 * 64
    cases.append(_metrics("rays-wrap-negative", big(3 * 10 ** 9), some(), scw(), 1))
    cases.append(_metrics("samples-wrap-negative", small(), big(3 * 10 ** 9), scw(), 2))
    def three(x):                                        # three pixels of 2 * 10^9 (a multiple of 128: exact) pass 2^32 on their own
        x[[5, 2048, 4095]] = 2 * 10 ** 9
        return x
    cases.append(_metrics("rays-wrap-positive", three(small()), some(), scw(), 3))
    cases.append(_metrics("samples-wrap-positive", small(), three(some()), scw(), 4))
    cases.append(_metrics("both-wrap", big(5 * 10 ** 9), big(7 * 10 ** 9), scw(), 5))
    negative = small()
    negative[::5] = -rng.integers(1, 10 ** 6, len(negative[::5]))
    cases.append(_metrics("negative-rays", negative, some(), scw(), 6))
    for m in (1, 257):
        cases.append(_metrics("all-weights-nan-%d" % m, small()[:m], np.zeros(m, np.int64), np.zeros(m, F), 7))
    lone = np.where(np.arange(257) % 2 == 0, NAN, F(0)).astype(F)      # NaN / 0 and 0 / 0 ...
    counts = np.zeros(257, np.int64)
    counts[200], lone[200] = 8, F(2.5)                                 # ... and one finite weight
    cases.append(_metrics("one-finite-weight", small()[:257], counts, lone, 8))
    w = scw()[:257]
    w[::3], w[1::3] = NAN, INF
    cases.append(_metrics("nan-and-inf-weights", small()[:257], some()[:257], w, 9))
    counts = some()[:255]
    counts[::4] = 0
    cases.append(_metrics("empty-pixels-with-weight", small()[:255], counts, scw()[:255], 10))
    return cases
