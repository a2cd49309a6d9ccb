"""numpy restatement of rtowUpsampleDevice's numeric specification (include/rtow.h, next to RtowUpsampleParams), vectorised over the dst pixels: positions in
int64, everything else in float32 with the association the header states (numpy neither contracts nor reassociates).  tests/test_upsample_reference.py holds it
to facts that do not come from it; tests/test_gpu_upsample.py compares the kernel with it bit for bit.  Also the one generator of random inputs both share."""
import numpy as np

F = np.float32
POINT, BILINEAR, GUIDED = 0, 1, 2
MATCH_ENTITY, DEMODULATE_ALBEDO = 1, 2
DEMOD_MIN = F(2.0 ** -10)
CAUSES = ("sky", "entity", "depth", "normal")


def axis_positions(src, dst):
    """One axis: (point pixel, bilinear base x0, fraction fx) for X = 0 .. dst-1"""
    X = np.arange(dst, dtype=np.int64)
    point = ((2 * X + 1) * src) // (2 * dst)
    N = (2 * X + 1) * src - dst
    x0 = N // (2 * dst)                                      # numpy's // floors
    r = N - x0 * 2 * dst
    assert (r >= 0).all() and (r < 2 * dst).all()
    return point, x0, r.astype(F) / F(2 * dst)


def _demod(c, a):
    with np.errstate(all="ignore"):
        return np.where(a >= DEMOD_MIN, c / a, c).astype(F)


def upsample(sw, sh, dw, dh, mode, normal_sharpness, depth_tolerance, flags, src_color, src_hits=None, src_albedo=None, dst_hits=None, dst_albedo=None):
    """-> (outColor (dw*dh, 3) float32, outStage (dw*dh,) uint8, rejected (dw*dh, 4) bool).  src_hits / dst_hits: (distance, entityIndex, normal).
    rejected[p, k]: a tap the pixel evaluated (stage A; stage B where it ran) got g = 0 for cause CAUSES[k] - the first that applies, in the specification's order."""
    nd = dw * dh
    src_color = np.ascontiguousarray(src_color, F).reshape(sw * sh, 3)
    demod = bool(flags & DEMODULATE_ALBEDO)
    match = bool(flags & MATCH_ENTITY)
    px, x0a, fxa = axis_positions(sw, dw)
    py, y0a, fya = axis_positions(sh, dh)
    X, Y = np.tile(np.arange(dw), dh), np.repeat(np.arange(dh), dw)
    out = src_color[py[Y] * sw + px[X]].copy()               # stage C everywhere; A and B overwrite where they answer
    stage = np.full(nd, 2, np.uint8)
    rejected = np.zeros((nd, 4), bool)
    if mode == POINT:
        return out, stage, rejected
    x0, y0, fx, fy = x0a[X], y0a[Y], fxa[X], fya[Y]
    if mode == GUIDED:
        st, se, sn = (np.ascontiguousarray(a) for a in src_hits)
        dt, de, dn = (np.ascontiguousarray(a) for a in dst_hits)
        st, dt, sn, dn = st.astype(F), dt.astype(F), sn.astype(F).reshape(-1, 3), dn.astype(F).reshape(-1, 3)
    tol = F(depth_tolerance)

    def guide(sel, q):
        e, t, n = de[sel], dt[sel], dn[sel]
        e2, t2, n2 = se[q], st[q], sn[q]
        with np.errstate(all="ignore"):
            sky = e < 0
            r_sky = np.where(sky, e2 >= 0, e2 < 0)
            r_ent = ~sky & ~r_sky & match & (e2 != e)
            near = np.abs(t2 - t) <= tol * t                 # NaN fails
            r_depth = ~sky & ~r_sky & ~r_ent & ~near
            d = (n[:, 0] * n2[:, 0] + n[:, 1] * n2[:, 1]) + n[:, 2] * n2[:, 2]
            d = np.where(d > 0, d, F(0)).astype(F)
            for _ in range(normal_sharpness):
                d = d * d
            compared = ~sky & ~r_sky & ~r_ent & ~r_depth
            r_normal = compared & ~(d > 0)
            g = np.where(sky, np.where(e2 < 0, F(1), F(0)), np.where(compared, d, F(0))).astype(F)
        rejected[sel] |= np.stack([r_sky, r_ent, r_depth, r_normal], axis=1)
        return g

    def accumulate(sel, taps):
        """taps: (qx, qy, base weight or None) per tap, arrays over `sel`; -> (acc, wsum)"""
        acc, wsum = np.zeros((sel.size, 3), F), np.zeros(sel.size, F)
        for qx, qy, base in taps:
            q = np.clip(qy, 0, sh - 1) * sw + np.clip(qx, 0, sw - 1)
            with np.errstate(all="ignore"):
                if mode == GUIDED:
                    g = guide(sel, q)
                    w = g if base is None else (base * g).astype(F)
                else:
                    w = base
                c = src_color[q]
                if demod:
                    c = _demod(c, src_albedo[q])
                ok = (w > 0) & np.isfinite(c).all(axis=1)
                acc = np.where(ok[:, None], acc + w[:, None] * c, acc).astype(F)
                wsum = np.where(ok, wsum + w, wsum).astype(F)
        return acc, wsum

    if demod:
        src_albedo = np.ascontiguousarray(src_albedo, F).reshape(sw * sh, 3)
        dst_albedo = np.ascontiguousarray(dst_albedo, F).reshape(nd, 3)

    def answer(sel, acc, wsum, which):
        got = wsum > 0
        with np.errstate(all="ignore"):
            r = (acc[got] / wsum[got][:, None]).astype(F)
            if demod:
                a = dst_albedo[sel[got]]
                r = np.where(a >= DEMOD_MIN, r * a, r).astype(F)
        out[sel[got]] = r
        stage[sel[got]] = which
        return sel[~got]

    everyone = np.arange(nd)
    bx0, by0 = F(1) - fx, F(1) - fy
    acc, wsum = accumulate(everyone, [(x0, y0, bx0 * by0), (x0 + 1, y0, fx * by0), (x0, y0 + 1, bx0 * fy), (x0 + 1, y0 + 1, fx * fy)])
    rest = answer(everyone, acc, wsum, 0)
    if mode == GUIDED and rest.size:
        ring = [(x0[rest] + i, y0[rest] + j, None) for j in range(-1, 3) for i in range(-1, 3) if not (i in (0, 1) and j in (0, 1))]
        acc, wsum = accumulate(rest, ring)
        answer(rest, acc, wsum, 1)
    return out, stage, rejected


# ---- the random inputs of the GPU test (and of the coverage check on the CPU) ----
HOLE_KINDS = ("nan", "opposed", "far", "sky", "foreign")


def _world(w, h, cells, rng_cells):
    """first-hit guides of a block-structured world sampled at the centres of a w x h grid: (distance, entity, normal, cell index)"""
    bx, by, ent, dist, nrm = cells
    X, Y = np.tile(np.arange(w), h), np.repeat(np.arange(h), w)
    cell = np.minimum((((Y + 0.5) / h) * by).astype(np.int64), by - 1) * bx + np.minimum((((X + 0.5) / w) * bx).astype(np.int64), bx - 1)
    e = ent[cell].astype(np.int32)
    t = np.where(e < 0, np.inf, dist[cell]).astype(F)
    n = nrm[cell] + rng_cells.normal(0, 0.02, (w * h, 3))                 # a little curvature
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(F)
    n[e < 0] = 0
    return t, e, n


def make_case(sw, sh, dw, dh, seed):
    """Inputs of one call.  Both guide sets sample ONE world of rectangular cells (entities 0..5, depths with steps inside and outside the usual tolerances, normals that
    agree, differ and oppose between cells, about a sixth of the cells sky).  On top of it the src side gets 3 x 3 holes - NaN colours, normals turned round, a surface
    64 times as far, a patch of sky, a foreign entity - which push dst pixels to stage B, single foreign pixels, and single NaN / inf colours; the dst side gets lonely
    pixels no src pixel agrees with (a distance a thousand times nearer, a normal of zero, an entity of their own), which end in stage C.  Albedos carry 0, 2^-11 and
    2^-10 in single channels."""
    rng = np.random.default_rng(seed)
    ns, nd = sw * sh, dw * dh
    bx, by = max(1, min(sw, dw) // 6), max(1, min(sh, dh) // 6)
    bx, by = min(bx, 24), min(by, 24)
    nc = bx * by
    ent = rng.integers(0, 6, nc)
    ent[rng.random(nc) < 0.16] = -1
    if nc == 1:
        ent[0] = -1 if seed % 3 == 0 else 2
    dist = rng.choice(np.array([1.0, 1.03, 1.5, 2.0, 8.0]), nc)
    axes = np.array([(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0.6, 0, 0.8), (0, 0.8, 0.6)], np.float64)
    nrm = axes[rng.integers(0, len(axes), nc)]
    cells = (bx, by, ent, dist, nrm)
    st, se, sn = _world(sw, sh, cells, rng)
    dt, de, dn = _world(dw, dh, cells, rng)

    src_color = rng.uniform(0, 3, (ns, 3)).astype(F)
    src_albedo, dst_albedo = rng.uniform(0.05, 1, (ns, 3)).astype(F), rng.uniform(0.05, 1, (nd, 3)).astype(F)
    # 3 x 3 src holes of every kind (cut at the border; a frame one or two pixels wide takes narrower ones)
    holes = max(1, int(np.ceil(0.035 * ns / 9))) if ns >= 9 else 0
    img = lambda a: a.reshape(sh, sw, *a.shape[1:])
    for kind in HOLE_KINDS:
        for _ in range(holes):
            cx, cy = int(rng.integers(0, sw)), int(rng.integers(0, sh))
            sl = (slice(max(0, cy - 1), cy + 2), slice(max(0, cx - 1), cx + 2))
            if kind == "nan":
                img(src_color)[sl] = np.nan
            elif kind == "opposed":
                img(sn)[sl] = -img(sn)[sl]
            elif kind == "far":
                img(st)[sl] = img(st)[sl] * F(64)
            elif kind == "sky":
                img(se)[sl], img(st)[sl], img(sn)[sl] = -1, np.inf, 0
            else:
                was_sky = img(se)[sl] < 0
                img(se)[sl] = np.where(was_sky, -1, 100 + int(rng.integers(0, 50)))
    if ns > 1:
        single = rng.choice(ns, max(1, ns // 80), replace=False)
        se[single] = np.where(se[single] < 0, -1, 200)
        for val in (np.nan, np.inf, -np.inf):
            idx = rng.choice(ns, max(1, ns // 150), replace=False)
            src_color[idx, rng.integers(0, 3, idx.size)] = val
    if nd > 1:
        lonely = rng.choice(nd, max(3, int(0.075 * nd)), replace=False)
        third = lonely.size // 3
        near, flat, own = lonely[:third], lonely[third:2 * third], lonely[2 * third:]
        surf = lambda i: i[de[i] >= 0]
        dt[surf(near)] *= F(2.0 ** -10)
        dn[surf(flat)] = 0
        # entities of their own (a sky pixel among them becomes a surface at distance 1 facing +z): with MATCH_ENTITY no src pixel agrees
        de[own], dt[own] = 300 + np.arange(own.size), np.where(np.isfinite(dt[own]), dt[own], F(1))
        dn[own] = np.where((dn[own] == 0).all(axis=1)[:, None], np.array([0, 0, 1], F), dn[own])
    for alb in (src_albedo, dst_albedo):
        for val in (0.0, 2.0 ** -11, 2.0 ** -10):
            idx = rng.choice(alb.shape[0], max(1, alb.shape[0] // 40), replace=False)
            alb[idx, rng.integers(0, 3, idx.size)] = val
    return {"sw": sw, "sh": sh, "dw": dw, "dh": dh, "src_color": src_color, "src_hits": (st, se, sn), "src_albedo": src_albedo, "dst_hits": (dt, de, dn),
            "dst_albedo": dst_albedo}


def reference(case, mode, normal_sharpness, depth_tolerance, flags):
    return upsample(case["sw"], case["sh"], case["dw"], case["dh"], mode, normal_sharpness, depth_tolerance, flags, case["src_color"], case["src_hits"],
                    case["src_albedo"], case["dst_hits"], case["dst_albedo"])


# the (src, dst) size pairs of the GPU comparison and the configurations (mode, normalSharpness, depthTolerance, flags) run at each
SIZE_PAIRS = [((1, 1), (1, 1)), ((1, 1), (7, 5)), ((5, 3), (10, 6)), ((13, 7), (37, 29)), ((48, 27), (96, 54)), ((96, 54), (96, 54)), ((64, 36), (48, 27)),
              ((3, 257), (9, 300)), ((16383, 1), (16384, 1)), ((16384, 1), (16383, 1))]
LARGE_PAIR = ((960, 540), (1920, 1080))
CONFIGS = [(POINT, 0, 0.0, 0), (BILINEAR, 0, 0.0, 0), (BILINEAR, 4, 0.05, DEMODULATE_ALBEDO),
           (GUIDED, 4, 0.05, MATCH_ENTITY | DEMODULATE_ALBEDO), (GUIDED, 0, 1.0, 0), (GUIDED, 8, 0.01, MATCH_ENTITY), (GUIDED, 2, 0.0, DEMODULATE_ALBEDO)]
LARGE_CONFIGS = [CONFIGS[0], CONFIGS[2], CONFIGS[3]]
COVERAGE_MIN_PIXELS = 1000


def case_seed(src, dst):
    return 7919 * src[0] + 31 * src[1] + 101 * dst[0] + dst[1]


def coverage(stage, rejected, flags):
    """The shares the coverage condition is about: pixels per stage, and pixels with a tap rejected for each cause.  The entity cause exists only with MATCH_ENTITY (without
    the flag the specification never compares entities), so it is reported as None there and not asked for."""
    n = stage.size
    out = {"A": float((stage == 0).sum()) / n, "B": float((stage == 1).sum()) / n, "C": float((stage == 2).sum()) / n}
    for k, name in enumerate(CAUSES):
        out[name] = float(rejected[:, k].sum()) / n if (name != "entity" or flags & MATCH_ENTITY) else None
    return out


def coverage_ok(cov):
    return all(cov[s] >= 0.02 for s in "ABC") and all(cov[c] is None or cov[c] >= 0.01 for c in CAUSES)
