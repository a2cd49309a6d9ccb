"""numpy float32 restatement of rtowReprojectAccumBilinearDevice (include/rtow.h): the previous view's accumulators, and optionally its luminance
moments, carried to the pixels of a new view through the four previous pixels around the reprojected point, vectorised over pixels.  Every operation is one
float32 operation of the specification - no contraction, correctly rounded division and square root - so the result is the kernel's, bit for bit.  Steps 1 to 3
are those of tests/reproject_reference.py: its dot and view constants are used as they are, its projection is restated here up to (fx, fy) because the nearest
restatement keeps them to itself (tests/test_reproject_bilinear_reference.py holds the two against each other).  A helper of the tests, not a test."""
import numpy as np

import reproject_reference as rr

F = rr.F
MATCH_ENTITY = rr.MATCH_ENTITY
KEYS = ("color", "normal", "albedo", "scw")


def project(w, h, pv, o, d, t, e):
    """steps 1 and 2: (inside bool[n], fx, fy, r float32[n]); fx, fy are meaningful where inside"""
    W, H = F(w), F(h)
    LF, LR, LU, HR, VU = rr.view_constants(pv)
    o, d, t = o.astype(F, copy=False), d.astype(F, copy=False), t.astype(F, copy=False)
    hit = e >= 0
    with np.errstate(all="ignore"):
        px, py, pz = o[:, 0] + t * d[:, 0], o[:, 1] + t * d[:, 1], o[:, 2] + t * d[:, 2]
        org = pv["origin"]
        wx = np.where(hit, px - org[0], d[:, 0]).astype(F)
        wy = np.where(hit, py - org[1], d[:, 1]).astype(F)
        wz = np.where(hit, pz - org[2], d[:, 2]).astype(F)
        r = np.sqrt((wx * wx + wy * wy) + wz * wz)
        s = rr.dot(wx, wy, wz, pv["forward"]) / LF
        u = (rr.dot(wx, wy, wz, pv["right"]) / s - LR) / HR
        v = (rr.dot(wx, wy, wz, pv["up"]) / s - LU) / VU
        fx, fy = u * W, v * H
        assert r.dtype == s.dtype == fx.dtype == fy.dtype == F
        inside = (s > 0) & (fx >= 0) & (fx < W) & (fy >= 0) & (fy < H)
    return inside, fx, fy, r


def taps(w, h, inside, fx, fy):
    """the four taps of every pixel: (q int64[4, n] - 0 where the tap is outside the image -, b float32[4, n], usable bool[4, n] = inside the image and b > 0)"""
    gx, gy = np.where(inside, fx, F(0.5)) - F(0.5), np.where(inside, fy, F(0.5)) - F(0.5)
    flx, fly = np.floor(gx), np.floor(gy)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    ax, ay = gx - x0.astype(F), gy - y0.astype(F)
    assert ax.dtype == ay.dtype == F
    one = F(1)
    b = np.stack([(one - ax) * (one - ay), ax * (one - ay), (one - ax) * ay, ax * ay]).astype(F)
    qx = np.stack([x0, x0 + 1, x0, x0 + 1])
    qy = np.stack([y0, y0, y0 + 1, y0 + 1])
    usable = inside[None, :] & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (b > 0)
    q = np.where(usable, qy * w + qx, 0)
    return q, b, usable


def matches(q, e, r, pt, pe, depth_tolerance, flags):
    """step 3 at previous pixels q (any shape broadcastable with e and r)"""
    tol = F(depth_tolerance)
    pe_q, pt_q = pe[q], pt[q].astype(F, copy=False)
    with np.errstate(all="ignore"):
        ok_hit = (pe_q >= 0) & (np.abs(pt_q - r) <= tol * r)
    if flags & MATCH_ENTITY:
        ok_hit &= pe_q == e
    return np.where(e >= 0, ok_hit, pe_q < 0)


def valid_taps(w, h, pv, o, d, t, e, pt, pe, color, depth_tolerance, flags):
    """(q, b, valid bool[4, n]) of step 4"""
    inside, fx, fy, r = project(w, h, pv, o, d, t, e)
    q, b, usable = taps(w, h, inside, fx, fy)
    c = color.astype(F, copy=False)[q]                                    # (4, n, 4)
    with np.errstate(all="ignore"):
        good = np.isfinite(c).all(axis=2) & (c[:, :, 3] >= F(1))
    return q, b, usable & matches(q, e[None, :], r[None, :], pt, pe, depth_tolerance, flags) & good


def _blend(b, valid, weight, cap, channels):
    """The several-taps rule for one weight channel (color.w, or the moments' n) and its data channels (a list of (4, n) arrays).
    Returns (count int[n], history n float32[n], [(sum / B) * n per channel])."""
    n_pix = b.shape[1]
    B = np.zeros(n_pix, F)
    sums = [np.zeros(n_pix, F) for _ in channels]
    hist = np.full(n_pix, np.inf, F)
    with np.errstate(all="ignore"):
        for k in range(4):
            v = valid[k]
            u = (b[k] / weight[k]).astype(F)
            B = np.where(v, B + b[k], B)
            for j, x in enumerate(channels):
                sums[j] = np.where(v, sums[j] + u * x[k], sums[j]).astype(F)
            hist = np.where(v, np.minimum(hist, np.minimum(weight[k], cap)), hist).astype(F)
        out = [((s / B) * hist).astype(F) for s in sums]
    return valid.sum(axis=0), hist, out


def reproject_bilinear(w, h, pv, o, d, t, e, pt, pe, previous, depth_tolerance, max_history, flags, moments=None, max_batches=None):
    """Arguments as reproject_reference.reproject, plus moments (n, 3) and max_batches.  Returns ({the four keys}, source int32[n], moments (n, 3) or None,
    valid bool[4, n])."""
    n = w * h
    q, b, valid = valid_taps(w, h, pv, o, d, t, e, pt, pe, previous["color"], depth_tolerance, flags)
    cap = F(max_history)
    col = previous["color"].astype(F, copy=False)[q]                      # (4, n, 4)
    data = {"color": col, "normal": previous["normal"].astype(F, copy=False)[q], "albedo": previous["albedo"].astype(F, copy=False)[q],
            "scw": previous["scw"].astype(F, copy=False)[q][:, :, None]}
    channels = [data[key][:, :, j] for key in KEYS for j in range(3 if key != "scw" else 1)]
    count, hist, blended = _blend(b, valid, col[:, :, 3], cap, channels)
    # the heaviest valid tap, the first among equals
    heavy = np.argmax(np.where(valid, b, F(-1)), axis=0)
    src = np.where(count > 0, q[heavy, np.arange(n)], -1)
    g = np.where(src >= 0, src, 0)
    # one valid tap: step 4 of the nearest call at it
    with np.errstate(all="ignore"):
        c1 = previous["color"].astype(F, copy=False)[g]
        scale = c1[:, 3] > cap
        k1 = np.where(scale, cap / c1[:, 3], F(1)).astype(F)
    out, at = {}, 0
    for key in KEYS:
        width = 3 if key != "scw" else 1
        several = np.stack(blended[at:at + width], axis=1)
        at += width
        x1 = previous[key].astype(F, copy=False)[g].reshape(n, -1)[:, :width]
        with np.errstate(all="ignore"):
            single = np.where(scale[:, None], x1 * k1[:, None], x1).astype(F)
        val = np.where((count == 1)[:, None], single, np.where((count > 1)[:, None], several, F(0))).astype(F)
        if key == "color":
            w1 = np.where(scale, cap, c1[:, 3])
            val = np.concatenate([val, np.where(count == 1, w1, np.where(count > 1, hist, F(0))).astype(F)[:, None]], axis=1)
        out[key] = val if key != "scw" else val[:, 0]
    assert out["color"].shape == (n, 4) and out["color"].dtype == F
    out_m = None
    if moments is not None:
        capm = F(max_batches)
        m = moments.astype(F, copy=False)[q]                              # (4, n, 3)
        with np.errstate(all="ignore"):
            part = valid & np.isfinite(m).all(axis=2) & (m[:, :, 2] >= F(1))
        countm, histm, (s1, s2) = _blend(b, part, m[:, :, 2], capm, [m[:, :, 0], m[:, :, 1]])
        only = q[np.argmax(part, axis=0), np.arange(n)]
        m1 = moments.astype(F, copy=False)[np.where(countm == 1, only, 0)]
        with np.errstate(all="ignore"):
            sc = m1[:, 2] > capm
            km = np.where(sc, capm / m1[:, 2], F(1)).astype(F)
            single = np.where(sc[:, None], np.stack([m1[:, 0] * km, m1[:, 1] * km, np.full(n, capm, F)], axis=1), m1).astype(F)
        several = np.stack([s1, s2, histm], axis=1)
        out_m = np.where((countm == 1)[:, None], single, np.where((countm > 1)[:, None], several, F(0))).astype(F)
    return out, src.astype(np.int32), out_m, valid
