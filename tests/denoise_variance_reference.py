"""numpy float32 restatement of rtowAccumulateMomentsDevice and rtowDenoiseVarianceDevice (include/rtow.h): the batch moments of the luminance and
the variance-guided a-trous filter, vectorised over pixels with the tap loops in the specification's order (j outer, i inner).  Every operation is one float32
operation of the specification - no contraction, correctly rounded division, no exp / pow / sqrt - so the result is the kernels', bit for bit.  The taps, skip
rules and guide weights are tests/denoise_reference.py's, statement for statement.  A helper of the tests, not a test."""
import numpy as np

import denoise_reference as dr

F = np.float32
H = dr.H
T = [F(0.25), F(0.5), F(0.25)]                   # the 3 x 3 variance filter, t(-1..1)
DEMOD_MIN = dr.DEMOD_MIN
DEMODULATE_ALBEDO = dr.DEMODULATE_ALBEDO
UNKNOWN = F(-1)
EPS = F(2.0 ** -20)


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def accumulate_moments(colors, moments=None):
    """rtowAccumulateMomentsDevice: colors = a sequence of (n, 4) float32 arrays in batch order, moments = (n, 3) or None (zeros); returns (n, 3) (s1, s2, n)"""
    colors = [np.ascontiguousarray(c, F).reshape(-1, 4) for c in colors]
    m = np.zeros((colors[0].shape[0], 3), F) if moments is None else np.ascontiguousarray(moments, F).reshape(-1, 3).copy()
    s1, s2, n = m[:, 0].copy(), m[:, 1].copy(), m[:, 2].copy()
    with np.errstate(all="ignore"):
        for c in colors:
            w = c[:, 3]
            mean = c[:, :3] / w[:, None]
            l = lum(mean)
            take = (w > 0) & np.isfinite(l)                                # NaN w fails w > 0
            s1 = np.where(take, s1 + l, s1)
            s2 = np.where(take, s2 + l * l, s2)
            n = np.where(take, n + F(1), n)
    return np.stack([s1, s2, n], axis=1).astype(F)


def initial_variance(moments, albedo, flags=DEMODULATE_ALBEDO):
    """v0 per pixel, (n,) float32: the variance of the mean of the batches' luminances, -1 = unknown"""
    m = np.ascontiguousarray(moments, F).reshape(-1, 3)
    a = np.ascontiguousarray(albedo, F).reshape(-1, 3)
    s1, s2, n = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(all="ignore"):
        mean = s1 / n
        d = s2 - s1 * mean
        d = np.where(d > 0, d, F(0)).astype(F)
        v = d / (n * (n - F(1)))
        ok = (n >= 2) & np.isfinite(v)
        if flags & DEMODULATE_ALBEDO:
            la = lum(a)
            v = np.where(la >= DEMOD_MIN, v / (la * la), v).astype(F)
    return np.where(ok, v, UNKNOWN).astype(F)


def _filtered_variance(v):
    """g = num / den over the known in-image taps of the 3 x 3 neighbourhood (h, w); meaningful where v itself is known (then den > 0)"""
    h, w = v.shape
    num, den = np.zeros((h, w), F), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for j in range(-1, 2):
            for i in range(-1, 2):
                y0, y1, x0, x1 = max(0, -j), min(h, h - j), max(0, -i), min(w, w - i)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                vq = v[y0 + j:y1 + j, x0 + i:x1 + i]
                g = T[i + 1] * T[j + 1]
                take = vq >= 0
                num[P] = np.where(take, num[P] + g * vq, num[P])
                den[P] = np.where(take, den[P] + g, den[P])
        return num / den


def _level(c, n, a, v, step, sharpness, sigma2, inv_a):
    """one level on (h, w, 3) colours / guides and the (h, w) variance plane; sigma2 / inv_a None = that term off; returns (colour, variance)"""
    h, w, _ = c.shape
    acc = np.zeros_like(c)
    ws = np.zeros((h, w), F)
    vacc = np.zeros((h, w), F)
    nz = (n == 0).all(-1)
    known = v >= 0                                                         # -1 and NaN: no estimate
    with np.errstate(all="ignore"):
        use_c = known if sigma2 is not None else np.zeros((h, w), bool)
        inv_c = F(1) / (sigma2 * _filtered_variance(v) + EPS) if sigma2 is not None else np.zeros((h, w), F)
        l = lum(c)
        for j in range(-2, 3):
            for i in range(-2, 3):
                dy, dx = j * step, i * step
                y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                if y0 >= y1 or x0 >= x1:
                    continue                                               # every tap of this offset lies outside the image
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                hij = H[i + 2] * H[j + 2]
                if i == 0 and j == 0:                                      # the centre: 9/64, no guide consulted
                    acc[P] = acc[P] + hij * c[P]
                    ws[P] = ws[P] + hij
                    vacc[P] = np.where(known[P], vacc[P] + (hij * hij) * v[P], vacc[P])
                    continue
                cq = c[Q]
                dl = l[P] - l[Q]
                wc = np.where(use_c[P], F(1) / (F(1) + (dl * dl) * inv_c[P]), F(1)).astype(F)
                d = (n[P][..., 0] * n[Q][..., 0] + n[P][..., 1] * n[Q][..., 1]) + n[P][..., 2] * n[Q][..., 2]
                d = np.where(d > 0, d, F(0)).astype(F)
                for _ in range(sharpness):
                    d = d * d
                zp, zq = nz[P], nz[Q]
                wn = np.where(zp & zq, F(1), np.where(zp | zq, F(0), d)).astype(F)
                wa = F(1) / (F(1) + dr._dist2(a[P], a[Q]) * inv_a) if inv_a is not None else F(1)
                wgt = (((hij * wc) * wn) * wa).astype(F)
                take = np.isfinite(cq).all(-1) & (wgt > 0)                 # skipped taps add nothing (not + 0)
                acc[P] = np.where(take[..., None], acc[P] + wgt[..., None] * cq, acc[P])
                ws[P] = np.where(take, ws[P] + wgt, ws[P])
                vq = v[Q]
                vacc[P] = np.where(take & known[P] & (vq >= 0), vacc[P] + (wgt * wgt) * vq, vacc[P])      # a tap without an estimate adds to the colour only
        out = acc / ws[..., None]
        vout = vacc / (ws * ws)
        vout = np.where(vout >= 0, vout, UNKNOWN).astype(F)               # 0 * inf: no NaN is ever stored
    through = ~np.isfinite(c).all(-1)                                      # a non-finite pixel passes through and keeps its variance
    cout = np.where(through[..., None], c, out).astype(F)
    vout = np.where(known, np.where(through, v, vout), UNKNOWN).astype(F)
    return cout, vout


def denoise_variance_levels(width, height, color, normal, albedo, moments, iterations=5, normal_sharpness=2, color_sigma=2.0, albedo_sigma=0.125,
                            flags=DEMODULATE_ALBEDO, v0=None):
    """(colour, variance) of every level, the colour BEFORE the final remodulation: level k of this list is what a call with iterations = k + 1 remodulates and
    writes to outVariance.  v0 (optional): the initial variance plane instead of the one the moments give (for known-answer tests)"""
    shape = (height, width, 3)
    c = np.ascontiguousarray(color, F).reshape(shape)
    n = np.ascontiguousarray(normal, F).reshape(shape)
    a = np.ascontiguousarray(albedo, F).reshape(shape)
    v = (initial_variance(moments, albedo, flags) if v0 is None else np.ascontiguousarray(v0, F)).reshape(height, width)
    if flags & DEMODULATE_ALBEDO:
        c = dr.demodulate(c, a)
    sc, sa = F(color_sigma), F(albedo_sigma)
    sigma2 = sc * sc if sc != 0 else None
    inv_a = F(1) / (sa * sa) if sa != 0 else None
    out = []
    for k in range(iterations):
        c, v = _level(c, n, a, v, 1 << k, normal_sharpness, sigma2, inv_a)
        out.append((c, v))
    return out


def finish(level_output, albedo, flags=DEMODULATE_ALBEDO):
    """the call's (outColor (n, 3), outVariance (n,)) from the last level's output"""
    c, v = level_output
    return dr.finish(c, albedo, flags), v.reshape(-1).copy()


def denoise_variance_reference(width, height, color, normal, albedo, moments, iterations=5, normal_sharpness=2, color_sigma=2.0, albedo_sigma=0.125,
                               flags=DEMODULATE_ALBEDO):
    """rtowDenoiseVarianceDevice's (outColor, outVariance)"""
    levels = denoise_variance_levels(width, height, color, normal, albedo, moments, iterations, normal_sharpness, color_sigma, albedo_sigma, flags)
    return finish(levels[-1], albedo, flags)
