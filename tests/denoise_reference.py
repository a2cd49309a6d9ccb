"""numpy float32 restatement of rtowDenoiseDevice (include/rtow.h): the edge-avoiding a-trous filter, vectorised over pixels with the
25-tap loop in the specification's order (j outer, i inner).  Every operation is one float32 operation of the specification - no contraction, correctly
rounded division, no exp / pow - so the result is the kernel's, bit for bit.  A helper of the tests, not a test."""
import numpy as np

F = np.float32
H = [F(1.0 / 16), F(1.0 / 4), F(3.0 / 8), F(1.0 / 4), F(1.0 / 16)]      # h(-2..2): exact binary fractions
DEMOD_MIN = F(2.0 ** -10)
DEMODULATE_ALBEDO = 1


def _dist2(a, b):
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def demodulate(c, a):
    with np.errstate(all="ignore"):
        return np.where(a >= DEMOD_MIN, c / a, c).astype(F)


def remodulate(r, a):
    with np.errstate(all="ignore"):
        return np.where(a >= DEMOD_MIN, r * a, r).astype(F)


def _level(c, n, a, step, sharpness, inv_c, inv_a):
    """one a-trous level on (h, w, 3) arrays; inv_c / inv_a None = that term off"""
    h, w, _ = c.shape
    acc = np.zeros_like(c)
    ws = np.zeros((h, w), F)
    nz = (n == 0).all(-1)
    with np.errstate(all="ignore"):
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
                    continue
                cp, cq = c[P], c[Q]
                wc = F(1) / (F(1) + _dist2(cp, cq) * inv_c) if inv_c is not None else F(1)
                d = (n[P][..., 0] * n[Q][..., 0] + n[P][..., 1] * n[Q][..., 1]) + n[P][..., 2] * n[Q][..., 2]
                d = np.where(d > 0, d, F(0)).astype(F)
                for _ in range(sharpness):
                    d = d * d
                zp, zq = nz[P], nz[Q]
                wn = np.where(zp & zq, F(1), np.where(zp | zq, F(0), d)).astype(F)
                wa = F(1) / (F(1) + _dist2(a[P], a[Q]) * inv_a) if inv_a is not None else F(1)
                wgt = (((hij * wc) * wn) * wa).astype(F)
                take = np.isfinite(cq).all(-1) & (wgt > 0)                 # skipped taps add nothing (not + 0)
                acc[P] = np.where(take[..., None], acc[P] + wgt[..., None] * cq, acc[P])
                ws[P] = np.where(take, ws[P] + wgt, ws[P])
        out = acc / ws[..., None]
    return np.where(np.isfinite(c).all(-1)[..., None], out, c).astype(F)    # a non-finite pixel passes through


def denoise_levels(width, height, color, normal, albedo, iterations=5, normal_sharpness=7, color_sigma=0.5, albedo_sigma=0.1, flags=DEMODULATE_ALBEDO):
    """the output of every level, BEFORE the final remodulation: level k of this list is what a call with iterations = k + 1 remodulates"""
    shape = (height, width, 3)
    c = np.ascontiguousarray(color, F).reshape(shape)
    n = np.ascontiguousarray(normal, F).reshape(shape)
    a = np.ascontiguousarray(albedo, F).reshape(shape)
    if flags & DEMODULATE_ALBEDO:
        c = demodulate(c, a)
    sc, sa = F(color_sigma), F(albedo_sigma)
    inv_a = F(1) / (sa * sa) if sa != 0 else None
    out = []
    with np.errstate(all="ignore"):
        for k in range(iterations):
            inv_c = F(1 << (2 * k)) / (sc * sc) if sc != 0 else None
            c = _level(c, n, a, 1 << k, normal_sharpness, inv_c, inv_a)
            out.append(c)
    return out


def finish(level_output, albedo, flags=DEMODULATE_ALBEDO):
    """the call's result from the last level's output: remodulated with the flag, flattened to (n, 3)"""
    r = level_output.reshape(-1, 3)
    return remodulate(r, np.ascontiguousarray(albedo, F).reshape(-1, 3)) if flags & DEMODULATE_ALBEDO else r.copy()


def denoise_reference(width, height, color, normal, albedo, iterations=5, normal_sharpness=7, color_sigma=0.5, albedo_sigma=0.1, flags=DEMODULATE_ALBEDO):
    """rtowDenoiseDevice's outColor, (width * height, 3) float32"""
    levels = denoise_levels(width, height, color, normal, albedo, iterations, normal_sharpness, color_sigma, albedo_sigma, flags)
    return finish(levels[-1], albedo, flags)
