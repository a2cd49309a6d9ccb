"""A numpy restatement of rtowBloomDevice as include/rtow.h specifies it: float32 with every operation rounded on its own, min and max as selects, the taps accumulated
one by one in the stated order (j outer, i inner) - vectorised over index arrays, never over taps.  Nothing here reads the product's kernels.
tests/test_bloom_reference.py holds this file to three properties that follow from the specification alone; tests/test_gpu_bloom.py compares the device with it bit
for bit."""
import numpy as np

F = np.float32
H = (F(0.125), F(0.375), F(0.375), F(0.125))
KARIS = 1
MAX_LEVELS = 8
RECOMMENDED = dict(levels=6, threshold=F(1), knee=F(0.5), scatter=F(0.7), karis=True)


def mip_sizes(w, h, levels=MAX_LEVELS):
    """(W_k, H_k) for k = 1 .. levels"""
    return [(-(-w // (1 << k)), -(-h // (1 << k))) for k in range(1, levels + 1)]


def _max(a, b):
    return np.where(a > b, a, b).astype(F)


def _min(a, b):
    return np.where(a < b, a, b).astype(F)


def lum(v):
    return (F(0.2126) * v[..., 0] + F(0.7152) * v[..., 1]) + F(0.0722) * v[..., 2]


def bright_pass(c, s, threshold, knee, karis):
    """b (h, w, 3) and wk (h, w) of the frame c (h, w, 3)"""
    s, threshold, knee = F(s), F(threshold), F(knee)
    with np.errstate(all="ignore"):
        q = np.where(c > F(0), c, F(0)).astype(F)
        q = np.where(q < F(65536), q, F(65536)).astype(F)
        le = lum(q) * s
        d = le - threshold
        k = F(threshold * knee)
        if k > F(0):
            r = _min(_max(d + k, F(0)), F(2) * k)
            m = _max((r * r) / (F(4) * k), d)
        else:
            m = d
        m = np.where(m > F(0), m, F(0)).astype(F)
        g = np.where((le > F(0)) & (le < F(np.inf)), m / le, F(0)).astype(F)
        b = (q * g[..., None]).astype(F)
        wk = (F(1) / (F(1) + lum(b) * s)).astype(F) if karis else np.ones(le.shape, F)
    return b, wk


def downsample(src, weights=None):
    """the sixteen clamped taps of every texel of the next mip; with `weights` (mip 1): w = (h_j * h_i) * wk and the texel is acc / wsum, 0 when wsum is not > 0"""
    h, w = src.shape[:2]
    dh, dw = (h + 1) // 2, (w + 1) // 2
    ys, xs = 2 * np.arange(dh) - 1, 2 * np.arange(dw) - 1
    acc, wsum = np.zeros((dh, dw, 3), F), np.zeros((dh, dw), F)
    with np.errstate(all="ignore"):
        for j in range(4):
            yy = np.clip(ys + j, 0, h - 1)
            for i in range(4):
                at = np.ix_(yy, np.clip(xs + i, 0, w - 1))
                hw = F(H[j] * H[i])
                if weights is None:
                    acc = acc + hw * src[at]
                else:
                    wt = (hw * weights[at]).astype(F)
                    acc = acc + wt[..., None] * src[at]
                    wsum = wsum + wt
        if weights is None:
            return acc.astype(F)
        return np.where((wsum > F(0))[..., None], acc / wsum[..., None], F(0)).astype(F)


def _tent_axis(n, coarse):
    x = np.arange(n)
    odd = (x & 1) == 1
    base = np.where(odd, x // 2, x // 2 - 1)
    return ((np.clip(base, 0, coarse - 1), np.clip(base + 1, 0, coarse - 1)),
            (np.where(odd, F(0.75), F(0.25)).astype(F), np.where(odd, F(0.25), F(0.75)).astype(F)))


def tent(U, fh, fw):
    """Up(U) at the fh x fw texels of the finer level"""
    ch, cw = U.shape[:2]
    (ys, uy), (xs, ux) = _tent_axis(fh, ch), _tent_axis(fw, cw)
    acc = np.zeros((fh, fw, 3), F)
    with np.errstate(all="ignore"):
        for j in range(2):
            for i in range(2):
                wt = (uy[j][:, None] * ux[i][None, :]).astype(F)
                acc = acc + wt[..., None] * U[np.ix_(ys[j], xs[i])]
    return acc.astype(F)


def bloom(color, w, h, levels, threshold, knee, scatter, intensity, s=1.0, karis=True):
    """{"out": float32 (n, 3), "layer": Up(U_1) (n, 3), "mips": U_1 .. U_levels as the scratch holds them after the call}"""
    c = np.asarray(color, F).reshape(h, w, 3)
    b, wk = bright_pass(c, s, threshold, knee, karis)
    mips = [downsample(b, wk)]
    for _ in range(2, levels + 1):
        mips.append(downsample(mips[-1]))
    scatter, intensity = F(scatter), F(intensity)
    with np.errstate(all="ignore"):
        for k in range(levels - 2, -1, -1):
            mips[k] = (mips[k] + scatter * tent(mips[k + 1], *mips[k].shape[:2])).astype(F)
        layer = tent(mips[0], h, w)
        out = np.where(np.isfinite(c).all(axis=2)[..., None], c + intensity * layer, c).astype(F)
    return {"out": out.reshape(-1, 3), "layer": layer.reshape(-1, 3), "mips": mips}


def scratch_words(mips):
    """the pyramid as the scratch holds it: the mips one behind the other, (r, g, b, 0) per texel, as uint32 words"""
    out = []
    for m in mips:
        texels = np.zeros(m.shape[:2] + (4,), F)
        texels[..., :3] = m
        out.append(texels.reshape(-1))
    return np.concatenate(out).view(np.uint32)
