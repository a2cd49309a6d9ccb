"""A numpy restatement of rtowMeterExposureDevice and rtowFinalizeToneMappedDevice as include/rtow.h specifies them: float32 with every operation rounded on its own,
Python integers for the ranks (no wider than the uint64 the header names), the deterministic exp2 from the oracle's own copy through a small host shim
(tests/native/tonemap_detmath_shim.cpp - its fmaf chain is not emulated here), and the bytes from oracle.finalize applied to the curve's output.  Nothing here reads the
product's kernels.  tests/test_tonemap_reference.py holds this file to hand-computed cases; tests/test_gpu_tonemap.py compares the device with it bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BINS = 256
RECORD_WORDS = 264                                                         # RtowExposureState: 8 words, then the histogram
CLAMP, ACES_FITTED, ACES_FILM = 0, 1, 2
CURVES = (CLAMP, ACES_FITTED, ACES_FILM)
LOG2_GREY = F(np.log2(0.18))                                               # the recommended compensation
RECOMMENDED = dict(low=500, high=950, compensation=LOG2_GREY, min_stops=F(-8), max_stops=F(8), rate=F(1))

_shim = None


def det_exp2(t):
    """dm_exp2f of oracle/detmath.h on one float32"""
    global _shim
    if _shim is None:
        out_dir = os.path.join(ROOT, "tests", "build")
        os.makedirs(out_dir, exist_ok=True)
        src, so = os.path.join(ROOT, "tests", "native", "tonemap_detmath_shim.cpp"), os.path.join(out_dir, "libtonemap_detmath_shim.so")
        deps = [src, os.path.join(ROOT, "oracle", "detmath.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", src, "-o", so], check=True, capture_output=True)
        _shim = C.CDLL(so)
        _shim.shim_det_exp2.restype = C.c_float
        _shim.shim_det_exp2.argtypes = [C.c_float]
    return F(_shim.shim_det_exp2(C.c_float(float(t))))


# ---------------------------------------------------------------- the meter
def luminance(color):
    c = np.asarray(color, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return (F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]) + F(0.0722) * c[:, 2]


def bin_of(l):
    """the bin of each luminance, -1 where the pixel is not metered"""
    l = np.asarray(l, F).reshape(-1)
    with np.errstate(all="ignore"):
        metered = np.isfinite(l) & (l >= F(2.0 ** -16))
    b = np.minimum((l.view(np.uint32) >> np.uint32(20)).astype(np.int64) - 0x378, BINS - 1)
    return np.where(metered, b, -1)


def histogram(color):
    b = bin_of(luminance(color))
    return np.bincount(b[b >= 0], minlength=BINS).astype(np.uint32)


def zero_state():
    return dict(exposure=F(0), stops=F(0), targetStops=F(0), meanLog2=F(0), valid=0, metered=0, ignored=0, reserved=0, histogram=np.zeros(BINS, np.uint32))


def _max(a, b):
    return a if a > b else b


def _min(a, b):
    return a if a < b else b


def resolve(hist, pixels, state, low, high, compensation, min_stops, max_stops, rate):
    """the record after a call whose frame has the histogram `hist`, from the record `state` before it"""
    hist = [int(x) for x in hist]
    compensation, min_stops, max_stops, rate, stops = F(compensation), F(min_stops), F(max_stops), F(rate), F(state["stops"])
    valid = int(state["valid"])
    metered = sum(hist)
    lo, hi = metered * int(low) // 1000, metered * int(high) // 1000
    n = hi - lo
    s_sum, cum = 0, 0
    for b, count in enumerate(hist):                                       # bin b owns the ranks [cum, cum + count)
        s_sum += b * max(0, min(cum + count, hi) - max(cum, lo))
        cum += count
    if n > 0:
        q = (s_sum * 256 + n // 2) // n
        mean = (F(q) * F(2.0 ** -11) - F(16)) + F(2.0 ** -4)
        target = compensation - mean
    else:
        mean = F(0)
        target = stops if valid else F(0)
    target_stops = _min(_max(target, min_stops), max_stops)
    s = stops + (target_stops - stops) * rate if (valid != 0 and rate < F(1)) else target_stops
    new_stops = _min(_max(F(s), min_stops), max_stops)
    return dict(exposure=det_exp2(new_stops), stops=F(new_stops), targetStops=F(target_stops), meanLog2=F(mean), valid=1 if n > 0 else valid, metered=metered,
                ignored=int(pixels) - metered, reserved=0, histogram=np.asarray(hist, np.uint32))


def meter(color, state, low=500, high=950, compensation=LOG2_GREY, min_stops=-8, max_stops=8, rate=1):
    color = np.asarray(color, F).reshape(-1, 3)
    return resolve(histogram(color), color.shape[0], state, low, high, compensation, min_stops, max_stops, rate)


def record(state):
    """the 264 words of RtowExposureState"""
    out = np.zeros(RECORD_WORDS, np.uint32)
    out[0:4] = np.array([state["exposure"], state["stops"], state["targetStops"], state["meanLog2"]], F).view(np.uint32)
    out[4:8] = [state["valid"], state["metered"], state["ignored"], state["reserved"]]
    out[8:] = state["histogram"]
    return out


def state_of(words):
    words = np.asarray(words, np.uint32)
    f = words[0:4].view(F)
    return dict(exposure=f[0], stops=f[1], targetStops=f[2], meanLog2=f[3], valid=int(words[4]), metered=int(words[5]), ignored=int(words[6]), reserved=int(words[7]),
                histogram=words[8:].copy())


# ---------------------------------------------------------------- the tone-mapped finalize
ACES_INPUT = ((0.59719, 0.35458, 0.04823), (0.07600, 0.90834, 0.01566), (0.02840, 0.13383, 0.83777))          # UTIL/Tools.cs:198-201
ACES_OUTPUT = ((1.60475, -0.53108, -0.07367), (-0.10208, 1.10813, -0.00605), (-0.00327, -0.07276, 1.07602))  # UTIL/Tools.cs:204-208


def scale_of(exposure, state=None):
    """s of the specification"""
    if state is None:
        return F(exposure)
    return F(exposure) * (F(state["exposure"]) if int(state["valid"]) else F(1))


def _rows(m, v):
    return np.stack([(F(r[0]) * v[:, 0] + F(r[1]) * v[:, 1]) + F(r[2]) * v[:, 2] for r in m], axis=1)


def tone(color, curve, s):
    """y of the specification: float32 (n, 3)"""
    c = np.asarray(color, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        x = c * F(s)
        x = np.where(x > F(0), x, F(0)).astype(F)                          # a NaN gives 0, and so does -0
        x = np.where(x < F(65536), x, F(65536)).astype(F)
        if curve == CLAMP:
            return x
        if curve == ACES_FILM:
            return ((x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))).astype(F)
        assert curve == ACES_FITTED
        v = _rows(ACES_INPUT, x)
        a = v * (v + F(0.0245786)) - F(0.000090537)
        b = v * (F(0.983729) * v + F(0.4329510)) + F(0.238081)
        return _rows(ACES_OUTPUT, (a / b).astype(F)).astype(F)


def finalize(oracle, color, normal, albedo, curve, exposure, state=None):
    """the three RGBA32 textures; a guide given as None comes back as None"""
    y = tone(color, curve, scale_of(exposure, state))
    n = y.shape[0]
    zeros = np.zeros((n, 3), F)
    oc, on, oa = oracle.finalize(y, zeros if normal is None else np.asarray(normal, F).reshape(n, 3), zeros if albedo is None else np.asarray(albedo, F).reshape(n, 3))
    return oc, (None if normal is None else on), (None if albedo is None else oa)


# ---------------------------------------------------------------- frames
def pred(x):
    return np.nextafter(F(x), F(-np.inf))


def color_with_luminance(target, rng):
    """a colour whose luminance, as the specification adds it up, is exactly `target` (found by search: nudge the green channel by a few ulps)"""
    target = F(target)
    for _ in range(4000):
        r, b = F(target * F(rng.uniform(0.0, 1.5))), F(target * F(rng.uniform(0.0, 1.5)))
        g0 = F((np.float64(target) - 0.2126 * np.float64(r) - 0.0722 * np.float64(b)) / 0.7152)
        if not g0 > 0:
            continue
        for k in range(-3, 4):
            cand = np.array([[r, np.uint32(int(g0.view(np.uint32)) + k).view(F), b]], F)      # k ulps from g0
            if luminance(cand)[0] == target:
                return cand[0]
    raise AssertionError("no colour found for luminance %r" % target)


def border_luminances():
    """exact bin borders and their predecessors, the two ends of the metered range included"""
    out = [F(2.0 ** -16), pred(2.0 ** -16), F(2.0 ** 16), pred(2.0 ** 16)]
    for k in (-15, -7, 0, 3, 15):
        out += [F(2.0 ** k), pred(2.0 ** k), F(2.0 ** k * 1.125), pred(2.0 ** k * 1.125)]
    return out


def make_frame(n, seed):
    """A seeded float3 frame of n pixels.  Luminances are stratified over the 320 eighth-octave steps from 2^-20 to 2^20 (linear in the mantissa, like the bins), so a
    frame of 320 pixels and more visits every bin, the stretch below 2^-16 that is ignored and the stretch from 2^16 up that bin 255 collects; frames of 64 pixels and
    more also carry the specials: NaN, +-inf, -0, negatives, denormals, zero, and colours whose luminance is exactly a bin border or the float before it."""
    rng = np.random.default_rng(seed)
    steps = rng.permutation(320)[np.arange(n) % 320] - 32                   # eighth-octaves from 2^-16
    lum = np.ldexp(1.0 + ((steps % 8) + rng.uniform(0, 1, n)) / 8.0, -16 + steps // 8)
    hue = rng.uniform(0.2, 1.8, (n, 3))
    hue /= (0.2126 * hue[:, 0] + 0.7152 * hue[:, 1] + 0.0722 * hue[:, 2])[:, None]
    frame = (hue * lum[:, None]).astype(F)
    if n >= 64:
        nan, inf = F(np.nan), F(np.inf)
        specials = [[nan, 1, 1], [1, nan, 1], [1, 1, nan], [inf, 0, 0], [0, -inf, 0], [inf, -inf, 0], [-0.0, -0.0, -0.0], [0, 0, 0], [-1, -2, -3], [-5, 0.25, 0.25],
                    [1e-40, 1e-40, 1e-40], [3e-39, 0, 1e-45], [3e38, 3e38, 3e38], [1e-6, 1e-6, 1e-6]]
        specials += [color_with_luminance(l, rng) for l in border_luminances()]
        at = rng.choice(n, len(specials), replace=False)
        frame[at] = np.array(specials, F)
    return frame


def make_guides(n, seed):
    """normals and albedos for the finalize pass: unit-ish vectors and colours, with the values the byte conversion treats specially"""
    rng = np.random.default_rng(seed + 77)
    normal = rng.uniform(-1.2, 1.2, (n, 3)).astype(F)
    albedo = rng.uniform(-0.1, 1.3, (n, 3)).astype(F)
    if n >= 64:
        at = rng.choice(n, 8, replace=False)
        normal[at[:4]] = np.array([[np.nan, 0, 1], [np.inf, -np.inf, 0], [-1, 1, -0.0], [1e-40, -1e-40, 0]], F)
        albedo[at[4:]] = np.array([[np.nan, 0, 1], [np.inf, -np.inf, 0.5], [-0.0, 1e-40, 1], [0.0031308, 0.5, 255]], F)
    return normal, albedo
