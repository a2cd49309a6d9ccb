"""CPU: the numpy restatement of rtowMeterExposureDevice and rtowFinalizeToneMappedDevice (tests/tonemap_reference.py) held to cases worked out by hand from the
specification in include/rtow.h - the bin borders, a two-bin frame's trimmed mean, empty rank ranges and empty frames, the temporal step, and the header's consequence
that CLAMP with exposure 1 is rtowFinalizeDevice - and the generated frames to the coverage the GPU tests rely on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tonemap_reference as tm  # noqa: E402

F = np.float32


def test_bin_borders():
    assert tm.bin_of([F(2.0 ** -16)])[0] == 0 and tm.bin_of([tm.pred(2.0 ** -16)])[0] == -1
    for k in range(-15, 17):
        at, before = tm.bin_of([F(2.0 ** k)])[0], tm.bin_of([tm.pred(2.0 ** k)])[0]
        assert at == min(8 * (k + 16), 255) and before == 8 * (k + 16) - 1, k             # neighbouring bins, until bin 255 takes both
    assert tm.bin_of([F(2.0 ** 16)])[0] == 255 and tm.bin_of([F(3e38)])[0] == 255 and tm.bin_of([F(np.inf)])[0] == -1
    assert list(tm.bin_of(np.array([np.nan, -np.inf, -0.0, 0.0, -1.0, 1e-40, 1e-6], F))) == [-1] * 7
    # eight bins per octave, linear in the mantissa
    assert list(tm.bin_of(np.array([1.0, 1.124, 1.125, 1.25, 1.875, 1.9999], F))) == [128, 128, 129, 130, 135, 135]


def test_the_luminance_is_added_in_the_stated_order():
    c = np.array([[1.0, 1.0, 1.0], [3.0, 0.1, 7.0]], F)
    want = [(F(0.2126) * x[0] + F(0.7152) * x[1]) + F(0.0722) * x[2] for x in c]
    assert list(tm.luminance(c)) == want
    rng = np.random.default_rng(5)
    for l in tm.border_luminances():
        assert tm.luminance(tm.color_with_luminance(l, rng)[None, :])[0] == l


def test_a_two_bin_frame_by_hand():
    """60 pixels of luminance 1 (bin 128) and 40 of luminance 4 (bin 144).  Ranks 0..59 belong to bin 128, 60..99 to bin 144."""
    frame = np.array([[1, 1, 1]] * 60 + [[4, 4, 4]] * 40, F)
    assert list(tm.bin_of(tm.luminance(frame))) == [128] * 60 + [144] * 40
    zero = tm.zero_state()
    # every rank: S = 128 * 60 + 144 * 40 = 13440, Q = (13440 * 256 + 50) / 100 = 34406, meanLog2 = 34406 / 2048 - 16 + 1 / 16
    s = tm.meter(frame, zero, low=0, high=1000, compensation=0.0, min_stops=-32, max_stops=32, rate=1)
    assert (s["metered"], s["ignored"], s["valid"], s["reserved"]) == (100, 0, 1, 0) and s["histogram"][128] == 60 and s["histogram"][144] == 40
    assert s["histogram"].sum() == 100
    assert s["meanLog2"] == F(34406 / 2048.0 - 16 + 0.0625) and s["targetStops"] == -s["meanLog2"] == s["stops"]
    assert s["exposure"] == tm.det_exp2(s["stops"]) and abs(float(s["exposure"]) - 2.0 ** float(s["stops"])) < 1e-6
    # ranks [50, 95): 10 of bin 128 and 35 of bin 144: S = 1280 + 5040 = 6320, N = 45, Q = (6320 * 256 + 22) / 45 = 35954
    s = tm.meter(frame, zero, low=500, high=950, compensation=0.0, min_stops=-32, max_stops=32, rate=1)
    assert s["meanLog2"] == F(35954 / 2048.0 - 16 + 0.0625)
    # ranks [60, 100): bin 144 alone - its centre is log2-linear 2 + 1 / 16
    s = tm.meter(frame, zero, low=600, high=1000, compensation=0.0, min_stops=-32, max_stops=32, rate=1)
    assert s["meanLog2"] == F(2.0625)
    # the stop limits cut the target, and the compensation moves it
    s = tm.meter(frame, zero, low=600, high=1000, compensation=tm.LOG2_GREY, min_stops=-1, max_stops=1, rate=1)
    assert s["targetStops"] == F(-1) == s["stops"] and s["exposure"] == F(0.5)
    s = tm.meter(frame, zero, low=600, high=1000, compensation=5.0, min_stops=-1, max_stops=1, rate=1)
    assert s["targetStops"] == F(1) and s["exposure"] == F(2)


def test_empty_rank_ranges_and_empty_frames():
    frame = np.array([[1, 1, 1]] * 7, F)
    zero = tm.zero_state()
    for low, high in ((300, 300), (1000, 1000), (0, 0), (0, 100)):           # 7 * 100 / 1000 = 0: no rank either
        s = tm.meter(frame, zero, low=low, high=high)
        assert (s["valid"], s["metered"], s["ignored"]) == (0, 7, 0) and s["meanLog2"] == 0 and s["stops"] == 0 and s["exposure"] == F(1)
    dark = np.array([[0, 0, 0], [np.nan, 1, 1], [-1, -1, -1], [np.inf, 0, 0], [1e-6, 1e-6, 1e-6]], F)
    s = tm.meter(dark, zero)
    assert (s["valid"], s["metered"], s["ignored"]) == (0, 0, 5) and not s["histogram"].any() and s["exposure"] == F(1)
    # no history and limits that exclude 0: the target 0 is cut to the nearer limit
    s = tm.meter(dark, zero, min_stops=2, max_stops=3)
    assert s["stops"] == F(2) and s["valid"] == 0
    # a valid state keeps its stops over an unmetered frame
    lit = tm.meter(np.array([[4, 4, 4]] * 9, F), zero, low=0, high=1000, compensation=0.0)
    assert lit["valid"] == 1 and lit["stops"] == F(-2.0625)
    s = tm.meter(dark, lit, rate=0.5)
    assert s["valid"] == 1 and s["stops"] == lit["stops"] == s["targetStops"] and s["exposure"] == lit["exposure"] and s["metered"] == 0


def test_the_temporal_step():
    bright, zero = np.array([[4, 4, 4]] * 9, F), tm.zero_state()
    kw = dict(low=0, high=1000, compensation=0.0)
    first = tm.meter(bright, zero, rate=0.25, **kw)                         # no history: at once, whatever the rate
    assert first["stops"] == F(-2.0625)
    dim = np.array([[1, 1, 1]] * 9, F)                                     # target -(0 + 1 / 16)
    held = tm.meter(dim, first, rate=0.0, **kw)
    assert held["stops"] == first["stops"] and held["targetStops"] == F(-0.0625)
    quarter = tm.meter(dim, held, rate=0.25, **kw)
    assert quarter["stops"] == F(-2.0625) + (F(-0.0625) - F(-2.0625)) * F(0.25) == F(-1.5625)
    there = tm.meter(dim, quarter, rate=1.0, **kw)
    assert there["stops"] == F(-0.0625)


def test_the_record_round_trips():
    s = tm.meter(tm.make_frame(500, 3), tm.zero_state())
    words = tm.record(s)
    assert words.shape == (264,) and words.dtype == np.uint32 and words[4] == 1 and words[5] + words[6] == 500 and words[8:].sum() == words[5]
    back = tm.state_of(words)
    assert np.array_equal(tm.record(back), words)


@pytest.mark.parametrize("n", [335, 771, 5184])
def test_generated_frames_cover_the_bins(n):
    frame = tm.make_frame(n, 11)
    s = tm.meter(frame, tm.zero_state())
    assert np.count_nonzero(s["histogram"]) >= 200 and s["ignored"] > 0 and s["histogram"][255] > 0
    l = tm.luminance(frame)
    with np.errstate(all="ignore"):
        fin = l[np.isfinite(l) & (l > 0)]
    assert fin.min() < 2.0 ** -19 and fin.max() > 2.0 ** 19
    assert np.isnan(frame).any() and np.isinf(frame).any() and np.signbit(frame[frame == 0]).any() and (frame < 0).any()
    assert ((np.abs(frame) < 1.1754944e-38) & (frame != 0)).any()           # denormals
    for b in tm.border_luminances():
        assert (l == b).any(), b


def test_the_curves_by_hand():
    c = np.array([[0.5, 2.0, 0.25], [np.nan, -1.0, 1e9], [-0.0, np.inf, 1.0]], F)
    x = tm.tone(c, tm.CLAMP, 2.0)
    assert np.array_equal(x, np.array([[1.0, 4.0, 0.5], [0.0, 0.0, 65536.0], [0.0, 65536.0, 2.0]], F)) and not np.signbit(x).any()
    y = tm.tone(c[:1], tm.ACES_FILM, 2.0)[0]
    for got, v in zip(y, (F(1.0), F(4.0), F(0.5))):
        assert got == (v * (F(2.51) * v + F(0.03))) / (v * (F(2.43) * v + F(0.59)) + F(0.14))
    # ACES_FITTED on grey 1: the rows of both matrices sum to 1, and the fit maps 1 to (1.0245786 - 0.000090537) / (0.983729 + 0.432951 + 0.238081) = 0.61911
    g = tm.tone(np.array([[1.0, 1.0, 1.0]], F), tm.ACES_FITTED, 1.0)[0]
    assert np.all(np.abs(g - 0.61911) < 2e-5)
    # pure red: the first column of the input matrix through the fit, then the first row of the output matrix
    z = tm.tone(np.array([[1.0, 0.0, 0.0]], F), tm.ACES_FITTED, 1.0)[0]
    vr = [F(0.59719), F(0.07600), F(0.02840)]
    w = [(v * (v + F(0.0245786)) - F(0.000090537)) / (v * (F(0.983729) * v + F(0.4329510)) + F(0.238081)) for v in vr]
    assert z[0] == (F(1.60475) * w[0] + F(-0.53108) * w[1]) + F(-0.07367) * w[2]
    # the scale: a state counts only when it is valid
    assert tm.scale_of(0.5) == F(0.5) and tm.scale_of(0.5, dict(valid=0, exposure=F(4))) == F(0.5) and tm.scale_of(0.5, dict(valid=1, exposure=F(4))) == F(2)


def test_clamp_with_exposure_one_is_the_plain_finalize(oracle):
    """the header's consequence, on 2^16 random bit patterns and the specials: the two clamps land on bytes the conversion saturates to anyway"""
    rng = np.random.default_rng(2026)
    bits = rng.integers(0, 2 ** 32, 3 * 65536, dtype=np.uint64).astype(np.uint32)
    specials = np.array([0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1.0, tm.pred(1.0), 65536.0, tm.pred(65536.0), 65537.0, 3e38, 1e-45, -1e-45, 0.0031308, 0.5, 255.0,
                         1e-40], F)
    c = np.concatenate([bits.view(F), specials, np.zeros((-len(specials)) % 3, F)]).reshape(-1, 3)
    guides = np.zeros_like(c)
    plain = oracle.finalize(c, guides, guides)[0]
    toned = tm.finalize(oracle, c, None, None, tm.CLAMP, 1.0)[0]
    assert np.array_equal(plain, toned)
    assert np.array_equal(tm.finalize(oracle, c, None, None, tm.CLAMP, 1.0, dict(valid=0, exposure=F(7)))[0], plain)        # a state without history: scale 1
