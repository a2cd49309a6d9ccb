"""CPU: the numpy restatement of rtowBloomDevice (tests/bloom_reference.py) held to three properties that follow from the specification in include/rtow.h alone: a
constant frame blooms to a closed form exactly, a firefly is damped by the Karis average and a frame below the threshold is left alone, and no input and no exposure
scale makes the bloom layer non-finite."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bloom_reference as bl  # noqa: E402

F = np.float32


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 5)])
@pytest.mark.parametrize("levels", [1, 3, 8])
def test_a_constant_frame_blooms_to_the_closed_form_exactly(w, h, levels):
    """Threshold and knee 0: le - 0 = le, g = le / le = 1, b = 1.  Every tap weight and every partial sum is dyadic, so every mip is exactly 1, U_k = 1 + 0.5 U_k+1
    and out = 1 + 0.25 * sum of 0.5^m for m < levels, with no rounding anywhere."""
    got = bl.bloom(np.ones((w * h, 3), F), w, h, levels, threshold=0.0, knee=0.0, scatter=0.5, intensity=0.25, s=1.0, karis=False)
    want = F(1 + 0.25 * sum(0.5 ** m for m in range(levels)))
    assert want == 1 + 0.25 * sum(0.5 ** m for m in range(levels)), "the closed form is a float32"
    assert np.array_equal(got["out"], np.full((w * h, 3), want, F))
    assert [m.shape[:2] for m in got["mips"]] == [(hh, ww) for ww, hh in bl.mip_sizes(w, h, levels)]


def test_a_firefly_is_damped_and_a_frame_below_the_threshold_is_left_alone():
    """A frame of 0.5 under threshold 1 with knee 0.25 - the bright pass starts to fade in at 0.75, clear of the frame's luminance whatever the rounding of the three
    luminance terms - has a bloom layer of exactly zero and comes out as it went in.  One pixel at 10^4 blooms; the Karis weight of that pixel is about 10^-4, so the
    peak of the layer with the flag is far below the peak without it."""
    w, h = 48, 32
    frame = np.full((h * w, 3), 0.5, F)
    kw = dict(levels=5, threshold=1.0, knee=0.25, scatter=0.7, intensity=1.0, s=1.0)
    for karis in (False, True):
        calm = bl.bloom(frame, w, h, karis=karis, **kw)
        assert not calm["layer"].any() and np.array_equal(calm["out"].view(np.uint32), frame.view(np.uint32))
    lit = frame.copy()
    lit[13 * w + 21] = 1e4
    plain, karis = bl.bloom(lit, w, h, karis=False, **kw), bl.bloom(lit, w, h, karis=True, **kw)
    print("peak of the layer: plain %g, karis %g" % (plain["layer"].max(), karis["layer"].max()))
    assert plain["layer"].max() > 100.0                                    # 9/64 of (10^4 - 1) lands in one texel of mip 1
    assert 0.0 < karis["layer"].max() < plain["layer"].max() / 100.0


HOSTILE = [np.nan, np.inf, -np.inf, -1.0, -3e38, 0.0, -0.0, 1e-40, 3e38, 65536.0]


@pytest.mark.parametrize("s", [0.0, 1.0, 2.0 ** 32, 3e38])
def test_hostile_inputs_leave_the_layer_finite_and_pass_through(s):
    w, h = 37, 11
    rng = np.random.default_rng(5)
    frame = np.array(HOSTILE, F)[rng.integers(0, len(HOSTILE), (h * w, 3))]
    frame[::7] = np.array(HOSTILE, F)[rng.integers(5, len(HOSTILE), (len(frame[::7]), 3))]      # some pixels finite in every channel
    broken = ~np.isfinite(frame).all(axis=1)
    assert broken.any() and (~broken).any()
    for karis in (False, True):
        for threshold, knee in ((0.0, 0.0), (1.0, 0.0), (1.0, 0.5), (1.0, 1.0)):
            got = bl.bloom(frame, w, h, 8, threshold, knee, 1.0, 0.5, s=s, karis=karis)
            assert np.isfinite(got["layer"]).all(), (s, karis, threshold, knee)
            assert all(np.isfinite(m).all() for m in got["mips"])
            assert np.array_equal(got["out"][broken].view(np.uint32), frame[broken].view(np.uint32)), "a pixel with a non-finite channel is copied through"
