"""CPU: tests/pixel_list_reference.py (the numpy restatement of rtowBuildPixelListDevice the GPU tests compare the device with) against a brute-force double loop
over tiles and pixels that reads the specification of include/rtow.h line by line."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pixel_list_reference as ref  # noqa: E402

SIZES = [(1, 1), (7, 5), (8, 8), (70, 37), (129, 65)]


def brute_force(width, height, color, mask, min_sample_count, rect, slice_offset, slice_divider):
    x0, y0, x1, y1 = rect
    out = []
    for ty in range((height + 7) // 8):
        for tx in range((width + 7) // 8):
            for j in range(8):
                for i in range(8):
                    x, y = tx * 8 + i, ty * 8 + j
                    if x >= width or y >= height:
                        continue
                    if not (max(x0, 0) <= x < min(x1, width) and max(y0, 0) <= y < min(y1, height)):
                        continue
                    if y % slice_divider != slice_offset:
                        continue
                    p = y * width + x
                    if mask is not None and mask[p] == 0:
                        continue
                    if color is not None:
                        c = float(color[4 * p + 3])
                        if not math.isnan(c) and c >= min_sample_count:
                            continue
                    out.append(p)
    return out


def frame_inputs(width, height, seed):
    """a mask with holes, and counts that include NaN, -0, +0, values around the bound and infinities"""
    rng = np.random.default_rng(seed)
    n = width * height
    mask = (rng.random(n) < 0.7).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    color = rng.random((n, 4)).astype(np.float32)
    color[:, 3] = rng.choice(np.array([np.nan, -0.0, 0.0, 0.5, 1.0, 2.0, 3.0, 64.0, np.inf, -np.inf, -1.0], dtype=np.float32), n)
    return mask, color.reshape(-1)


def rectangles(width, height):
    return [(0, 0, width, height),                               # full
            (-5, -3, width + 9, height + 2),                     # sticks out on every side
            (3, 2, 3, height), (width, 0, width + 4, height), (5, 4, 2, 1),      # empty
            (width // 3, height // 4, width - 1, height - 1),    # inside, off the tile grid
            (-2, height // 2, width // 2 + 1, height + 7)]       # sticks out of two sides


@pytest.mark.parametrize("width,height", SIZES)
def test_restatement_equals_the_double_loop(width, height):
    mask, color = frame_inputs(width, height, 1000 * width + height)
    cases = 0
    for rect in rectangles(width, height):
        for divider, offset in ((1, 0), (2, 0), (2, 1), (3, 0), (3, 2)):
            for use_mask, use_color, bound in ((False, False, 0.0), (True, False, 0.0), (False, True, 1.0), (True, True, 2.0), (False, True, 0.0)):
                m, c = mask if use_mask else None, color if use_color else None
                want = brute_force(width, height, c, m, bound, rect, offset, divider)
                got = ref.qualifiers(width, height, color=c, mask=m, min_sample_count=bound, rect=rect, slice_offset=offset, slice_divider=divider)
                assert got.dtype == np.uint32 and got.tolist() == want, (rect, divider, offset, use_mask, use_color, bound)
                assert len(set(want)) == len(want)
                cases += 1
    assert cases == 7 * 5 * 5


def test_nan_and_negative_zero_counts():
    """a NaN count qualifies under every bound; -0 is 0: it qualifies under a bound of 1 and not under a bound of 0 (nothing is below 0 but NaN)"""
    color = np.zeros((4, 4), np.float32)
    color[:, 3] = np.array([np.nan, -0.0, 0.0, 1.0], np.float32)
    assert ref.qualifiers(4, 1, color=color.reshape(-1), min_sample_count=1.0).tolist() == [0, 1, 2]
    assert ref.qualifiers(4, 1, color=color.reshape(-1), min_sample_count=0.0).tolist() == [0]
    assert ref.qualifiers(4, 1, color=color.reshape(-1), min_sample_count=np.inf).tolist() == [0, 1, 2, 3]


def test_tile_order_of_a_ragged_frame():
    """10 x 9: two tiles per row of tiles, the right one two pixels wide, the upper row of tiles one pixel high"""
    got = ref.qualifiers(10, 9).tolist()
    first = [y * 10 + x for y in range(8) for x in range(8)]
    second = [y * 10 + x for y in range(8) for x in (8, 9)]
    assert got == first + second + [80 + x for x in range(8)] + [88, 89]


@pytest.mark.parametrize("width,height", SIZES)
def test_capacity_and_overflow(width, height):
    mask, color = frame_inputs(width, height, 7)
    q = ref.qualifiers(width, height, color=color, mask=mask, min_sample_count=2.0)
    total = q.size
    assert (width, height) == (1, 1) or total > 1
    for capacity in sorted({0, max(total - 1, 0), total, total + 1}):
        words = ref.build_pixel_list(width, height, capacity, fill=0xDEADBEEF, color=color, mask=mask, min_sample_count=2.0)
        assert words.dtype == np.uint32 and words.size == 4 + capacity
        assert words[0] == total and not words[1:4].any()                 # the total, whatever the capacity
        n = min(total, capacity)
        assert np.array_equal(words[4:4 + n], q[:n])                      # the FIRST capacity qualifiers
        assert (words[4 + n:] == 0xDEADBEEF).all()                        # nothing behind them
