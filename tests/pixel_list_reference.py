"""numpy restatement of rtowBuildPixelListDevice (include/rtow.h, next to RtowPixelListParams): which pixels of a frame qualify, and the order they are listed in.

    words = build_pixel_list(width, height, capacity, color=..., mask=..., min_sample_count=..., rect=(x0, y0, x1, y1), slice_offset=..., slice_divider=...)

returns the 4 + capacity uint32 words of the list: words[0] = the number of ALL qualifiers, words[1..3] = 0, words[4 + i] = the i-th qualifier (row * W + col) for
i < min(words[0], capacity); the words behind them keep `fill` (the builder does not write them).  tests/test_pixel_list_reference.py checks this against a
double loop over the pixels; tests/test_gpu_pixel_list.py compares the device with it word for word."""
import numpy as np

TILE = 8


def qualifiers(width, height, color=None, mask=None, min_sample_count=0.0, rect=None, slice_offset=0, slice_divider=1):
    """the qualifying frame pixel indices, in list order, as uint32"""
    x0, y0, x1, y1 = rect if rect is not None else (0, 0, width, height)
    y, x = np.mgrid[0:height, 0:width]
    ok = (x >= max(x0, 0)) & (x < min(x1, width)) & (y >= max(y0, 0)) & (y < min(y1, height))
    ok &= (y % slice_divider) == slice_offset
    if mask is not None:
        ok &= np.asarray(mask, dtype=np.uint8).reshape(height, width) != 0
    if color is not None:
        count = np.asarray(color, dtype=np.float32).reshape(height, width, 4)[:, :, 3]
        with np.errstate(invalid="ignore"):
            ok &= ~(count >= np.float32(min_sample_count))               # a NaN count qualifies
    # tiles anchored at (0, 0): row of tiles by row of tiles, left to right; inside a tile row by row, left to right
    key = (((y // TILE) * ((width + TILE - 1) // TILE) + x // TILE) * (TILE * TILE) + (y % TILE) * TILE + x % TILE)
    p = (y * width + x)[ok]
    return p[np.argsort(key[ok], kind="stable")].astype(np.uint32)


def build_pixel_list(width, height, capacity, fill=0, **predicate):
    q = qualifiers(width, height, **predicate)
    words = np.full(4 + capacity, fill, dtype=np.uint32)
    words[0] = q.size
    words[1:4] = 0
    n = min(q.size, capacity)
    words[4:4 + n] = q[:n]
    return words
