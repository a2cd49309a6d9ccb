"""CPU: tests/schedule_reference.py (the numpy restatement of the chunk-order and ticket-map kernels that tests/test_gpu_schedule.py compares the device with) on
hand-worked cases of a few elements each, and against plain loops over super-tiles, tiles and tickets that read the specification line by line."""
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schedule_reference as ref  # noqa: E402


def chunk(*head):
    """one chunk's 64 ray counts: `head`, then zeros"""
    return list(head) + [0] * (64 - len(head))


# ---- chunk cost, key, bucket ----

def test_chunk_costs_are_unsigned_sums_and_maxima():
    cost = np.array(chunk(3, 5, 1) + [65535] * 64 + chunk(), np.uint16)
    sums, maxima = ref.chunk_costs(cost)
    assert sums.dtype == np.uint32 and maxima.dtype == np.uint32
    assert sums.tolist() == [9, 64 * 65535, 0] and maxima.tolist() == [5, 65535, 0]          # 4 194 240: no 16-bit wrap


def test_keys_by_total_and_by_the_most_expensive_pixel():
    sums, maxima = np.array([9, 128, 0], np.uint32), np.array([5, 2, 0], np.uint32)
    assert ref.chunk_keys(sums, maxima, 0).tolist() == [9.0, 128.0, 0.0]
    k = ref.chunk_keys(sums, maxima, 1)
    assert k.dtype == np.float32 and k.tolist() == [5 * 64 + 9 / 64, 2 * 64 + 2.0, 0.0]      # 320.140625, 130: exact in float32


def test_key_by_max_is_rounded_to_float32_once_per_operation():
    """max = 65 535, sum = 4 194 239: 4 194 240 + 65 534.984375 = 4 259 774.984375 needs 29 bits; float32 keeps a step of 0.5 there, ties to even -> 4 259 775.0"""
    k = ref.chunk_keys(np.array([4194239], np.uint32), np.array([65535], np.uint32), 1)
    assert k.dtype == np.float32 and float(k[0]) == 4259775.0
    # and a sum whose 1/64 part cannot be kept: max = 65 535, sum = 65 535 + 63 -> 4 194 240 + 1 024.96875 = 4 195 264.96875 -> 4 195 265.0
    assert float(ref.chunk_keys(np.array([65598], np.uint32), np.array([65535], np.uint32), 1)[0]) == 4195265.0


def test_buckets_hand_worked():
    # M = 1023: scale = 1, bucket = 1023 - key
    assert ref.chunk_buckets(np.array([1023, 512, 0, 1, 1022.5], np.float32)).tolist() == [0, 511, 1023, 1022, 1]
    # all zero: M stays 1, everything in the last bucket
    assert ref.chunk_buckets(np.zeros(5, np.float32)).tolist() == [1023] * 5
    # keys below 1: M stays 1, scale = 1023
    assert ref.chunk_buckets(np.array([0.5, 0.25], np.float32)).tolist() == [1023 - 511, 1023 - 255]
    # M = 2046: scale = 0.5; trunc, not round
    assert ref.chunk_buckets(np.array([2046, 3, 2, 1], np.float32)).tolist() == [0, 1022, 1022, 1023]


def test_the_largest_key_can_land_in_bucket_one():
    """for some M, float32(M * float32(1023 / M)) is just below 1023: bucket 0 stays empty.  Restated, not corrected - and no key ever leaves 0 .. 1023."""
    m = np.arange(1, 1 << 16, dtype=np.float32)
    scale = np.float32(1023) / m
    top = 1023 - np.trunc(m * scale).astype(np.int64)
    assert set(top.tolist()) == {0, 1}
    first = int(m[top == 1][0])
    b = ref.chunk_buckets(np.array([first, 0], np.float32))
    assert b.tolist() == [1, 1023]
    # the same through float arithmetic done by hand on the bit patterns' values
    s = struct.unpack("f", struct.pack("f", 1023.0 / first))[0]
    assert struct.unpack("f", struct.pack("f", first * s))[0] < 1023.0
    rng = np.random.default_rng(5)
    for _ in range(200):
        keys = rng.integers(0, rng.integers(1, 1 << 23), 300).astype(np.float32)
        bk = ref.chunk_buckets(keys)
        assert bk.min() >= 0 and bk.max() <= 1023
        assert (np.diff(bk[np.argsort(-keys, kind="stable")]) >= 0).all()                  # a larger key never sits in a later bucket


# ---- ticket map ----

def test_init_map_is_the_identity():
    m = ref.init_map(5)
    assert m.dtype == np.uint32 and m.tolist() == [0, 1, 2, 3, 4]
    assert ref.init_map(0).size == 0


def test_regroup_one_tile_by_cost_hand_worked():
    """one tile, side 2 (a partial super-tile of 1 x 1): costs 0 0 7 7 2 65535 65534 0 ... ; pixels 100 + place"""
    cost = np.array(chunk(0, 0, 7, 7, 2, 65535, 65534), np.uint16)
    pixel = (100 + np.arange(64)).astype(np.uint32)
    c, m = ref.regroup(cost, pixel, 1, 1, 2, (0, 0, 0))
    # 65 535 and 65 534 share the saturated primary: pixel order decides (105 before 106); then the 7s (102, 103), the 2, the zeros in pixel order
    assert m[:7].tolist() == [105, 106, 102, 103, 104, 100, 101] and m[7:].tolist() == list(range(107, 164))
    assert c[:7].tolist() == [65535, 65534, 7, 7, 2, 0, 0] and not c[7:].any()
    assert c.dtype == np.uint16 and m.dtype == np.uint32


def test_regroup_ties_follow_the_pixel_number_not_the_place():
    cost = np.array(chunk(4, 4, 4, 9), np.uint16)
    pixel = np.arange(64, dtype=np.uint32)[::-1].copy() + 1000                                 # descending pixel numbers
    c, m = ref.regroup(cost, pixel, 1, 1, 4, (0, 0, 0))
    assert m[0] == 1060 and c[0] == 9                                                          # the 9
    assert m[1:4].tolist() == [1061, 1062, 1063] and c[1:4].tolist() == [4, 4, 4]              # the 4s, pixel ascending: places 2, 1, 0
    assert m[4:].tolist() == list(range(1000, 1060)) and not c[4:].any()


def test_regroup_classes_hand_worked():
    """classes {8, 22, 32}: <= 8 | 9 .. 22 | 23 .. 32 | beyond; inside a class the pixel order, whatever the cost"""
    cost = np.array(chunk(8, 9, 22, 23, 32, 33, 40, 0), np.uint16)
    pixel = np.arange(64, dtype=np.uint32)
    c, m = ref.regroup(cost, pixel, 1, 1, 2, (8, 22, 32))
    assert m[:6].tolist() == [5, 6, 3, 4, 1, 2] and c[:6].tolist() == [33, 40, 23, 32, 9, 22]
    assert m[6:].tolist() == [0] + list(range(7, 64)) and c[6] == 8 and not c[7:].any()
    # {8, none, none}: two classes
    c, m = ref.regroup(cost, pixel, 1, 1, 2, (8, 0xffffffff, 0xffffffff))
    assert m[:6].tolist() == [1, 2, 3, 4, 5, 6] and m[6:].tolist() == [0] + list(range(7, 64))
    assert c[:7].tolist() == [9, 22, 23, 32, 33, 40, 8]


def test_regroup_partial_super_tile_enumeration():
    """3 x 1 tiles, side 2: super-tile 0 = tiles 0, 1; super-tile 1 = tile 2 alone.  The most expensive pixel of tile 1 moves to ticket 0, nothing crosses into tile 2."""
    cost = np.zeros(192, np.uint16)
    cost[64 + 10] = 5                       # tile 1
    cost[128 + 63] = 9                      # tile 2
    pixel = np.arange(192, dtype=np.uint32)
    c, m = ref.regroup(cost, pixel, 3, 1, 2, (0, 0, 0))
    assert m[0] == 74 and c[0] == 5 and m[1:75].tolist() == list(range(0, 74)) and m[75:128].tolist() == list(range(75, 128))
    assert m[128] == 191 and c[128] == 9 and m[129:].tolist() == list(range(128, 191))
    # 1 x 3 tiles, side 2: tiles 0 and 1 (rows 0, 1) together, tile 2 alone
    c, m = ref.regroup(cost, pixel, 1, 3, 2, (0, 0, 0))
    assert m[0] == 74 and m[128] == 191


def test_regroup_two_by_two_enumeration_is_tile_by_tile():
    """3 x 2 tiles, side 2: super-tile 0 = tiles 0, 1, 3, 4 in that order; super-tile 1 = tiles 2, 5"""
    n = 6 * 64
    cost = np.zeros(n, np.uint16)
    pixel = np.arange(n, dtype=np.uint32)
    cost[3 * 64:4 * 64] = 1                  # all of tile 3 costs 1: it must come out as the FIRST tile of its super-tile
    cost[5 * 64 + 1] = 2
    c, m = ref.regroup(cost, pixel, 3, 2, 2, (0, 0, 0))
    assert m[0:64].tolist() == list(range(192, 256)) and (c[0:64] == 1).all()
    assert m[64:128].tolist() == list(range(0, 64)) and m[192:256].tolist() == list(range(64, 128)) and m[256:320].tolist() == list(range(256, 320))
    assert m[128] == 321 and c[128] == 2 and m[129:192].tolist() == list(range(128, 191))
    assert m[320:].tolist() == [191, 320] + list(range(322, 384))


def loop_regroup(cost, pixel, tiles_per_row, tile_rows, side, classes):
    cost, pixel = [int(v) for v in cost], [int(v) for v in pixel]
    out_cost, out_map = list(cost), list(pixel)
    for sy in range(0, tile_rows, side):
        for sx in range(0, tiles_per_row, side):
            tickets = []
            for ty in range(sy, min(sy + side, tile_rows)):
                for tx in range(sx, min(sx + side, tiles_per_row)):
                    tickets += [(ty * tiles_per_row + tx) * 64 + lane for lane in range(64)]
            def primary(c):
                if classes[0] == 0:
                    return min(c + 1, 65535)
                return 1 + (c > classes[0]) + (c > classes[1]) + (c > classes[2])
            pairs = sorted(((pixel[t], cost[t]) for t in tickets), key=lambda pc: (-primary(pc[1]), pc[0]))
            for t, (p, c) in zip(tickets, pairs):
                out_map[t], out_cost[t] = p, c
    return out_cost, out_map


@pytest.mark.parametrize("side", [2, 3, 4, 5, 8])
@pytest.mark.parametrize("grid", [(1, 1), (2, 1), (3, 3), (5, 7), (9, 4)])
def test_regroup_equals_the_loops(side, grid):
    tiles_per_row, tile_rows = grid
    n = tiles_per_row * tile_rows * 64
    rng = np.random.default_rng(side * 100 + tiles_per_row)
    pixel = (rng.permutation(1 << 20)[:n] + (1 << 26)).astype(np.uint32)
    for classes in ((0, 0, 0), (8, 0xffffffff, 0xffffffff), (8, 22, 32)):
        for cost in (rng.integers(0, 40, n), rng.choice([0, 8, 65534, 65535], n), np.zeros(n)):
            cost = cost.astype(np.uint16)
            want_cost, want_map = loop_regroup(cost, pixel, tiles_per_row, tile_rows, side, classes)
            got_cost, got_map = ref.regroup(cost, pixel, tiles_per_row, tile_rows, side, classes)
            assert got_map.tolist() == want_map and got_cost.tolist() == want_cost, (classes,)
            assert sorted(got_map.tolist()) == sorted(pixel.tolist())


def test_order_tiles_hand_worked():
    """levels 0: by the ray count, stable.  levels 4 with top = 99: level = cost * 4 // 100 -> 0 .. 24 | 25 .. 49 | 50 .. 74 | 75 .. 99"""
    cost = np.array(chunk(1, 99, 50, 74, 75, 24, 25), np.uint16)
    pixel = (500 - np.arange(64)).astype(np.uint32)                                             # pixel numbers play no part here
    c, m = ref.order_tiles(cost, pixel, 0)
    assert c[:7].tolist() == [99, 75, 74, 50, 25, 24, 1] and m[:7].tolist() == [499, 496, 497, 498, 494, 495, 500]
    assert m[7:].tolist() == list(range(493, 436, -1))                                           # the zeros keep their places' order
    c, m = ref.order_tiles(cost, pixel, 4)
    # level 3: 99, 75 (places 1, 4); level 2: 50, 74 (places 2, 3 - place order, not cost order); level 1: 25; level 0: 1, 24, zeros by place
    assert c[:7].tolist() == [99, 75, 50, 74, 25, 1, 24] and m[:7].tolist() == [499, 496, 498, 497, 494, 500, 495]
    assert ref.regroup(cost, pixel, 1, 1, 1, (4, 0, 0))[1].tolist() == m.tolist()                # side 1 of regroup is this function, classes[0] = levels


def test_order_tiles_saturated_cost_and_lane_63():
    cost = np.zeros(128, np.uint16)
    cost[63] = 65535                          # tile 0: the expensive pixel in the last place
    cost[64:] = 7                             # tile 1: all equal - unchanged under every level count
    pixel = np.arange(128, dtype=np.uint32)
    for levels in (0, 4, 8, 16):
        c, m = ref.order_tiles(cost, pixel, levels)
        assert m[:64].tolist() == [63] + list(range(63)) and c[0] == 65535 and not c[1:64].any()
        assert m[64:].tolist() == list(range(64, 128)) and (c[64:] == 7).all()


@pytest.mark.parametrize("levels", [0, 4, 8, 16])
def test_order_tiles_equals_the_loop(levels):
    rng = np.random.default_rng(levels)
    tiles = 5
    cost = rng.choice(np.array([0, 1, 2, 3, 100, 1000, 65534, 65535]), tiles * 64).astype(np.uint16)
    pixel = rng.permutation(tiles * 64).astype(np.uint32)
    got_cost, got_map = ref.order_tiles(cost, pixel, levels)
    for tile in range(tiles):
        c = [int(v) for v in cost[tile * 64:tile * 64 + 64]]
        top = max(c)
        prim = [v if levels == 0 else (v * levels) // (top + 1) for v in c]
        places = sorted(range(64), key=lambda i: -prim[i])                                      # sorted() is stable
        assert got_cost[tile * 64:tile * 64 + 64].tolist() == [c[i] for i in places]
        assert got_map[tile * 64:tile * 64 + 64].tolist() == [int(pixel[tile * 64 + i]) for i in places]
