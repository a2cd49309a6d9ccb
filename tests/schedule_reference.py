"""numpy restatement of the scheduling kernels (raytracing-in-one-weekend_amd/csrc/rtow_schedule.hip.h): the launch order of the 64-pixel chunks and the ticket map.

Written from the specification, with np.sort / np.lexsort - no histogram, no prefix sum, no bitonic network:

    sums, maxima = chunk_costs(pixel_cost)              per chunk of 64 tickets, uint32
    keys = chunk_keys(sums, maxima, by_max)             float32, every operation rounded once
    buckets = chunk_buckets(keys)                       0 = most expensive .. 1023; a valid order is any permutation of the chunks with non-decreasing buckets
    cost, ticket_map = regroup(pixel_cost, ticket_map, tiles_per_row, tile_rows, side, classes)       side 2 .. 8: super-tiles; side 1: order_tiles
    cost, ticket_map = order_tiles(pixel_cost, ticket_map, levels)
    ticket_map = init_map(n)

Tiles are numbered row by row over tiles_per_row x tile_rows; tile t owns tickets 64 t .. 64 t + 63; ticket_map[t] is the pixel ticket t stands for and pixel_cost[t] the ray
count the last launch measured for that pixel.  tests/test_schedule_reference.py pins this file on hand-worked cases and against loops over tiles and tickets;
tests/test_gpu_schedule.py compares the device with it word for word."""
import functools

import numpy as np

CHUNK = 64
BUCKETS = 1024
MAX_SIDE = 8


def chunk_costs(pixel_cost):
    c = np.asarray(pixel_cost, dtype=np.uint16).reshape(-1, CHUNK).astype(np.uint32)
    return c.sum(axis=1, dtype=np.uint32), c.max(axis=1)


def chunk_keys(sums, maxima, by_max):
    s, m = np.asarray(sums, dtype=np.uint32).astype(np.float32), np.asarray(maxima, dtype=np.uint32).astype(np.float32)
    if by_max:
        return m * np.float32(64) + s * np.float32(1.0 / 64.0)          # the most expensive pixel first, ties by the total
    return s


def chunk_buckets(keys):
    """bucket of every chunk: 1023 - trunc(key * (1023 / M)), M = max(1, the largest key), all in float32.  (For some M, M * (1023 / M) rounds to just below 1023:
    the most expensive chunk then sits in bucket 1 and bucket 0 is empty - specified behaviour.)"""
    keys = np.asarray(keys, dtype=np.float32)
    m = max(np.float32(1.0), keys.max()) if keys.size else np.float32(1.0)
    scale = np.float32(BUCKETS - 1) / np.float32(m)
    assert scale.dtype == np.float32
    return (BUCKETS - 1) - np.trunc(keys * scale).astype(np.int64)


def init_map(n):
    return np.arange(n, dtype=np.uint32)


def _primary(cost, classes):
    cost = cost.astype(np.int64)
    t1, t2, t3 = (int(c) for c in classes)
    if t1 == 0:
        return np.minimum(cost + 1, 65535)                               # the ray count itself; 65 534 and 65 535 share the saturated key
    return 1 + (cost > t1) + (cost > t2) + (cost > t3)


@functools.lru_cache(maxsize=8)
def _super_tiles(tiles_per_row, tile_rows, side):
    """(the super-tile of every ticket, the tickets of every super-tile in the order they are written back over) - the geometry alone, kept between calls"""
    t = np.arange(tiles_per_row * tile_rows * CHUNK)
    tile, lane = t // CHUNK, t % CHUNK
    ty, tx = tile // tiles_per_row, tile % tiles_per_row
    sy, sx = ty // side, tx // side
    group = sy * ((tiles_per_row + side - 1) // side) + sx               # which super-tile
    width = np.minimum(side, tiles_per_row - sx * side)                  # partial at the right edge (and, with fewer rows, at the bottom)
    place = ((ty - sy * side) * width + (tx - sx * side)) * CHUNK + lane  # tile by tile inside the super-tile (tiles row-major), 64 per tile
    # (np.lexsort over the columns says the same and takes five times as long: they are packed into one 64-bit sort key - here super-tile | place)
    assert group.max() < (1 << 16) and place.max() < (1 << 32)
    group = group.astype(np.uint64)
    return group, np.argsort((group << np.uint64(32)) | place.astype(np.uint64), kind="stable")


def regroup(pixel_cost, ticket_map, tiles_per_row, tile_rows, side, classes):
    """one regrouping; returns (pixel_cost', ticket_map') as uint16 / uint32"""
    cost, pixel = np.asarray(pixel_cost, dtype=np.uint16), np.asarray(ticket_map, dtype=np.uint32)
    assert cost.size == pixel.size == tiles_per_row * tile_rows * CHUNK
    if side == 1:
        return order_tiles(cost, pixel, classes[0])
    assert 2 <= side <= MAX_SIDE
    group, slots = _super_tiles(tiles_per_row, tile_rows, side)
    falling = (65535 - _primary(cost, classes)).astype(np.uint64)        # primary descending, then pixel number ascending: super-tile | 65 535 - primary | pixel, 16 + 16 + 32 bits
    ranked = np.argsort((group << np.uint64(48)) | (falling << np.uint64(32)) | pixel.astype(np.uint64), kind="stable")
    out_cost, out_map = np.empty_like(cost), np.empty_like(pixel)
    out_cost[slots], out_map[slots] = cost[ranked], pixel[ranked]
    return out_cost, out_map


def order_tiles(pixel_cost, ticket_map, levels):
    """side 1: every tile's 64 tickets by primary descending, equal primaries in the order of their places (stable); the pairs move together"""
    cost, pixel = np.asarray(pixel_cost, dtype=np.uint16).reshape(-1, CHUNK), np.asarray(ticket_map, dtype=np.uint32).reshape(-1, CHUNK)
    c = cost.astype(np.int64)
    top = c.max(axis=1, keepdims=True)
    primary = c if int(levels) == 0 else (c * int(levels)) // (top + 1)
    idx = np.argsort(-primary, axis=1, kind="stable")
    return np.take_along_axis(cost, idx, axis=1).reshape(-1), np.take_along_axis(pixel, idx, axis=1).reshape(-1)
