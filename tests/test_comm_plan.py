"""CPU: the staging layout of the multi-GPU row transport (csrc/rtow_comm_plan.h) held to its contract without a GPU.

rtowGatherRowsDevice and rtowExchangeAccumDevice move the rows a rank owns (row % world == rank) as packed regions of two staging blocks per context.  Where every
region begins and how large a block must be is pure arithmetic; the library's own functions are compared here, integer for integer, with a restatement that counts a
rank's rows as `len(range(rank, height, world))`: for every world size 1..9, frame heights that include fewer rows than ranks, every selection of accumulators, every
root, and for the exchange every tile count that divides the world.  No region may overlap another, and a block ends where its last region ends."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPONENTS = (4, 3, 3, 1)       # floats per pixel of colour, normal, albedo, sample-count weight: bits 0..3 of `what`
WORLDS = range(1, 10)
HEIGHTS = (1, 2, 7, 36, 54, 1080)
WIDTHS = (1, 5, 64)


@pytest.fixture(scope="module")
def shim():
    csrc = os.path.join(ROOT, "raytracing-in-one-weekend_amd", "csrc")
    out_dir = os.path.join(ROOT, "tests", "build")
    os.makedirs(out_dir, exist_ok=True)
    src, so = os.path.join(ROOT, "tests", "native", "comm_plan_shim.cpp"), os.path.join(out_dir, "libcomm_plan_shim.so")
    deps = [src, os.path.join(csrc, "rtow_comm_plan.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-fPIC", "-shared", "-x", "c++", src, "-o", so], check=True, capture_output=True)
    lib = C.CDLL(so)
    lib.shim_packed_floats.restype = C.c_uint64
    return lib


def rows_of(rank, height, world):
    return len(range(rank, height, world))


def floats_per_pixel(what):
    return sum(c for b, c in enumerate(COMPONENTS) if what >> b & 1)


def laid_end_to_end(sizes):
    """offsets of regions of these sizes one after the other, and the end of the last"""
    offsets, at = [], 0
    for n in sizes:
        offsets.append(at)
        at += n
    return offsets, at


def assert_disjoint_and_closed(offsets, sizes, total):
    spans = sorted((o, o + n) for o, n in zip(offsets, sizes) if n)
    for (_, end), (begin, _) in zip(spans, spans[1:]):
        assert end <= begin, (offsets, sizes)
    assert total == (spans[-1][1] if spans else 0), (offsets, sizes, total)


def test_rows_owned_and_packed_size(shim):
    for world in WORLDS:
        for height in HEIGHTS:
            owned = [int(shim.shim_rows_owned_by(r, world, height)) for r in range(world)]
            assert owned == [rows_of(r, height, world) for r in range(world)]
            assert sum(owned) == height, "every row has exactly one owner"
            for what in range(1, 16):
                assert int(shim.shim_floats_per_pixel(what)) == floats_per_pixel(what)
                for width in WIDTHS:
                    for r in range(world):
                        assert int(shim.shim_packed_floats(width, height, world, what, r)) == owned[r] * width * floats_per_pixel(what)


def test_gather_root_receive_block(shim):
    offsets, total = (C.c_uint64 * 16)(), C.c_uint64()
    for world in WORLDS:
        for height in HEIGHTS:
            for what in range(1, 16):
                for width in WIDTHS:
                    for root in range(world):
                        assert shim.shim_gather_regions(width, height, world, what, root, offsets, C.byref(total)) == world
                        # one region per rank in rank order; the root's own rows do not travel
                        sizes = [0 if r == root else rows_of(r, height, world) * width * floats_per_pixel(what) for r in range(world)]
                        want, end = laid_end_to_end(sizes)
                        got = [int(offsets[r]) for r in range(world)]
                        assert got == want, (world, height, what, width, root)
                        assert int(total.value) == end == sum(sizes)
                        assert_disjoint_and_closed(got, sizes, int(total.value))


def test_exchange_send_and_receive_blocks(shim):
    send, recv, send_total, recv_total = (C.c_uint64 * 16)(), (C.c_uint64 * 16)(), C.c_uint64(), C.c_uint64()
    for world in WORLDS:
        for tiles in [t for t in range(1, world + 1) if world % t == 0]:
            groups = world // tiles
            for height in HEIGHTS:
                for what in range(1, 16):
                    for width in WIDTHS:
                        for rank in range(world):
                            assert shim.shim_exchange_regions(width, height, world, what, rank, tiles, send, C.byref(send_total), recv, C.byref(recv_total)) == groups
                            tile, own = rank % tiles, rank // tiles
                            fpp = floats_per_pixel(what)
                            # send block: what the peer of every other group owns (the rows with row % world == peer), in group order
                            sizes = [0 if g == own else rows_of(tile + tiles * g, height, world) * width * fpp for g in range(groups)]
                            want, end = laid_end_to_end(sizes)
                            got = [int(send[g]) for g in range(groups)]
                            assert got == want, (world, tiles, height, what, width, rank)
                            assert int(send_total.value) == end
                            assert_disjoint_and_closed(got, sizes, end)
                            # receive block: one region of this rank's own rows per group, region g at g x the region size (its own group's region stays unused)
                            region = rows_of(rank, height, world) * width * fpp
                            assert [int(recv[g]) for g in range(groups)] == [g * region for g in range(groups)]
                            assert int(recv_total.value) == groups * region
                            assert_disjoint_and_closed([int(recv[g]) for g in range(groups)], [region] * groups, int(recv_total.value))
