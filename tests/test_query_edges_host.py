"""CPU: the product's host walk (csrc/rtow_walk.hip.h through csrc/rtow_probe.hip: probeIntervalHost nearest and any-hit, probeNearestHitHost - the text the device
kernels compile) against the brute-force reference on the inputs of tests/query_edge_cases.py: leaves forced at MaxBvhDepth, TimeRanges other than (0, 1), ray times
outside the ranges and non-finite, one-entity scenes.  Every ray gets every interval family; no ray is left out of any assertion.  The conditions that make these
inputs worth running are computed from the oracle alone and asserted here."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_edge_cases as qe  # noqa: E402
import trace_interval_reference as ir  # noqa: E402
from test_interval_walk_host import shim  # noqa: E402,F401  (the fixture that builds tests/native/interval_shim.cpp)


def _bits(x):
    return np.float32(x).view(np.uint32)


@pytest.mark.parametrize("case", qe.CASES, ids=repr)
def test_the_host_walk_equals_the_brute_force_reference(rt, oracle, shim, case):  # noqa: F811
    """tests/test_interval_walk_host.py's three assertions per ray and family (hit bit, distance bits, entity in the minimal set; the open probe equals the NULL
    family; any-hit equals the bit), on every case.  Every scene has hits and misses under (0, +inf).  The two sphere-only time-range scenes compile to
    SCENE_KIND_SPHERES_MOTION with and without the common-range hoist; forced-leaf cases really have entities whose gate box is wider than their own."""
    x = qe.expected(rt, oracle, case)                                                # (the reference's own self-check against HitWorld runs here, on every ray)
    kind = shim.shim_interval_compile(C.byref(x.desc))
    assert kind >= 0, kind
    if case.kind == "ranges":
        assert kind == 1 and shim.shim_interval_common_time_range() == (1 if case.name == "ranges_common" else 0), (case, kind)
    if case.name == "one_moving_sphere":
        assert kind == 1 and shim.shim_interval_common_time_range() == 1
    if case.kind in ("one",):
        assert x.desc.entityCount == 1
    if case.kind == "planes":
        assert (x.forced_entities > 0) == case.forced, (case, x.forced_entities)
    dist, ent = C.c_float(), C.c_int()
    hits = misses = 0
    for k, ((o, d), t) in enumerate(zip(x.pairs, x.times)):
        o3, d3 = (C.c_float * 3)(*o), (C.c_float * 3)(*d)
        for fam in ir.FAMILIES:
            tmin, tmax = x.families[fam][k]
            want_t, want_set, want_any, _ = x.want[fam][k]
            hit = shim.shim_interval_probe(o3, d3, t, tmin, tmax, 0, C.byref(dist), C.byref(ent))
            assert bool(hit) == want_any == (ent.value >= 0), (case, k, fam)
            assert _bits(dist.value) == _bits(want_t), (case, k, fam, dist.value, want_t)
            assert (ent.value in want_set) if want_any else ent.value == -1, (case, k, fam, ent.value, sorted(want_set))
            if fam == "null":
                d0, e0 = C.c_float(), C.c_int()
                shim.shim_nearest_probe(o3, d3, t, C.byref(d0), C.byref(e0))
                assert _bits(d0.value) == _bits(dist.value) and e0.value == ent.value, (case, k)
                hits += want_any
                misses += not want_any
            if fam in ir.INVALID:
                assert not hit and np.isposinf(dist.value), (case, k, fam)
            occluded = shim.shim_interval_probe(o3, d3, t, tmin, tmax, 1, C.byref(dist), C.byref(ent))
            assert bool(occluded) == want_any, (case, k, fam)
    print(case, "%d rays: %d hits, %d misses, %d entities in forced leaves" % (len(x.pairs), hits, misses, x.forced_entities))
    assert hits > 0 and misses > 0, (case, hits, misses)


def test_forced_leaves_change_the_answers_of_the_plane_rays(rt, oracle):
    """Input condition: of plane_scene's 576 rays, lying exactly in the planes of the entities' own boxes, OracleScene.hit_world answers at least 20 differently with
    max_bvh_depth 1 than with 32 (measured: 40; 73 hits at depth 32, 108 at depth 1, 5 of the 6 entities in a forced leaf)."""
    deep, flat = qe.expected(rt, oracle, qe.BY_NAME["planes_d32"]), qe.expected(rt, oracle, qe.BY_NAME["planes_d1"])
    assert len(deep.pairs) == len(flat.pairs) == 96 * deep.desc.entityCount
    assert all(d[0] == 0 or d[1] == 0 for _, d in deep.pairs) and all(np.count_nonzero(d) == 1 for _, d in deep.pairs)
    a = qe.hit_world_answers(oracle, deep.desc, deep.pairs, 0.0)
    b = qe.hit_world_answers(oracle, flat.desc, flat.pairs, 0.0)
    print("plane rays: %d hits at depth 32, %d at depth 1, %d answers differ" % ((a != 0).sum(), (b != 0).sum(), (a != b).sum()))
    assert (a != b).sum() >= 20


@pytest.mark.parametrize("name", ["ranges_common", "ranges_mixed", "ranges_general"])
def test_clamped_ray_times_change_the_answers(rt, oracle, name):
    """Input condition: in each sphere-only time-range scene at least 80 rays answer differently (OracleScene.hit_world: hit bit or distance bits) at ray time NaN, and at
    +inf, than at 0.25, the start of the range (measured: shared range 197 and 197 of 517 rays; mixed ranges 271 and 274 of 637); with mixed ranges the two counts differ
    (Unity's min / max return an operand that depends on the order when one is NaN, and a reversed range turns +inf into the other end).  The general scene has four
    movers: some rays must differ (measured: 146 and 159 of 517)."""
    x = qe.expected(rt, oracle, qe.BY_NAME[name])
    at_nan, at_inf = qe.rays_that_differ_from_the_range_start(oracle, x, qe.NAN), qe.rays_that_differ_from_the_range_start(oracle, x, qe.INF)
    print("%s: %d rays; %d differ at NaN, %d at +inf" % (name, len(x.pairs), at_nan, at_inf))
    assert min(at_nan, at_inf) >= (80 if name != "ranges_general" else 1), (name, at_nan, at_inf)
    if name == "ranges_mixed":
        assert at_nan != at_inf, (at_nan, at_inf)
    if name == "ranges_common":
        assert at_nan == at_inf


def test_the_different_range_twins_coincide_only_at_clamped_times(rt, oracle):
    """Input condition: for the twin pair with TimeRanges (0.25, 0.75) and (0.4, 0.6), the brute force's minimal set under (0, +inf) is both members at ray times 0.1 and
    0.9 and one member at 0.5 on at least 20 of the 40 ray triples aimed at it (measured: 40 of 40)."""
    x = qe.expected(rt, oracle, qe.BY_NAME["ranges_mixed"])
    sizes = qe.twin_set_sizes(x, x.scene.twins["different"])
    good = sum(s == (2, 1, 2) for s in sizes)
    print("twin triples with sets of 2, 1, 2 members: %d of %d" % (good, len(sizes)))
    assert good >= 20, sizes
