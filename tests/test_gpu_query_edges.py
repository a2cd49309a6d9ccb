"""GPU: the six ray queries (rtowProbeNearestHit[Interval], rtowTraceRaysDevice, rtowTraceViewDevice, rtowTraceRaysIntervalDevice, rtowTraceOcclusionDevice) on the
inputs of tests/query_edge_cases.py - leaves forced at MaxBvhDepth, TimeRanges other than (0, 1) with and without the common-range hoist, ray times outside the ranges,
NaN and +-inf, one-entity scenes - against the host probe (every ray, every interval family) and against the brute force of tests/trace_interval_reference.py (oracle
calls only; computed once per case and shared with the context variants).  The forced-leaf cases and the two sphere-only time-range scenes also run under
RTOW_CONTEXT_FORCE_WIDE_CODES and with an LDS scene budget of 1024 bytes.  One context of this module at a time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_edge_cases as qe  # noqa: E402
import test_gpu_trace_rays as tr  # noqa: E402
import trace_interval_reference as ir  # noqa: E402

pytestmark = pytest.mark.gpu
_u32 = tr._u32
# (ordered by context variant: the module keeps one context and replaces it when the variant changes)
RUNS = [(c, "default") for c in qe.CASES] + [(c, how) for how in ("wide", "hbm") for c in qe.DEVICE_VARIANT_CASES]


@pytest.fixture(scope="module")
def context_of(rt):
    held = {}

    def get(how):
        if held.get("how") != how:
            if "ctx" in held:
                held.pop("ctx").close()
            kw = {"default": {}, "wide": {"flags": rt.abi.CONTEXT_FORCE_WIDE_CODES}, "hbm": {"lds_scene_budget": 1024}}[how]
            held["ctx"], held["how"] = rt.Context(0, **kw), how
        return held["ctx"]

    yield get
    if "ctx" in held:
        held.pop("ctx").close()


@pytest.mark.parametrize("case,how", RUNS, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_every_query_equals_the_host_probe_and_the_brute_force(rt, oracle, context_of, case, how):
    """On every ray of the case, nothing left out:
    1. rtowTraceRaysDevice, and rtowTraceRaysIntervalDevice with NULL intervals and with every interval family: distance bits and entity of the host probe
       (rtowProbeNearestHit / rtowProbeNearestHitInterval); NULL intervals reproduce rtowTraceRaysDevice's three outputs bit for bit;
    2. rtowTraceOcclusionDevice = (entityIndex >= 0) of the nearest form;
    3. the brute force: distance bits, any-hit, the entity in the minimal set, and where that set has one member the normal bit for bit after `0 + x` on both sides
       (tests/test_gpu_trace_interval.py's rule: the sphere kinds skip the rotation by the identity quaternion through which the reference's -0 becomes +0).
    Both hits and misses under (0, +inf) in every case (asserted from the oracle alone in tests/test_query_edges_host.py, with the other input conditions)."""
    x = qe.expected(rt, oracle, case)
    rays = qe.ray_array(rt, x)
    n = len(x.pairs)
    ctx = context_of(how)
    ctx.upload_scene(x.desc)
    info = ctx.scene_info()
    if how == "wide":
        assert info.wideCodes == 1
    if how == "hbm" and case.kind == "ranges":
        assert info.sceneInLds == 0
    plain = ctx.trace_rays(rays)
    null = ctx.trace_rays_interval(rays)
    for k in ("distance", "entityIndex", "normal"):
        assert np.array_equal(np.ascontiguousarray(null[k]).view(np.uint32), np.ascontiguousarray(plain[k]).view(np.uint32)), (case, how, k)
    assert np.array_equal(ctx.trace_occlusion(rays), (plain["entityIndex"] >= 0).astype(np.uint8)), (case, how)
    dist, ent = np.zeros(n, np.float32), np.zeros(n, np.int32)
    for k, ((o, d), t) in enumerate(zip(x.pairs, x.times)):
        _, dist[k], ent[k] = ctx.hit_world(o, d, t)
    assert np.array_equal(_u32(plain["distance"]), _u32(dist)), (case, how, np.flatnonzero(_u32(plain["distance"]) != _u32(dist))[:8])
    assert np.array_equal(plain["entityIndex"], ent), (case, how, np.flatnonzero(plain["entityIndex"] != ent)[:8])
    assert np.array_equal(_u32(plain["distance"]), _u32(x.first)), (case, how, np.flatnonzero(_u32(plain["distance"]) != _u32(x.first))[:8])
    zero = np.zeros(3, np.float32)
    normals = 0
    for fam in ir.FAMILIES:
        iv = x.families[fam]
        got, occ = ctx.trace_rays_interval(rays, iv), ctx.trace_occlusion(rays, iv)
        for k, ((o, d), t) in enumerate(zip(x.pairs, x.times)):
            _, dist[k], ent[k] = ctx.hit_world_interval(o, d, t, iv[k, 0], iv[k, 1])
        assert np.array_equal(_u32(got["distance"]), _u32(dist)), (case, how, fam, np.flatnonzero(_u32(got["distance"]) != _u32(dist))[:8])
        assert np.array_equal(got["entityIndex"], ent), (case, how, fam, np.flatnonzero(got["entityIndex"] != ent)[:8])
        assert occ.dtype == np.uint8 and np.array_equal(occ, (ent >= 0).astype(np.uint8)), (case, how, fam, np.flatnonzero(occ != (ent >= 0))[:8])
        miss = ent < 0
        assert np.all(np.isposinf(got["distance"][miss])) and np.all(_u32(got["normal"][miss]) == 0), (case, how, fam)
        if fam in ir.INVALID:
            assert miss.all(), (case, how, fam)
        for k, (want_t, want_set, want_any, want_normal) in enumerate(x.want[fam]):
            assert _u32(got["distance"][k]) == _u32(want_t), (case, how, fam, k, got["distance"][k], want_t)
            assert bool(occ[k]) == want_any, (case, how, fam, k)
            e = int(got["entityIndex"][k])
            assert (e in want_set) if want_any else e == -1, (case, how, fam, k, e, sorted(want_set))
            if want_normal is not None:
                normals += 1
                assert np.array_equal(_u32(got["normal"][k] + zero), _u32(want_normal + zero)), (case, how, fam, k, got["normal"][k], want_normal)
    assert normals > 0, (case, how)


@pytest.mark.parametrize("name,time", [("fuzz1_d1", 1.2), ("ranges_mixed", 1.5), ("ranges_common", -0.5)])
def test_view_queries_equal_ray_queries_of_their_own_rays(rt, oracle, context_of, name, time):
    """rtowTraceViewDevice at 61 x 37 with a view time outside the TimeRanges, on a scene whose leaves are forced and on the time-range scenes: the three outputs equal
    rtowTraceRaysDevice's on the view's own outRays bit for bit, every ray carries the view time, and the frame has hits and misses."""
    w, h = 61, 37
    x = qe.expected(rt, oracle, qe.BY_NAME[name])
    view = tr._view_params(rt, x.scene, w, h).view
    ctx = context_of("default")
    ctx.upload_scene(x.desc)
    got = ctx.trace_view(view, w, h, time=time, want_rays=True)
    again = ctx.trace_rays(got["rays"])
    assert got["rays"].shape == (w * h,) and np.all(_u32(got["rays"]["time"]) == _u32(time))
    for k in ("distance", "entityIndex", "normal"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(again[k]).view(np.uint32)), (name, k)
    hit = got["entityIndex"] >= 0
    print("%s: %d of %d pixels hit" % (name, hit.sum(), w * h))
    assert hit.any() and (~hit).any(), name
