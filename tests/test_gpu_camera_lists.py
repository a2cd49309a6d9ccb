"""GPU: pruned camera-ray lists (csrc/rtow_camera_lists.hip.h, primary_candidates_kernel) against the CPU oracle and against whole lists, bit for bit.

By default a sphere scene's lists leave out every node none of whose spheres a camera ray of the pixel can hit or see.  The frame must not change by a bit: each scene of
tests/camera_lists_support.py runs plain, as a chain of 3 and as a group of 3 (32 x 18, the cover scene 64 x 36; 4 samples, seeds 1 .. 3, depth 8) in a default context,
in one with RTOW_CONTEXT_UNPRUNED_CAMERA_RAY_LISTS and in one with RTOW_CONTEXT_NO_CAMERA_RAY_LISTS; all three must give the oracle's accumulators and RayCount.
rtowGetCameraRayListStats shows that the default context pruned, what it pruned where the scene was picked for it, and that the long lists (5 to 8 nodes, and the fall
back to the walk beyond 8) are still driven; tests/test_camera_lists.py holds the same scenes to the oracle ray by ray on the CPU.
"""
import numpy as np
import pytest

import camera_lists_support as S

KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))
SCENES = ("cover", "stack", "cluster", "inside_glass", "tangent", "horizon", "lens", "moving", "one")


def _size(name):
    return (64, 36) if name == "cover" else (S.W, S.H)


def _plist(name, sc, stride=4):
    w, h = _size(name)
    return [S.params(sc, seed=seed, jitter=name != "tangent", w=w, h=h, stride=stride, name=name) for seed in (1, 2, 3)]


@pytest.fixture(scope="module")
def references(oracle):
    """scene name -> (scene, desc, the three batches' parameters, each batch alone, the three in a chain): computed once"""
    out = {}
    for name in SCENES:
        sc = S.scene(name)
        desc = sc.desc()
        plist = _plist(name, sc)
        osc = oracle.OracleScene(desc)
        try:
            alone = [osc.sample_batch(p) for p in plist]
            chain = alone[0]
            for p in plist[1:]:
                chain = osc.sample_batch(p, {k: chain[k] for k, _ in KEYS})
        finally:
            osc.close()
        out[name] = (sc, desc, plist, alone, chain)
    return out


@pytest.fixture(scope="module")
def contexts(rt):
    a = rt.abi
    made = {"pruned": rt.Context(0), "unpruned": rt.Context(0, flags=a.CONTEXT_UNPRUNED_CAMERA_RAY_LISTS), "walk": rt.Context(0, flags=a.CONTEXT_NO_CAMERA_RAY_LISTS),
            "ties pruned": rt.Context(0, flags=a.CONTEXT_EXACT_TIES_ALWAYS), "ties unpruned": rt.Context(0, flags=a.CONTEXT_EXACT_TIES_ALWAYS | a.CONTEXT_UNPRUNED_CAMERA_RAY_LISTS)}
    yield made
    for ctx in made.values():
        ctx.close()


def _same(got, ref, what):
    for k, _ in KEYS:
        assert np.array_equal(got[k].reshape(-1).view(np.uint32), ref[k].reshape(-1).view(np.uint32)), (what, k)
    assert np.array_equal(got["diag"][:, 0], ref["diag"][:, 0]), (what, "RayCount")


def _all_forms(rt, ctx, desc, plist, n):
    """the plain launch of batch 0, the chain's final accumulators with the last batch's RayCount, the group's three frames"""
    ctx.upload_scene(desc)
    plain = rt.sample_batch_host(ctx, plist[0])
    stats = ctx.camera_ray_list_stats()
    bufs = [rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS]
    diags = [rt.DeviceBuffer(ctx, n * 4).zero() for _ in plist]
    outs = [[rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS] for _ in plist]
    try:
        rt.lib.check(rt.sample_batch_chain_device(ctx, plist, bufs, bufs, diags), "rtowSampleBatchChainDevice")
        ctx.synchronize()
        chain = {k: b.download(np.float32, (n, c)) for (k, c), b in zip(KEYS, bufs)}
        chain["diag"] = diags[2].download(np.float32, (n, 1))
        for b in bufs:
            b.zero()
        rt.lib.check(rt.sample_batch_group_device(ctx, plist, bufs, outs, diags), "rtowSampleBatchGroupDevice")
        ctx.synchronize()
        group = []
        for k in range(3):
            got = {key: b.download(np.float32, (n, c)) for (key, c), b in zip(KEYS, outs[k])}
            got["diag"] = diags[k].download(np.float32, (n, 1))
            group.append(got)
    finally:
        for b in bufs + diags + [x for o in outs for x in o]:
            b.free()
    return plain, chain, group, stats


def _mean(stats):
    listed = sum(stats["entries"])
    return sum(k * c for k, c in enumerate(stats["entries"])) / max(listed, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_pruned_lists_give_the_oracles_frame(rt, references, contexts, name):
    sc, desc, plist, alone, chain_ref = references[name]
    w, h = _size(name)
    n = w * h
    kinds = ("pruned", "unpruned", "walk") + (("ties pruned", "ties unpruned") if name == "tangent" else ())
    got = {kind: _all_forms(rt, contexts[kind], desc, plist, n) for kind in kinds}
    for kind in kinds:
        plain, chain, group, _ = got[kind]
        _same(plain, alone[0], (name, kind, "plain"))
        _same(chain, chain_ref, (name, kind, "chain"))
        for k in range(3):
            _same(group[k], alone[k], (name, kind, "group", k))
    for kind in kinds[1:]:                                          # (follows from the above; said outright: the same launch under the two development flags)
        for a, b in zip([got["pruned"][0], got["pruned"][1]] + got["pruned"][2], [got[kind][0], got[kind][1]] + got[kind][2]):
            _same(a, b, (name, "pruned against", kind))
    pruned, whole, walk = got["pruned"][3], got["unpruned"][3], got["walk"][3]
    cs = S.Compiled(sc)
    cpu = S.list_lengths(cs, plist[0], True) if n <= 64 * 36 else None
    print(name, "pruned", pruned["entries"], pruned["no_list"], "whole", whole["entries"], whole["no_list"], "CPU restatement", cpu)
    assert pruned["valid"] and pruned["pruned"] and whole["valid"] and not whole["pruned"] and not walk["valid"]
    for st in (pruned, whole):
        assert st["owned"] == n == sum(st["entries"]) + st["no_list"]
    listed = lambda st: sum(k * c for k, c in enumerate(st["entries"]))
    assert pruned["no_list"] <= whole["no_list"]
    if name in ("cover", "stack", "inside_glass", "tangent", "horizon", "lens", "moving", "one"):
        assert pruned["entries"] != whole["entries"] and (listed(pruned) < listed(whole) or pruned["no_list"] < whole["no_list"]), "lists get shorter"
    if name == "cover":
        assert _mean(pruned) < 0.75 * _mean(whole)
    if name == "stack":
        assert sum(whole["entries"][4:]) > 0 and sum(pruned["entries"][2:]) == 0, "nine spheres behind one another: one node is left"
    if name == "cluster":
        assert sum(pruned["entries"][5:9]) > 0 and pruned["no_list"] > 0, "lists of 5 to 8 nodes survive, longer ones still fall back to the walk"
    if name == "horizon":
        assert whole["entries"][0] == 0 and pruned["entries"][0] >= n // 3, "the ground's node leaves the lists of the sky pixels"
    if name == "one":
        assert whole["entries"][0] < pruned["entries"][0] and sum(pruned["entries"][2:]) == 0
    if cpu is not None:
        assert (pruned["entries"], pruned["no_list"]) == (cpu[0], cpu[1]), "the device's lists are the restatement's"


@pytest.mark.gpu
def test_diagnostic_records_keep_whole_lists(rt, references):
    """A launch with 16-byte records between two with 4-byte ones on one context: its BoundsHitCount / CandidateCount are those of a fresh context with whole lists,
    and the lists are rebuilt each time the record size changes."""
    sc, desc, _, alone, _ = references["cover"]
    w, h = _size("cover")
    small, big = _plist("cover", sc)[0], _plist("cover", sc, stride=16)[0]
    with rt.Context(0) as ctx, rt.Context(0, flags=rt.abi.CONTEXT_UNPRUNED_CAMERA_RAY_LISTS) as fresh:
        ctx.upload_scene(desc)
        fresh.upload_scene(desc)
        want = rt.sample_batch_host(fresh, big)
        assert not fresh.camera_ray_list_stats()["pruned"]
        first = rt.sample_batch_host(ctx, small)
        assert ctx.camera_ray_list_stats()["pruned"]
        got = rt.sample_batch_host(ctx, big)
        between = ctx.camera_ray_list_stats()
        assert between["valid"] and not between["pruned"] and between["entries"] == fresh.camera_ray_list_stats()["entries"]
        again = rt.sample_batch_host(ctx, small)
        assert ctx.camera_ray_list_stats()["pruned"]
    assert want["diag"].shape[1] == 4 and want["diag"][:, 1].sum() > 0 and want["diag"][:, 2].sum() > 0
    assert np.array_equal(got["diag"].view(np.uint32), want["diag"].view(np.uint32)), "all four counters of the 16-byte records"
    _same(got, alone[0], "16-byte records")
    _same(first, alone[0], "before")
    _same(again, alone[0], "after")
