"""GPU: the sign-ordered box walk of the sphere kernels (csrc/rtow_sample_kernel.hip.h "sign-ordered box walk") against the CPU oracle, bit for bit.

The static-sphere kernels with the scene in LDS and the path history in registers (trace depth <= 8 / <= 16) walk an 80-byte node image whose planes the
ray's sign picks by address, whenever every walking lane of a wave has a finite origin and three finite non-zero reciprocal direction components; otherwise the whole
wave runs the generic slab test on the same image.  A context created with CONTEXT_NODE_IMAGE_64 keeps the 64-byte nodes and the generic test everywhere.  Both must
give the oracle's frames - colour, normal, albedo, weight and RayCount - through the plain, the chained and the grouped entry point: camera rays (the list loops of REGEN
and TEST) and bounces (the walk, all eight sign octants after a diffuse bounce).  The moving-sphere kernels keep the 64-byte nodes (csrc: signed_walk_variant); their scene
runs through the same launches in both contexts all the same."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))
W, H, SPP = 64, 36, 4


@pytest.fixture(scope="module")
def contexts(rt):
    """(name, context, its level-4 log) for the default context (80-byte image where it fits) and one that keeps the 64-byte nodes"""
    made = []
    for name, flags in (("image80", 0), ("image64", rt.abi.CONTEXT_NODE_IMAGE_64)):
        log = []
        made.append((name, rt.Context(0, log=lambda lvl, tag, msg, ud, log=log: log.append((tag.decode(), msg.decode())), log_level=4, flags=flags), log))
    yield made
    for _, ctx, _ in made:
        ctx.close()


def _same(got, ref, what, diag=True):
    for k, _ in KEYS:
        assert np.array_equal(got[k].reshape(-1).view(np.uint32), ref[k].reshape(-1).view(np.uint32)), (what, k)
    if diag:
        assert np.array_equal(got["diag"][:, 0], ref["diag"][:, 0]), (what, "RayCount")


def _download(bufs, n):
    return {k: b.download(np.float32, (n, c)) for (k, c), b in zip(KEYS, bufs)}


def _all_entry_points(rt, oracle, contexts, scene, w, h, spp, depth, expect_image=True, **kw):
    """one frame through plain, chained (3 batches) and grouped (3 batches) launches in both contexts; the oracle's frames are computed once"""
    desc = scene.desc()
    plist = [rt.scenes.make_params(scene, w, h, spp=spp, trace_depth=depth, seed=s, **kw) for s in (1, 2, 3)]
    n = w * h
    osc = oracle.OracleScene(desc)
    try:
        alone = [osc.sample_batch(p) for p in plist]                       # each batch from zeroed accumulators: the plain launch and the group
        chain = alone[0]
        for p in plist[1:]:                                                # the three batches one after the other: the chain
            chain = osc.sample_batch(p, {k: chain[k] for k, _ in KEYS})
    finally:
        osc.close()
    for name, ctx, log in contexts:
        del log[:]
        ctx.upload_scene(desc)
        said = [m for tag, m in log if tag == "scene"]
        assert len(said) == 1 and ("80-byte node image" in said[0]) == (name == "image80" and expect_image), (name, said)
        _same(rt.sample_batch_host(ctx, plist[0]), alone[0], (name, "plain"))
        bufs = [rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS]
        diags = [rt.DeviceBuffer(ctx, n * 4).zero() for _ in plist]
        rt.lib.check(rt.sample_batch_chain_device(ctx, plist, bufs, bufs, diags), "rtowSampleBatchChainDevice")
        ctx.synchronize()
        got = _download(bufs, n)
        got["diag"] = diags[2].download(np.float32, (n, 1))
        _same(got, chain, (name, "chain"))
        for b in bufs:
            b.zero()
        outs = [[rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS] for _ in plist]
        rt.lib.check(rt.sample_batch_group_device(ctx, plist, bufs, outs, diags), "rtowSampleBatchGroupDevice")
        ctx.synchronize()
        for k in range(3):
            got = _download(outs[k], n)
            got["diag"] = diags[k].download(np.float32, (n, 1))
            _same(got, alone[k], (name, "group", k))
        for b in bufs + diags + [x for o in outs for x in o]:
            b.free()
    return alone[0]


@pytest.mark.parametrize("which,depth", [("cover", 8), ("cover", 16), ("moving", 8), ("moving", 16)])
def test_cover_and_moving_scenes_every_entry_point(rt, oracle, contexts, which, depth):
    """trace depth 8: the 4-word history kernels; 16: the 8-word ones.  The moving scene has a lens (the origin differs per sample) and no image."""
    scene = rt.scenes.cover_scene() if which == "cover" else rt.scenes.moving_scene()
    ref = _all_entry_points(rt, oracle, contexts, scene, W, H, SPP, depth, expect_image=which == "cover")
    assert ref["diag"][:, 0].sum() > 2.0 * W * H * SPP, "the frame bounces: the walk runs, not only the camera-ray lists"


def _axis_scene(rt):
    """Camera on the z axis looking exactly along it at mirrors centred on the axis: with an odd frame and no jitter the centre pixel's ray has two zero direction
    components (its reciprocal: two infinities), and so has every bounce of it between the two mirrors.  One sphere's box has a plane through the ray's x."""
    s = rt.scenes.Scene("axis")
    mirror = s.materials.append(rt.scenes.metal((0.9, 0.9, 0.9), 0.0)) or 0
    grey = s.materials.append(rt.scenes.lambertian((0.5, 0.5, 0.5))) or 1
    s.add_sphere((0.0, 0.0, 0.0), 1.0, mirror)
    s.add_sphere((0.0, 0.0, 12.0), 2.0, mirror)                  # behind the camera: the axis ray bounces between the two
    s.add_sphere((0.5, 0.0, -3.0), 0.5, grey)                    # box plane lo.x == 0 == the axis ray's origin.x: 0 x inf if the wave took the ordered visit
    s.add_sphere((0.0, -101.0, 0.0), 100.0, grey)
    for i in range(12):
        s.add_sphere((2.5 * np.cos(i * 0.5236), 0.3 * (i % 3), 2.5 * np.sin(i * 0.5236)), 0.4, grey if i % 2 else mirror)
    s.camera = {"position": [0.0, 0.0, 5.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    return s


@pytest.mark.parametrize("depth", [8, 16])
def test_axis_rays_take_the_generic_visit(rt, oracle, contexts, depth):
    scene = _axis_scene(rt)
    w, h = 63, 35
    p = rt.scenes.make_params(scene, w, h, spp=SPP, trace_depth=depth, jitter=False, focus=5.0)
    # input condition: the centre pixel's direction has two components that are exactly zero
    v = p.view
    u = np.float32(np.float32(w // 2) + np.float32(0.5)) / np.float32(w)
    t = np.float32(np.float32(h // 2) + np.float32(0.5)) / np.float32(h)
    dx = np.float32(np.float32(v.lowerLeftCorner.x) + u * np.float32(v.horizontal.x)) + t * np.float32(v.vertical.x)
    dy = np.float32(np.float32(v.lowerLeftCorner.y) + u * np.float32(v.horizontal.y)) + t * np.float32(v.vertical.y)
    assert dx == 0.0 and dy == 0.0, (dx, dy)
    ref = _all_entry_points(rt, oracle, contexts, scene, w, h, SPP, depth, jitter=False, focus=5.0)
    centre = (h // 2) * w + w // 2
    assert ref["diag"][centre, 0] >= 2 * SPP, "the axis ray bounces off the mirror in front of it"


@pytest.mark.parametrize("count", [1, 2])
def test_one_and_two_entity_scenes(rt, oracle, contexts, count):
    """one entity: the root's second child is a placeholder the kernel masks (twoChildren false); two: the smallest real node"""
    s = rt.scenes.Scene("few%d" % count)
    s.add_sphere((0.0, 0.0, 0.0), 1.0, rt.scenes.lambertian((0.6, 0.3, 0.3)))
    if count == 2:
        s.add_sphere((1.2, 0.4, 1.0), 0.5, rt.scenes.metal((0.8, 0.8, 0.8), 0.1))
    s.camera = {"position": [3.0, 1.5, 4.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 35.0, "aperture": 0.0}
    ref = _all_entry_points(rt, oracle, contexts, s, W, H, SPP, 8, focus=5.0)
    assert ref["diag"][:, 0].max() >= 2 * SPP


@pytest.mark.parametrize("visits", [65535, 65536, 100000, 1 << 20])
def test_any_positive_slice_is_a_legal_option(rt, oracle, visits):
    """RtowContextOptions.schedulerTune[8], the walk's visits per trip, is a caller's value and any positive one is legal (a huge one means "never slice").  Bit 16 of the
    kernel's slice word carries the image grant: a caller's 65 536 or 100 000 has that bit set and 1 << 20 has sixteen zero bits below it - the host confines the value
    (csrc/rtow_kernels.h travSliceOf, held to its contract on the CPU by tests/test_node_image.py), the image is still staged, and the frame is the oracle's."""
    scene = rt.scenes.cover_scene()
    desc = scene.desc()
    p = rt.scenes.make_params(scene, W, H, spp=SPP, trace_depth=8)
    osc = oracle.OracleScene(desc)
    try:
        ref = osc.sample_batch(p)
    finally:
        osc.close()
    log = []
    with rt.Context(0, log=lambda lvl, tag, msg, ud: log.append((tag.decode(), msg.decode())), log_level=4, scheduler_tune=[0] * 8 + [visits]) as ctx:
        ctx.upload_scene(desc)
        assert any(tag == "scene" and "80-byte node image" in m for tag, m in log), log
        assert ctx.scene_info().ldsBytesScene == ctx.scene_info().sceneBytesDevice + 16 * ctx.scene_info().bvhNodeCount
        _same(rt.sample_batch_host(ctx, p), ref, ("slice", visits))
