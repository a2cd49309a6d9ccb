"""GPU: the LDS cursors of the headline kernels' box walk (csrc/rtow_sample_kernel.hip.h "LDS cursors of the walk") against the CPU oracle, bit for bit.

The static-sphere kernels with the scene in LDS and the path history in registers carry the top of a lane's traversal stack and the end of its candidate list as LDS
addresses, through the camera-ray lists, the walk and the exact tests.  A cursor that is off by a row reads another level's node or another slot's candidate; one that
is off by a lane reads a neighbour's.  Either shows in the frame.  Small scenes, each picked for an edge of the cursors:

  one      one sphere: the root has no second child, nothing is ever pushed, and every walk ends with a pop from the empty stack
  two      one node, two leaves;  three: a leaf next to an inner sibling
  row      eight glass spheres in a row along the view axis: a ray through their centres enters every box of the tree (the scene compiler builds it balanced: three
           inner levels = three stack rows), so every node with two inner children pushes and the visit's unconditional store reaches the plan's last row;
           all eight spheres are candidates of one ray: the walk hands over to the exact tests at its threshold and resumes, several times
  shells   two concentric mirror shells around the camera: both children are entered at distance 0 (equal: the near-first swap is false), every ray hits, every path
           runs to the trace depth
  stack    nine spheres stacked on the camera ray of the frame's centre: more candidates than the list holds (8), in the camera-ray lists as well

Frame 32 x 18, 4 samples; trace depth 4 (four history words) and 16 (eight); plain launch, a chain of 3 and a group of 3; with the 80-byte node image (sign-ordered
visit where the wave's rays allow) and in a context that keeps the 64-byte nodes (generic visit) - the cursors serve both.  Colour, normal, albedo, weight and RayCount
must be the oracle's.

test_scenes_exercise_their_cases (CPU) checks with the oracle alone that each scene does what it was picked for.
"""
import numpy as np
import pytest

KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))
W, H, SPP = 32, 18, 4
kCandCapacity = 8          # csrc/rtow_kernels.h


def _scene(rt, name):
    s = rt.scenes.Scene(name)
    grey = s.materials.append(rt.scenes.lambertian((0.6, 0.5, 0.4))) or 0
    mirror = s.materials.append(rt.scenes.metal((0.9, 0.9, 0.9), 0.0)) or 1
    glass = s.materials.append(rt.scenes.dielectric(1.5)) or 2
    s.camera = {"position": [0.0, 0.0, 4.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 40.0, "aperture": 0.0}
    if name in ("one", "two", "three"):
        s.add_sphere((0.0, 0.0, 0.0), 1.0, grey)
        if name != "one":
            s.add_sphere((1.3, 0.4, 0.8), 0.5, mirror)
        if name == "three":
            s.add_sphere((-1.2, -0.3, 0.5), 0.4, glass)
    elif name == "row":
        for i in range(8):
            s.add_sphere((0.0, 0.0, -1.5 * i), 0.6, glass)
    elif name == "shells":
        s.add_sphere((0.0, 0.0, 4.0), 6.0, mirror)
        s.add_sphere((0.0, 0.0, 4.0), 9.0, mirror)
    elif name == "stack":
        for i in range(9):
            s.add_sphere((0.0, 0.0, 2.0 - 1.0 * i), 0.45, glass if i % 2 else grey)
    else:
        raise KeyError(name)
    return s


SCENES = ("one", "two", "three", "row", "shells", "stack")


def _params(rt, scene, depth, seed=1):
    return rt.scenes.make_params(scene, W, H, spp=SPP, trace_depth=depth, seed=seed, focus=4.0)


@pytest.fixture(scope="module")
def references(rt, oracle):
    """(scene name, depth) -> (scene desc, the three batches' parameters, each batch alone, the three in a chain, the oracle's counters of batch 0): computed once"""
    out = {}
    for name in SCENES:
        scene = _scene(rt, name)
        desc = scene.desc()
        osc = oracle.OracleScene(desc)
        try:
            for depth in (4, 16):
                plist = [_params(rt, scene, depth, seed) for seed in (1, 2, 3)]
                first, counters = osc.sample_batch(plist[0], want_counters=True)
                alone = [first] + [osc.sample_batch(p) for p in plist[1:]]
                chain = alone[0]
                for p in plist[1:]:
                    chain = osc.sample_batch(p, {k: chain[k] for k, _ in KEYS})
                out[(name, depth)] = (desc, plist, alone, chain, counters)
        finally:
            osc.close()
    return out


@pytest.mark.parametrize("name", SCENES)
def test_scenes_exercise_their_cases(references, name):
    for depth in (4, 16):
        _, _, alone, _, c = references[(name, depth)]
        rays = alone[0]["diag"][:, 0]
        n = W * H
        print(name, depth, "rays", int(c.rays), "maxCandidates", c.maxCandidates, "maxNodeStack", c.maxNodeStack, "bvhDepth", c.bvhDepth, "max rays of a pixel", rays.max())
        assert rays.min() >= SPP                                     # every sample traces its camera ray
        if name in ("one", "two", "three"):
            assert rays.min() == SPP and rays.max() > SPP            # rays that miss everything (the walk ends on the empty stack) and rays that bounce
            assert c.maxCandidates >= 1
        elif name == "row":
            assert c.maxCandidates == 8                              # one ray inside all eight leaf boxes
            assert rays.max() == depth * SPP                         # straight through the glass: paths that use every segment they may
        elif name == "shells":
            assert c.maxCandidates == 2 and c.candidates == 2 * c.rays   # every ray starts inside both boxes: entry distance 0 for both children
            assert rays.min() == depth * SPP and rays.max() == depth * SPP
        elif name == "stack":
            assert c.maxCandidates == 9 > kCandCapacity


def _same(got, ref, what):
    for k, _ in KEYS:
        assert np.array_equal(got[k].reshape(-1).view(np.uint32), ref[k].reshape(-1).view(np.uint32)), (what, k)
    assert np.array_equal(got["diag"][:, 0], ref["diag"][:, 0]), (what, "RayCount")


@pytest.fixture(scope="module")
def contexts(rt):
    made = []
    for name, flags in (("image80", 0), ("image64", rt.abi.CONTEXT_NODE_IMAGE_64)):
        log = []
        made.append((name, rt.Context(0, log=lambda lvl, tag, msg, ud, log=log: log.append((tag.decode(), msg.decode())), log_level=4, flags=flags), log))
    yield made
    for _, ctx, _ in made:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [4, 16])
@pytest.mark.parametrize("name", SCENES)
def test_every_launch_form_gives_the_oracles_frame(rt, references, contexts, name, depth):
    desc, plist, alone, chain, _ = references[(name, depth)]
    n = W * H
    for cname, ctx, log in contexts:
        del log[:]
        ctx.upload_scene(desc)
        said = [m for tag, m in log if tag == "scene"]
        assert len(said) == 1 and ("80-byte node image" in said[0]) == (cname == "image80"), (cname, said)
        if name == "row":
            assert ctx.scene_info().bvhDepth == 3, "eight leaves under three inner levels: the axis ray's two pushes put the top on the last of three stack rows"
        _same(rt.sample_batch_host(ctx, plist[0]), alone[0], (name, depth, cname, "plain"))
        bufs = [rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS]
        diags = [rt.DeviceBuffer(ctx, n * 4).zero() for _ in plist]
        outs = [[rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS] for _ in plist]
        try:
            rt.lib.check(rt.sample_batch_chain_device(ctx, plist, bufs, bufs, diags), "rtowSampleBatchChainDevice")
            ctx.synchronize()
            got = {k: b.download(np.float32, (n, c)) for (k, c), b in zip(KEYS, bufs)}
            got["diag"] = diags[2].download(np.float32, (n, 1))
            _same(got, chain, (name, depth, cname, "chain"))
            for b in bufs:
                b.zero()
            rt.lib.check(rt.sample_batch_group_device(ctx, plist, bufs, outs, diags), "rtowSampleBatchGroupDevice")
            ctx.synchronize()
            for k in range(3):
                got = {key: b.download(np.float32, (n, c)) for (key, c), b in zip(KEYS, outs[k])}
                got["diag"] = diags[k].download(np.float32, (n, 1))
                _same(got, alone[k], (name, depth, cname, "group", k))
        finally:
            for b in bufs + diags + [x for o in outs for x in o]:
                b.free()
