"""GPU: the 44-instruction node visit of the headline kernels (csrc/rtow_sample_kernel.hip.h: leaf codes ready to store, the empty-stack sentinel row, the strict inner
test) against the CPU oracle, bit for bit, where each of the three can go wrong.

Frames of 64 x 36 at 4 samples, seeds 1 .. 3, through plain, chained (3 batches) and grouped launches in both contexts - the default one (80-byte image, codes re-encoded
while the image is staged) and CONTEXT_NODE_IMAGE_64 (64-byte nodes, codes re-encoded per load) - at trace depth 8 and 16 (the HW 4 and HW 8 kernels), as in
tests/test_gpu_signed_walk.py, whose launcher this reuses:
  (a) the 200-sphere exponentially spaced chain of tests/test_scene_compiler.py: its tree takes all 24 stack rows, so the sentinel sits under a full stack and the top row
      is used;
  (b) sixteen glass and lambert spheres strung along the view axis behind one another: camera lists of five to eight nodes and candidate lists that reach the flush
      bound under the sentinel row - with the default hand-over count, with schedulerTune[6] = 7 (confined to 6 in these kernels) and with 1;
  (c) three spheres, a root with one leaf and one inner child: the first pop of nearly every walk meets the empty stack."""
import numpy as np
import pytest

from test_gpu_signed_walk import H, SPP, W, _all_entry_points, contexts  # noqa: F401

pytestmark = pytest.mark.gpu


def _chain_scene(rt):
    s = rt.scenes.Scene("chain")
    m = rt.scenes.lambertian((0.5, 0.5, 0.5))
    for i in range(200):
        s.add_sphere((1.5 ** (i * 0.25) * 3.0, 0.0, 0.0), 1.5 ** (i * 0.25), m if i == 0 else 0)
    # seen from near the origin every sphere fills the same cone around +x (centre 3 r, radius r): the frame looks down that cone
    s.camera = {"position": [-2.0, 0.5, 0.5], "target": [10.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 30.0, "aperture": 0.0}
    return s


def _strung_scene(rt):
    s = rt.scenes.Scene("strung")
    glass = s.materials.append(rt.scenes.dielectric(1.5)) or 0
    grey = s.materials.append(rt.scenes.lambertian((0.6, 0.5, 0.4))) or 1
    for i in range(16):
        s.add_sphere((0.05 * (i % 3 - 1), 0.04 * (i % 2), -1.6 * i), 0.7 + 0.02 * i, grey if i % 4 == 3 else glass)
    s.camera = {"position": [0.0, 0.0, 6.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 25.0, "aperture": 0.0}
    return s


def _three_scene(rt):
    s = rt.scenes.Scene("three")
    s.add_sphere((-4.0, 0.0, 0.0), 1.0, rt.scenes.lambertian((0.7, 0.3, 0.3)))
    s.add_sphere((1.5, 0.0, 0.0), 1.0, rt.scenes.metal((0.8, 0.8, 0.8), 0.05))
    s.add_sphere((3.6, 0.2, 0.3), 1.0, rt.scenes.lambertian((0.3, 0.3, 0.7)))
    s.camera = {"position": [0.0, 1.5, 9.0], "target": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov": 50.0, "aperture": 0.0}
    return s


def _scene_info(rt, scene):
    with rt.Context(0) as ctx:
        ctx.upload_scene(scene.desc())
        info = ctx.scene_info()
        return int(info.bvhDepth), int(info.bvhNodeCount), int(info.sceneInLds)


@pytest.mark.parametrize("depth", [8, 16])
def test_full_stack_over_the_sentinel(rt, oracle, contexts, depth):  # noqa: F811
    scene = _chain_scene(rt)
    levels, _, in_lds = _scene_info(rt, scene)
    assert levels == 24 and in_lds == 1, (levels, in_lds)        # input condition: every stack row, the top one included, belongs to this tree
    ref = _all_entry_points(rt, oracle, contexts, scene, W, H, SPP, depth, focus=10.0)
    assert ref["diag"][:, 0].sum() > 1.25 * W * H * SPP, "input condition: at least a quarter of the samples bounce - the walk runs, not only the camera-ray lists"


@pytest.mark.parametrize("depth", [8, 16])
@pytest.mark.parametrize("handover", [0, 7, 1])
def test_long_camera_lists_and_full_candidate_lists(rt, oracle, contexts, handover, depth):  # noqa: F811
    """handover: schedulerTune[6], the candidates a walk collects before it hands them to the exact tests (0: the built-in value)"""
    scene = _strung_scene(rt)
    if handover == 0:
        used = contexts
    else:
        used = [(name, rt.Context(0, log=lambda lvl, tag, msg, ud, log=log: log.append((tag.decode(), msg.decode())), log_level=4, flags=flags,
                            scheduler_tune=[0] * 6 + [handover, 0, 0]), log)
                for name, flags, log in (("image80", 0, []), ("image64", rt.abi.CONTEXT_NODE_IMAGE_64, []))]
    try:
        ref = _all_entry_points(rt, oracle, used, scene, W, H, SPP, depth, focus=6.0)
    finally:
        if used is not contexts:
            for _, ctx, _ in used:
                ctx.close()
    # input condition: rays go through many spheres one behind the other (glass passes them on), so paths are long where the spheres are
    assert ref["diag"][:, 0].max() >= 6 * SPP, ref["diag"][:, 0].max()


@pytest.mark.parametrize("depth", [8, 16])
def test_first_pop_meets_the_empty_stack(rt, oracle, contexts, depth):  # noqa: F811
    scene = _three_scene(rt)
    levels, nodes, _ = _scene_info(rt, scene)
    assert nodes == 2 and levels == 2, (levels, nodes)            # a root with one leaf and one inner child
    ref = _all_entry_points(rt, oracle, contexts, scene, W, H, SPP, depth, focus=9.0)
    assert ref["diag"][:, 0].max() >= 2 * SPP
