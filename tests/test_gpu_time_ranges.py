"""GPU: the sample kernels on TimeRanges other than (0, 1) - the moving-sphere kernels (rtow_sample_spheres_motion[_ties].hip) with the common-range hoist at
(0.25, 0.75) and without it (mixed ranges, one reversed; sphere_at clamps per test), and the general kernel with the same ranges on a rect, a rotated box, a triangle and
a sphere - against OracleScene.sample_batch bit for bit: colour, normal, albedo, sample-count weight and RayCount.  The scenes are tests/query_edge_cases.py's; their
coincident twins make the tie watch and the _ties kernels run at sample times that clamp."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import query_edge_cases as qe  # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = (("color", 4), ("normal", 3), ("albedo", 3), ("scw", 1))
SPHERE_SCENES = ("ranges_common", "ranges_mixed")
RUNS = ([(name, how) for name in SPHERE_SCENES for how in ("reference", "per_sample", "xoroshiro", "chain", "wide")] + [("ranges_general", "reference")])


def _same(got, ref, what):
    for k, _ in KEYS:
        a, b = got[k].reshape(ref[k].shape).view(np.uint32), ref[k].view(np.uint32)
        assert np.array_equal(a, b), (what, k, int((a != b).reshape(len(a), -1).any(axis=1).sum()))
    assert np.array_equal(got["diag"][:, 0], ref["diag"][:, 0]), (what, "RayCount")


@pytest.mark.parametrize("name,how", RUNS)
def test_time_range_frames_equal_the_oracle(rt, oracle, name, how):
    """64 x 36, 4 samples per pixel, trace depth 6.  reference / per_sample / xoroshiro: the three RNG policies; chain: two batches through rtowSampleBatchChainDevice
    against the oracle's two batches in sequence; wide: RTOW_CONTEXT_FORCE_WIDE_CODES.  Input condition, from the oracle alone: the frame differs from the same scene's
    with every TimeRange set to (0, 1) in at least 10 % of its pixels (measured: 54 %, 50 % and 21 % for the three scenes) - so a kernel that took the ranges for (0, 1)
    cannot pass."""
    abi = rt.abi
    policy = {"per_sample": abi.RNG_PER_SAMPLE, "xoroshiro": abi.RNG_PER_SAMPLE_XOROSHIRO}.get(how, abi.RNG_REFERENCE)
    share = qe.share_of_pixels_the_ranges_change(rt, oracle, name, policy)
    print("%s %s: %.1f %% of the pixels differ from the (0, 1) frame" % (name, how, 100 * share))
    assert share >= 0.10, (name, how, share)
    scene, desc, ref = qe.oracle_frames(rt, oracle, name, policy)
    w, h = qe.FRAME[:2]
    n = w * h
    plist = [qe.frame_params(rt, scene, policy, seed) for seed in (1, 2)]
    with rt.Context(0, **({"flags": abi.CONTEXT_FORCE_WIDE_CODES} if how == "wide" else {})) as ctx:
        ctx.upload_scene(desc)
        info = ctx.scene_info()
        assert info.wideCodes == (1 if how == "wide" else 0)
        if how != "chain":
            _same(rt.sample_batch_host(ctx, plist[0]), ref[0], (name, how))
            return
        bufs = [rt.DeviceBuffer(ctx, n * c * 4).zero() for _, c in KEYS]
        diags = [rt.DeviceBuffer(ctx, n * 4).zero() for _ in plist]
        rt.lib.check(rt.sample_batch_chain_device(ctx, plist, bufs, bufs, diags), "rtowSampleBatchChainDevice")
        ctx.synchronize()
        got = {k: b.download(np.float32, (n, c)) for (k, c), b in zip(KEYS, bufs)}
        first_rays = diags[0].download(np.float32, (n, 1))
        got["diag"] = diags[1].download(np.float32, (n, 1))
        for b in bufs + diags:
            b.free()
    assert np.array_equal(first_rays[:, 0], ref[0]["diag"][:, 0]), (name, how, "RayCount of the first batch")
    _same(got, ref[1], (name, how))
