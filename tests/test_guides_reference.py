"""CPU: tests/guides_reference.py - the numpy restatement of rtowTraceGuideRaysDevice's specification - anchored against the oracle without a GPU: its mirror and glass
directions against the oracle's Material.Scatter, and its end point against the albedo and normal AOVs of the oracle's own sample path on a scene of mirrors."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guides_reference as ref  # noqa: E402
import shade_hits_reference as shade  # noqa: E402

f32 = np.float32


def _scatter(oracle, material, rd, normal, state):
    """the oracle's Material.Scatter at a hit with normal `normal`: (scattered direction, reflectance)"""
    out = (C.c_float * 16)()
    s = C.c_uint32(state)
    zero = (C.c_float * 3)(0, 0, 0)
    oracle.load().oracle_kat_scatter(C.byref(material), zero, ref._c3(rd), 0.0, zero, ref._c3(normal), 1.0, C.byref(s), out)
    assert out[12] == 1.0                                                          # Material.IsPerfectSpecular
    return np.asarray(out[6:9], dtype=f32), np.asarray(out[0:3], dtype=f32)


def _cases(seed, count):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        n = ref.normalize(rng.normal(size=3).astype(f32))
        rd = rng.normal(size=3).astype(f32)
        if rng.random() < 0.5:
            rd = ref.normalize(rd)
        yield rd, n


def test_a_mirror_scatters_along_the_restatements_reflection(rt, oracle):
    """Standard with metallic 1 and glossiness 1: whichever of its two reflecting branches the coin picks, the direction is reflect(rd, N)"""
    white = 0
    for material in (rt.scenes.metal((0.9, 0.8, 0.7), 0), rt.scenes.metal((1, 1, 1), 0)):
        assert shade.is_perfect_specular(material)
        albedo = shade.sample_color(None, material.albedo, (0, 0))
        for rd, n in _cases(5, 12):
            if ref.dot(rd, n) > 0:
                n = (-n).astype(f32)
            want, tint, _ = ref.scatter(oracle, material, rd, n, albedo)
            for state in (1, 12345, 0x9e3779b9, 0xfffffffe, 77):
                got, reflectance = _scatter(oracle, material, rd, n, state)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (rd, n, state)
                # the glossy branch the chain leaves out is untinted; the other carries the albedo the chain multiplies in
                assert np.array_equal(reflectance, tint) or np.array_equal(reflectance, np.ones(3, f32)), (reflectance, tint)
                white += int(not np.array_equal(reflectance, tint))
    print("untinted reflections among the draws:", white)


def test_glass_scatters_along_the_restatements_refraction_or_reflection(rt, oracle):
    """Dielectric with glossiness 1 over 64 rng states: every scattered direction is the restatement's refracted or its reflected direction, bit for bit up to the sign of
    a zero component (the reference adds 0 * a random direction to the normal); both occur, and so does total internal reflection."""
    material = rt.scenes.dielectric(1.5)
    albedo = shade.sample_color(None, material.albedo, (0, 0))
    same = lambda a, b: np.all((a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0)))
    refracted = reflected = total = 0
    for k, (rd, n) in enumerate(_cases(9, 40)):
        if k % 2:                                                                   # from inside, at a grazing angle now and then
            n = n if ref.dot(rd, n) > 0 else (-n).astype(f32)
            if k % 4 == 1:
                rd = (rd - (f32(0.9) * ref.dot(rd, n) * n).astype(f32)).astype(f32)
        want, tint, took_reflection = ref.scatter(oracle, material, rd, n, albedo)
        mirror = ref.reflect(rd, ref.normalize(n))
        total += took_reflection
        if took_reflection:
            assert np.array_equal(want, mirror) and np.array_equal(tint, np.ones(3, f32))
        for state in range(1, 65):
            got, _ = _scatter(oracle, material, rd, n, state * 2654435761 % 2**32 or 1)
            if same(got, want) and not took_reflection:
                refracted += 1
            else:
                assert same(got, mirror), (k, state, got, want, mirror)
                reflected += 1
    print("refracted %d, reflected %d, cases under total internal reflection %d" % (refracted, reflected, total))
    assert refracted > 0 and reflected > 0 and total > 0


def test_the_chains_end_point_is_the_oracles_one_sample_aov(rt, oracle):
    """The mirror scene at 61 x 37: the oracle's SampleBatchJob (1 spp, jitter off, lens 0, white noise, traceDepth 9, zeroed accumulators) holds, at every pixel whose chain
    is not cut, 0 + (emission + albedo) of the chain's end surface (the gradient sky along the last direction on a miss) and 0 + N (0 + -direction on a miss): uint32 words."""
    w, h = 61, 37
    scene = ref.mirror_scene(rt)
    desc = scene.desc()
    p = ref.mirror_params(rt, scene, w, h)
    rays = shade.view_rays(p.view, w, h)
    got, _ = ref.guides(oracle, scene, desc, rays, 8)
    osc = oracle.OracleScene(desc)
    try:
        sample = osc.sample_batch(p)
    finally:
        osc.close()
    surface = shade.surface(oracle, scene, desc, got["rays"], got["entityIndex"], p.environment)
    albedo, normal = ref.expected_aovs(scene, p.environment, got["rays"], got["entityIndex"], got["normal"], surface)
    keep = got["end"] != ref.END_CUT
    print("%d of %d pixels compared; bounces: %s" % (keep.sum(), w * h, np.bincount(got["bounces"]).tolist()))
    assert keep.all() and got["bounces"].max() >= 3 and (got["end"] == ref.END_SKY).any() and (got["bounces"] >= 1).sum() > w * h // 10
    have_albedo = (f32(0) + sample["albedo"]).astype(f32)
    have_normal = (f32(0) + sample["normal"]).astype(f32)
    bad = ~(shade.same_bits(have_albedo, albedo).all(axis=1) & shade.same_bits(have_normal, normal).all(axis=1)) & keep
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8], have_albedo[bad][:3], albedo[bad][:3], have_normal[bad][:3], normal[bad][:3])
    # the same frame cut after one surface: exactly the pixels whose chain goes on are cut, at the second mirror
    cut, _ = ref.guides(oracle, scene, desc, rays, 1)
    assert np.array_equal((cut["end"] == ref.END_CUT) & (cut["bounces"] == 1), got["bounces"] > 1) and (got["bounces"] > 1).sum() > 10
