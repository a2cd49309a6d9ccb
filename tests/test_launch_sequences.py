"""CPU: the mutation table of tests/launch_sequences.py covers RtowSampleParams leaf by leaf, and why the fraction of Size belongs in the key of the camera-ray lists.

(a) Every leaf field of abi.SampleParams is changed by at least one mutation and every mutation changes its block: a field added to the struct later fails here until the
    table has a mutation for it, and tests/test_gpu_launch_sequences.py then runs it under a warm context.
(b) On the host restatement of primary_candidates_kernel (tests/camera_lists_support.py): a pixel's beam spans cx / Size.x .. (cx + 1) / Size.x, so lists built for
    64 x 36 are not the lists of 64.9 x 36.9 - some pixel's new list names a node the old one lacks, and some camera ray of the larger Size has its nearest sphere in a
    leaf the old list does not keep.  With equal sizes both counts are 0."""
import ctypes as C

import numpy as np
import pytest

import camera_lists_support as S
import launch_sequences as L

abi = L.abi


def test_every_leaf_of_the_struct_has_a_mutation():
    scene = L.scenes.tiny_scene()
    P = L.base_params(scene, 32, 18)
    leaves = L.leaves()
    assert sum(size for _, _, size in leaves) == C.sizeof(abi.SampleParams), "no padding: every byte of the block belongs to a leaf"
    changed_by = {name: [] for name, _, _ in leaves}
    for m in L.MUTATIONS:
        p0 = m.base(P, scene)
        p1 = m.apply(p0, scene)
        assert bytes(p0) == bytes(m.base(P, scene)), (m, "apply must not modify its argument")
        b0, b1 = bytes(p0), bytes(p1)
        assert b0 != b1, (m, "changes nothing")
        for name, at, size in leaves:
            if b0[at:at + size] != b1[at:at + size]:
                changed_by[name].append(m.name)
    missing = [name for name, by in changed_by.items() if not by]
    assert not missing, ("no mutation changes", missing)
    for name, by in changed_by.items():
        print("%-32s %s" % (name, ", ".join(by)))


def test_the_fractional_sizes_keep_the_integer_frame():
    """what the issue's four fractional sizes are: (int) Size stays W x H, the float does not"""
    for w, h in ((32, 18), (64, 36), (512, 144)):
        sizes = L.fractional_sizes(w, h)
        assert len(set(sizes)) == 4
        for x, y in sizes:
            assert (int(x), int(y)) == (w, h) and (x, y) != (float(w), float(h)), (x, y)
        assert sizes[3] == (float(np.nextafter(np.float32(w + 1), np.float32(0))), float(np.nextafter(np.float32(h + 1), np.float32(0))))
    scene = L.scenes.tiny_scene()
    P = L.base_params(scene, 32, 18)
    got = [(q.size.x, q.size.y) for q in (L.BY_NAME[name].apply(P, scene) for name in L.SIZE_FRACTIONAL)]
    assert got == L.fractional_sizes(32, 18)


def test_expected_status_follows_the_per_batch_checks():
    scene = L.scenes.tiny_scene()
    P = L.base_params(scene, 32, 18)
    bad, unsupported, ok = abi.RTOW_ERROR_INVALID_VALUE, abi.RTOW_ERROR_UNSUPPORTED, abi.RTOW_SUCCESS

    def status(entry, name):
        m = L.BY_NAME[name]
        p0 = m.base(P, scene)
        return L.expected_status(entry, [p0, m.apply(p0, scene), p0])

    for name in L.SIZE_FRACTIONAL:
        assert [status(e, name) for e in L.ENTRY_POINTS] == [ok, ok, ok, ok, bad], name        # the adaptive call's reduction wants one Size, bit for bit
    for name in ("size.x+1", "size.y+1", "size transposed", "diagnosticsStride 16"):
        assert [status(e, name) for e in L.ENTRY_POINTS] == [ok, bad, ok, bad if name != "diagnosticsStride 16" else ok, bad], name
    for name in ("slice 0/2", "slice 1/2", "slice 2/3"):
        assert [status(e, name) for e in L.ENTRY_POINTS] == [ok, bad, ok, bad, bad], name
    assert [status(e, "rngPolicy 1") for e in L.ENTRY_POINTS] == [ok, ok, ok, unsupported, ok]
    assert [status(e, "rngPolicy 1 -> 2") for e in L.ENTRY_POINTS] == [ok, ok, ok, unsupported, ok]
    for name in ("seed", "camera position", "traceDepth 64", "noise blue", "sky cubemap", "lensRadius 0.1 -> -0.1", "extrema maximum"):
        assert [status(e, name) for e in L.ENTRY_POINTS] == [ok] * 5, name


# ------------------------------------------------------------------ (b) ------------------------------------------------------------------
def _leaf_nodes(cs):
    """primitive -> the tree node whose leaf child it is, read from the compiled blob (GpuNode: 64 bytes, child0 / child1 at bytes 48 / 52, a leaf child is ~primitive)"""
    node_offset, node_count = int(cs.layout[0]), int(cs.layout[1])
    raw = np.frombuffer(cs.buf, np.uint8, node_count * 64, node_offset).reshape(node_count, 64)
    children = raw[:, 48:56].copy().view(np.int32)
    out = {}
    for node in range(node_count):
        for child in children[node]:
            if child < 0:
                out.setdefault(int(~child), node)
    return out


def _stale_counts(name, w, h, delta, rays_per_pixel=16):
    """lists built for W x H, rays and lists of (W + delta) x (H + delta): (pixels whose new pruned list names a node the old pruned list lacks, the same for the whole
    lists, rays whose nearest sphere's leaf the old pruned list does not keep, pixels with such a ray, rays drawn)"""
    sc = S.scene(name)
    cs = S.Compiled(sc)
    old = S.params(sc, w=w, h=h, name=name)
    new = L.copy_params(old)
    new.size = abi.Float2(float(np.float32(w + delta)), float(np.float32(h + delta)))
    assert (int(new.size.x), int(new.size.y)) == (w, h)
    node_of = _leaf_nodes(cs)
    grown = grown_whole = lost_rays = lost_pixels = drawn = 0
    for cy in range(h):
        for cx in range(w):
            kept, _, _ = cs.pixel(old, cx, cy)
            if kept is None or len(kept) > S.LIST_CAPACITY:
                continue                                      # no list: the pixel's rays walk the tree, nothing can be stale
            wanted, _, _ = cs.pixel(new, cx, cy)
            grown += wanted is None or not set(wanted) <= set(kept)
            whole_old, whole_new = cs.pixel(old, cx, cy, prune=False)[0], cs.pixel(new, cx, cy, prune=False)[0]
            grown_whole += whole_old is not None and (whole_new is None or not set(whole_new) <= set(whole_old))
            _, nearest, _ = cs.rays(new, cx, cy, rays_per_pixel, 1, [])
            lost = sum(1 for prim in nearest.tolist() if prim >= 0 and node_of[prim] not in kept)
            drawn += rays_per_pixel
            lost_rays += lost
            lost_pixels += lost > 0
    return grown, grown_whole, lost_rays, lost_pixels, drawn


@pytest.mark.parametrize("name,w,h", [("cover", 64, 36), ("one", 32, 18)])
def test_lists_of_the_integer_size_are_stale_for_a_fractional_size(name, w, h):
    grown, grown_whole, lost_rays, lost_pixels, drawn = _stale_counts(name, w, h, 0.9)
    print("%s %d x %d -> +0.9: the new pruned list names a node the old one lacks in %d pixels (whole lists: %d); %d of %d rays in %d pixels have their nearest sphere in a "
          "leaf the old list does not keep" % (name, w, h, grown, grown_whole, lost_rays, drawn, lost_pixels))
    assert grown >= 1, "the pruned lists of Size + 0.9 are a subset of the integer Size's in every pixel"
    assert lost_rays >= 1, "every ray of the larger Size finds its nearest sphere in the integer Size's list"
    same = _stale_counts(name, w, h, 0.0)
    assert same[:4] == (0, 0, 0, 0), same
