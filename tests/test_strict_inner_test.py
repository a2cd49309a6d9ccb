"""CPU: the strict inner-child test of the sign-ordered node visit loses no candidate (csrc/rtow_sample_kernel.hip.h, finishVisit).

The sign-ordered loop tests every child - leaf or inner - with tmin <= bestPrune && tmin < tfar.  For a leaf that is the reference's own test.  For an inner child it is
stricter than the tmin <= min(tfar, bestPrune) the generic loop keeps: it skips inner boxes the ray meets with tmin == tfar.  The claim: a stored child box encloses the
stored boxes of its children, (plane - o) * inv is monotone in the plane for a finite origin and a finite non-zero inv, max3 / min3 are monotone, so
tmin_inner <= tmin_leaf < tfar_leaf <= tfar_inner for every passing leaf - every ancestor of a passing leaf passes the strict test too.

This restates the visit's expressions in numpy float32 (subtract, then multiply, near / far plane by the sign of inv, max3 with the clamp at 0 / min3), walks the FULL tree
for every ray once with each inner test and asserts the two sets of passing leaves are equal ray by ray, for bestPrune = inf and a few finite values:
  * the cover scene's compiled tree with random rays;
  * a synthetic tree of grid cubes with small-integer planes, integer origins and power-of-two inv components: the arithmetic is exact, rays run through box edges and
    corners, and the test asserts that inner children with tmin == tfar do occur among the visited ones - it cannot pass vacuously."""
import numpy as np
import pytest

from test_leaf_codes import _nodes, rt, shim  # noqa: F401  (the scene compiler through the host-only shim)

F = np.float32


def _tree_of_words(words):
    """64-byte nodes (uint32[count, 16]) -> lo, hi as float32[count, child, axis] and the children as int32[count, 2] (a leaf is ~prim)"""
    planes = words[:, :12].view(np.float32)
    lo = planes[:, 0:6].reshape(-1, 3, 2).transpose(0, 2, 1).copy()
    hi = planes[:, 6:12].reshape(-1, 3, 2).transpose(0, 2, 1).copy()
    return lo, hi, words[:, 12:14].view(np.int32).copy()


def _passing_leaves(tree, o, inv, prune, strict):
    """every leaf whose own test passes under ancestors that all pass the inner test, per ray: bool[prims, rays]; and how many visited inner children had tmin == tfar"""
    lo, hi, child = tree
    rays = o.shape[0]
    prims = int((~child[child < 0]).max()) + 1
    reached = np.zeros((child.shape[0], rays), bool)
    reached[0] = True
    out = np.zeros((prims, rays), bool)
    equalities = 0
    order = [0]
    for node in order:
        for c in (0, 1):
            down = inv < 0                                                    # near plane: lo, or hi when the ray runs down the axis
            near = np.where(down, hi[node, c][None, :], lo[node, c][None, :]).astype(F)
            far = np.where(down, lo[node, c][None, :], hi[node, c][None, :]).astype(F)
            tn = ((near - o).astype(F) * inv).astype(F)                       # sub, then mul: two roundings, as the packed instructions do
            tf = ((far - o).astype(F) * inv).astype(F)
            tmin = np.maximum(np.maximum(tn[:, 0], tn[:, 1]), np.maximum(tn[:, 2], F(0)))
            tfar = np.minimum(np.minimum(tf[:, 0], tf[:, 1]), tf[:, 2])
            code = int(child[node, c])
            if code < 0:
                out[~code] |= reached[node] & (tmin <= prune) & (tmin < tfar)
            else:
                hit = (tmin <= prune) & (tmin < tfar) if strict else tmin <= np.minimum(tfar, prune)
                equalities += int((reached[node] & (tmin == tfar) & (tmin <= prune)).sum())
                reached[code] = reached[node] & hit
                order.append(code)
    assert len(order) == child.shape[0], "every node has exactly one parent"
    return out, equalities


def _both_tests_agree(tree, o, inv, prunes):
    assert np.isfinite(o).all() and np.isfinite(inv).all() and (inv != 0).all()
    equalities = 0
    passing = 0
    for prune in prunes:
        today, eq = _passing_leaves(tree, o, inv, F(prune), strict=False)
        strict, _ = _passing_leaves(tree, o, inv, F(prune), strict=True)
        assert np.array_equal(today, strict), ("bestPrune", prune, "rays", np.nonzero((today != strict).any(axis=0))[0][:8])
        equalities += eq
        passing += int(today.sum())
    return equalities, passing


def test_cover_scene_random_rays(shim):  # noqa: F811
    words, spheres = _nodes(shim, rt.scenes.cover_scene())
    tree = _tree_of_words(words)
    lo, hi, child = tree
    assert np.all(lo <= hi)
    rng = np.random.default_rng(18)
    rays = 3000
    o = np.concatenate([rng.uniform(-12, 12, (rays // 2, 3)) * [1, 0.15, 1] + [0, 1.0, 0],                      # among the spheres
                        np.array([13.0, 2.0, 3.0]) + rng.normal(0, 0.5, (rays - rays // 2, 3))]).astype(F)      # around the camera
    d = rng.normal(0, 1, (rays, 3))
    d[:, 1] *= 0.3                                                                                              # mostly along the ground, where the spheres are
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    d[d == 0] = F(1e-3)
    inv = (F(1) / d).astype(F)
    _, passing = _both_tests_agree(tree, o, inv, [np.inf, 2.0, 8.0, 15.0])
    assert passing > rays, "the rays do find leaves"


def _grid_tree():
    """16 cubes of edge 2 on a 4 x 4 grid in the plane z in [0, 2] under a median-split tree; an inner child's box is the exact union of its subtree's boxes"""
    cubes = [((2 * i, 2 * j, 0), (2 * i + 2, 2 * j + 2, 2)) for i in range(4) for j in range(4)]
    lo, hi, child = [], [], []

    def box(ids):
        return (tuple(min(cubes[k][0][a] for k in ids) for a in range(3)), tuple(max(cubes[k][1][a] for k in ids) for a in range(3)))

    def build(ids, axis):
        """-> child code of this subtree"""
        if len(ids) == 1:
            return ~ids[0]
        me = len(child)
        lo.append(None), hi.append(None), child.append(None)
        ids = sorted(ids, key=lambda k: cubes[k][0][axis])
        halves = (ids[:len(ids) // 2], ids[len(ids) // 2:])
        boxes = [box(h) for h in halves]
        codes = [build(h, 1 - axis) for h in halves]
        lo[me], hi[me], child[me] = [b[0] for b in boxes], [b[1] for b in boxes], codes
        return me

    assert build(list(range(16)), 0) == 0
    return np.array(lo, F), np.array(hi, F), np.array(child, np.int32)


def test_exact_grid_tree_edges_and_corners():
    tree = _grid_tree()
    assert tree[2].shape == (15, 2)
    # integer origins around and inside the grid, inv components +-1/2, +-1, +-2: every difference and every product is exact in float32
    axis = np.arange(-3, 12, dtype=F)
    oz = np.array([-2, 0, 1, 2, 4], F)
    origins = np.stack(np.meshgrid(axis, axis, oz, indexing="ij"), -1).reshape(-1, 3)
    steps = np.array([-2, -1, -0.5, 0.5, 1, 2], F)
    invs = np.stack(np.meshgrid(steps, steps, steps, indexing="ij"), -1).reshape(-1, 3)
    o = np.repeat(origins, len(invs), axis=0)
    inv = np.tile(invs, (len(origins), 1))
    equalities, passing = _both_tests_agree(tree, o, inv, [np.inf, 1.0, 3.0, 4.0])
    print("rays", o.shape[0], "inner children met with tmin == tfar", equalities, "passing leaf tests", passing)
    assert equalities > 0, "the set must hold rays through edges and corners of inner boxes"
    assert passing > 0
