"""Box queries without a GPU: the brute-force shim (tests/box_oracle.c) that test_gpu_boxes.py compares with is pinned on hand-made
cases -- containment either way, the diagonal near-miss, shared faces and corners, flat / line / point boxes, invalid boxes, degenerate
triangles, instance poses -- and against an independent float64 separating-axis test; the Python wrappers reject bad arguments before
they touch a device."""
import numpy as np
import pytest

import box_oracle as bo
import scene_defs as sd
from test_crossing_host import _cube, _mesh, _scene
from test_tri_intersect_host import _verts, _world_copy

F32 = np.float32
UNIT = np.array([(0, 0, 0), (1, 1, 1)], F32)


def _sat64(corners, tri):
    """float64 separating axes of a box given by its eight corners (k's bit a set = hi on axis a) and a triangle, vectorised over
    leading dimensions: corners [..., 8, 3], tri [..., 3, 3] -> the largest gap over the normalised axes (three box edges, the triangle's
    normal, nine cross products; > 0 disjoint by at least that, < 0 overlapping by that on every axis).  Axes shorter than 1e-12 are
    left out."""
    c, t = np.asarray(corners, np.float64), np.asarray(tri, np.float64)
    e = [c[..., 1, :] - c[..., 0, :], c[..., 2, :] - c[..., 0, :], c[..., 4, :] - c[..., 0, :]]
    f = [t[..., 1, :] - t[..., 0, :], t[..., 2, :] - t[..., 1, :], t[..., 0, :] - t[..., 2, :]]
    axes = e + [np.cross(f[0], f[1])] + [np.cross(u, v) for u in e for v in f]
    best = np.full(c.shape[:-2], -np.inf)
    for ax in axes:
        n = np.linalg.norm(ax, axis=-1)
        ok = n > 1e-12
        ax = ax / np.where(ok, n, 1.0)[..., None]
        pb, pt = (c * ax[..., None, :]).sum(-1), (t * ax[..., None, :]).sum(-1)
        gap = np.maximum(pt.min(-1) - pb.max(-1), pb.min(-1) - pt.max(-1))
        best = np.where(ok, np.maximum(best, gap), best)
    return best


def test_triangle_wholly_inside_a_box_and_far_outside():
    inside = [(.2, .2, .2), (.4, .2, .3), (.3, .5, .4)]
    assert bo.pair(UNIT, inside) == (True, "pair")
    assert bo.pair(UNIT, np.asarray(inside, F32) + F32(2)) == (False, "boxes")
    assert bo.pair(UNIT + F32(100), np.asarray(inside, F32) + F32(100)) == (True, "pair")


def test_box_inside_a_large_triangle_passes_on_the_normal_alone():
    """A small box in the interior of a large tilted triangle: the triangle's box contains the query's and every edge axis overlaps,
    so only N could separate.  With the plane through the box it is a pair; with the plane lifted off it, N separates."""
    n = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    u = np.cross(n, [0, 0, 1.0])
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    centre = np.array([.5, .5, .5])
    tri = np.array([centre + 50 * u, centre - 25 * u + 43 * v, centre - 25 * u - 43 * v])
    assert bo.pair(UNIT, tri.astype(F32)) == (True, "pair")
    assert bo.pair(UNIT, (tri + 2.0 * n).astype(F32)) == (False, "N")
    assert bo.pair(UNIT, (tri - 2.0 * n).astype(F32)) == (False, "N")


def test_diagonal_near_miss_is_separated_by_a_cross_axis():
    """A triangle in z = 0.5 that cuts the corner region beyond (1, 1): its box overlaps the unit box, the box's edges and the normal
    do not separate, Ez x F0 (the direction (1, 1, 0)) does.  Moved in by 0.2 it is a pair."""
    tri = np.array([(1.6, .5, .5), (.5, 1.6, .5), (1.6, 1.6, .5)], F32)
    assert bo.pair(UNIT, tri) == (False, "EzxF0")
    assert bo.pair(UNIT, tri - np.array([.2, .2, 0], F32)) == (True, "pair")


def test_triangle_in_the_face_two_cells_share_is_reported_by_both():
    """Identity pose: the cells [0, 1]^3 and [1, 2] x [0, 1]^2 share the face x = 1 bit for bit; a triangle lying in it touches both
    (the test is closed).  Through the scene form too, where the cells come from the grid formula."""
    tri = np.array([(1, .2, .2), (1, .8, .3), (1, .4, .9)], F32)
    right = UNIT + np.array([1, 0, 0], F32)
    assert bo.pair(UNIT, tri)[0] and bo.pair(right, tri)[0]
    assert bo.pair(UNIT + np.array([2, 0, 0], F32), tri) == (False, "boxes")


def test_shared_face_through_a_scene_and_the_grid_formula(orc):
    so = _scene(orc, _mesh(orc, [(1, .2, .2), (1, .8, .3), (1, .4, .9)], [(0, 1, 2)]))
    try:
        cells = bo.grid_boxes((0, 0, 0), (1, 1, 1), (3, 1, 1))
        assert np.array_equal(cells[0, 0, 0, 1], cells[0, 0, 1, 0] * [1, 0, 0] + cells[0, 0, 0, 1] * [0, 1, 1])
        assert bo.count_in_boxes(so, cells).tolist() == [1, 1, 0]
        # a spacing that is not representable: cell i's hi and cell i + 1's lo are the same float
        g = bo.grid_boxes((0.1, 0.2, 0.3), (0.1, 0.1, 0.1), (9, 7, 5))
        assert np.array_equal(g[:, :, :-1, 1, 0], g[:, :, 1:, 0, 0]) and np.array_equal(g[:, :-1, :, 1, 1], g[:, 1:, :, 0, 1])
        assert np.array_equal(g[:-1, :, :, 1, 2], g[1:, :, :, 0, 2])
        assert g[0, 0, 3, 0, 0] == F32(0.1) + F32(3) * F32(0.1)
    finally:
        so.close()


def test_grid_cells_are_grid_boxes_at_flat_indices():
    """the helper for grids too large to make whole: any subset of cells, in any order, and the last index of a 2^24 axis"""
    o, s, dims = (0.1, 0.2, 0.3), (0.1, 0.13, 0.17), (9, 7, 5)
    g = bo.grid_boxes(o, s, dims).reshape(-1, 2, 3)
    idx = np.random.default_rng(5).permutation(len(g))[:100]
    assert np.array_equal(bo.grid_cells(o, s, dims, np.arange(len(g))), g) and np.array_equal(bo.grid_cells(o, s, dims, idx), g[idx])
    last = bo.grid_cells((-1, 0, 0), (1.2e-7, 1, 1), (2 ** 24, 1, 1), [2 ** 24 - 1])[0]
    assert last[0, 0] == F32(-1) + F32(2 ** 24 - 1) * F32(1.2e-7) and last[1, 0] == F32(-1) + F32(2 ** 24) * F32(1.2e-7)
    assert last.dtype == F32 and last[:, 1].tolist() == [0, 1]


def test_vertex_exactly_on_a_corner():
    tri = np.array([(1, 1, 1), (2, 1.5, 1.2), (1.5, 2, 1.7)], F32)
    assert bo.pair(UNIT, tri) == (True, "pair")
    assert not bo.pair(UNIT, tri + np.array([1e-6, 0, 0], F32))[0]


def test_flat_line_and_point_boxes():
    tri = np.array([(0, 0, .5), (1, 0, .5), (0, 1, .5)], F32)
    flat_on = np.array([(.1, .1, .5), (.3, .3, .5)], F32)          # a flat box in the triangle's plane
    flat_across = np.array([(.2, .1, .2), (.2, .3, .8)], F32)      # a flat box across it
    flat_off = np.array([(.1, .1, .6), (.3, .3, .6)], F32)
    assert bo.pair(flat_on, tri)[0] and bo.pair(flat_across, tri)[0] and not bo.pair(flat_off, tri)[0]
    line_through = np.array([(.2, .2, 0), (.2, .2, 1)], F32)
    line_beside = np.array([(.8, .8, 0), (.8, .8, 1)], F32)
    assert bo.pair(line_through, tri)[0] and not bo.pair(line_beside, tri)[0]
    point_on = np.array([(.25, .25, .5)] * 2, F32)
    point_off = np.array([(.25, .25, .75)] * 2, F32)
    point_vertex = np.array([(1, 0, .5)] * 2, F32)
    assert bo.pair(point_on, tri)[0] and bo.pair(point_vertex, tri)[0] and not bo.pair(point_off, tri)[0]


def test_inverted_and_nan_boxes_give_no_pairs(orc):
    tri = [(.2, .2, .2), (.4, .2, .3), (.3, .5, .4)]
    for a in range(3):
        b = UNIT.copy()
        b[0, a], b[1, a] = 1, 0
        assert bo.pair(b, tri) == (False, "invalid")
        for row in (0, 1):
            b = UNIT.copy()
            b[row, a] = np.nan
            assert bo.pair(b, tri) == (False, "invalid")
    so = _scene(orc, _cube(orc))
    try:
        boxes = np.stack([UNIT, UNIT[::-1], np.full((2, 3), np.nan, F32), UNIT * [1, np.nan, 1]]).astype(F32)
        assert bo.count_in_boxes(so, boxes).tolist() == [12, 0, 0, 0]
        r = bo.list_in_boxes(so, boxes, max_hits=3)
        assert r["triangle"].tolist() == [[0, 1, 2], [-1] * 3, [-1] * 3, [-1] * 3] and r["count"].tolist() == [12, 0, 0, 0]
    finally:
        so.close()


def test_degenerate_triangles():
    """A triangle that is a point or a segment has zero axes among its thirteen (they never separate); it is a pair exactly when the
    point or the segment meets the box."""
    assert bo.pair(UNIT, [(.5, .5, .5)] * 3)[0] and bo.pair(UNIT, [(1, 1, 1)] * 3)[0]
    assert not bo.pair(UNIT, [(1.5, .5, .5)] * 3)[0]
    assert bo.pair(UNIT, [(-1, .5, .5), (-1, .5, .5), (2, .5, .5)])[0]
    assert not bo.pair(UNIT, [(-1, 1.5, .5), (-1, 1.5, .5), (2, 1.5, .5)])[0]
    assert bo.pair(UNIT, [(1.6, .5, .5), (.5, 1.6, .5), (1.6, .5, .5)]) == (False, "EzxF0")    # a segment past the corner


def test_cube_scene_counts_and_lists(orc):
    so = _scene(orc, _cube(orc))
    try:
        boxes = np.array([[(-1, -1, -1), (2, 2, 2)], [(.25, .25, .25), (.75, .75, .75)], [(.9, .4, .4), (1.1, .6, .6)],
                          [(.9, .9, .9), (1.1, 1.1, 1.1)], [(3, 3, 3), (4, 4, 4)]], F32)
        r = bo.list_in_boxes(so, boxes)
        assert r["count"].tolist()[:2] == [12, 0] and r["count"][4] == 0
        assert 1 <= r["count"][2] <= 2 and r["count"][3] >= 3
        for j in range(len(boxes)):
            t = r["triangle"][r["offsets"][j]:r["offsets"][j + 1]]
            assert sorted(t.tolist()) == t.tolist() and (r["instance"][r["offsets"][j]:r["offsets"][j + 1]] == 0).all()
        for K in (1, 2, 16):
            k = bo.list_in_boxes(so, boxes, max_hits=K)
            for j in range(len(boxes)):
                a, b = r["offsets"][j], r["offsets"][j + 1]
                m = min(b - a, K)
                assert np.array_equal(k["triangle"][j, :m], r["triangle"][a:a + m]) and (k["triangle"][j, m:] == -1).all()
                assert (k["instance"][j, m:] == -1).all()
            assert np.array_equal(k["count"], r["count"])
    finally:
        so.close()


def test_agrees_with_float64_separating_axes(orc):
    """20 000 random posed boxes (edges 1e-3 to 3, coordinates within +-5) against random triangles: wherever the float64 separation or
    penetration exceeds 1e-4 of the largest coordinate magnitude the shim's verdict is the float64 one; at most 5 % are left out."""
    rng = np.random.default_rng(11)
    n = 20000
    edge = 10.0 ** rng.uniform(-3, np.log10(3.0), (n, 3))
    lo = rng.uniform(-5, 5 - edge)
    box = np.stack([lo, lo + edge], axis=1).astype(F32)
    pose = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.uniform(-np.pi, np.pi, (n, 3))], axis=1).astype(F32)
    corners = np.stack([bo.corners(b, p) for b, p in zip(box, pose)])
    centre = corners.astype(np.float64).mean(1)
    size = np.linalg.norm(edge, axis=1)[:, None, None] * 10.0 ** rng.uniform(-1, 0.5, (n, 1, 1))
    reach = np.linalg.norm(edge, axis=1)[:, None, None] / 2 + size     # the triangle's centre: within about that of the box's
    tri = centre[:, None, :] + rng.normal(size=(n, 1, 3)) / np.sqrt(3.0) * reach * rng.uniform(0, 0.8, (n, 1, 1)) \
        + rng.normal(size=(n, 3, 3)) * size
    tri = np.clip(tri, -5, 5).astype(F32)
    gap = _sat64(corners, tri)
    mag = np.maximum(np.abs(corners).max((1, 2)), np.abs(tri).max((1, 2)))
    clear = np.abs(gap) > 1e-4 * mag
    got = np.array([bo.pair(b, t, p)[0] for b, t, p in zip(box, tri, pose)])
    assert clear.sum() >= 0.95 * n, clear.sum()
    assert np.array_equal(got[clear], gap[clear] < 0), np.flatnonzero(clear & (got != (gap < 0)))[:10]
    assert 0.1 * n < got.sum() < 0.9 * n, got.sum()                  # (both verdicts, thousands of each)


@pytest.mark.parametrize("pose,scale", [((0.3, -0.2, 0.5, 0.4, -0.3, 0.2), (1.5, 0.7, 1.2)),
                                        ((-0.1, 0.4, 0.0, -0.6, 0.1, 0.9), (1.0, -1.3, 0.8))])
def test_posed_scaled_mirrored_instance_matches_world_copy(orc, pose, scale):
    """A posed, non-uniformly scaled (and mirrored) instance of a mesh and the same triangles placed in world space as an identity
    instance give the same pairs wherever the float64 separation in world space is clear."""
    tris = sd.random_triangles(60, seed=3, spread=1.0, size=0.4)
    a = _scene(orc, tris, [(0, 0, tuple(pose), tuple(scale))])
    b = _scene(orc, _world_copy(orc, tris, pose, scale))
    try:
        world = _verts(orc, _world_copy(orc, tris, pose, scale))
        rng = np.random.default_rng(9)
        lo = rng.uniform(-1.3, 0.9, (300, 3))
        boxes = np.stack([lo, lo + rng.uniform(0.02, 0.8, (300, 3))], axis=1).astype(F32)
        ra, rb = bo.list_in_boxes(a, boxes), bo.list_in_boxes(b, boxes)
        corners = np.stack([bo.corners(x) for x in boxes])
        gap = _sat64(corners[:, None], world[None])                   # [boxes, triangles]
        clear = np.abs(gap) > 1e-4 * 3.0
        assert clear.mean() > 0.95
        for j in range(len(boxes)):
            for r in (ra, rb):
                got = np.zeros(len(world), bool)
                got[r["triangle"][r["offsets"][j]:r["offsets"][j + 1]]] = True
                assert np.array_equal(got[clear[j]], gap[j][clear[j]] < 0), j
        assert ra["count"].sum() > 100
    finally:
        a.close()
        b.close()


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    b = np.zeros((10, 2, 3), F32)
    calls = (lambda a: s.count_in_boxes(a), lambda a: s.list_in_boxes(a), lambda a: s.list_in_boxes(a, max_hits=2))
    for bad in (b.astype(np.float64), np.zeros((10, 3), F32), np.zeros((10, 3, 3), F32), np.zeros((3, 2, 10), F32).transpose(2, 1, 0),
                b.reshape(-1), b.tolist()):
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    for m in (0, -1, 2.0, True, "3", 2 ** 31):
        with pytest.raises(ValueError):
            s.list_in_boxes(b, max_hits=m)
    for outs in ((), ("t",), ("occupied",), ("normal",)):
        with pytest.raises(ValueError):
            s.count_in_boxes(b, outputs=outs)
    for outs in ((), ("count",), ("count", "pops"), ("any",), ("instance", "normal"), ("instance", "instance")):
        with pytest.raises(ValueError):
            s.list_in_boxes(b, outputs=outs)
    for args in (((0, 0), (1, 1, 1), (2, 2, 2)), ((0, 0, 0), (1, 1), (2, 2, 2)), ((0, 0, 0), (1, 1, 1), (2, 2)),
                 ((0, 0, 0), (1, 1, 1), (2.0, 2.0, 2.0)), ((0, 0, 0), (1, 1, 1), (-1, 2, 2)), ((0, 0, 0), (1, 1, 1), (2 ** 24 + 1, 1, 1)),
                 ((0, 0, 0), (1, 1, 1), (2 ** 11, 2 ** 10, 2 ** 10))):
        with pytest.raises(ValueError):
            s.occupancy_grid(*args, as_numpy=True)
    for outs in ((), ("any",), ("pops",)):
        with pytest.raises(ValueError):
            s.occupancy_grid((0, 0, 0), (1, 1, 1), (2, 2, 2), outputs=outs, as_numpy=True)
    assert not touched
    assert rt.Scene.BOX_COUNT_OUTPUTS == ("count", "any", "pops") and rt.Scene.BOX_LIST_OUTPUTS == ("instance", "triangle")
    s.close()
