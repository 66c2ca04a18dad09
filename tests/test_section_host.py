"""Plane sections without a GPU: the brute-force shim (tests/section_oracle.c) that test_gpu_sections.py compares with is pinned on
hand-made cases with exact ends -- the half-open rule at vertices and edges, -0, zero and NaN planes, degenerate triangles -- on the
contour of a cube (closed, oriented, reversed by the normal and by a mirror), on posed instances against world copies and against
float64; the Python wrappers reject bad arguments before they touch a device."""
import numpy as np
import pytest

import scene_defs as sd
import section_oracle as sc
from test_crossing_host import _cube, _scene
from test_tri_intersect_host import _verts, _world_copy

F32 = np.float32
Z0 = [(0, 0, 0), (0, 0, 1)]                     # the plane z = 0, normal +z


def _pair(plane, tri, pose=(0.0,) * 6):
    hit, seg, h, _m = sc.pair(plane, tri, pose)
    return hit, seg.tolist(), h.tolist()


def test_straddling_triangle_has_exact_oriented_ends():
    tri = [(0, 0, -1), (2, 0, 1), (0, 2, 1)]
    hit, seg, h = _pair(Z0, tri)
    assert hit and h == [-1, 1, 1]
    assert seg == [[0, 1, 0], [1, 0, 0]]         # end 0 on C->A (ABOVE to BELOW), end 1 on A->B; along cross(n, face normal) = (4, -4, 0)
    # the other winding of the same triangle runs the other way, the reversed normal too; the points are the same
    assert _pair(Z0, [tri[0], tri[2], tri[1]])[1] == [[1, 0, 0], [0, 1, 0]]
    assert _pair([(0, 0, 0), (0, 0, -1)], tri)[1] == [[1, 0, 0], [0, 1, 0]]
    # N is not normalised: a scaled normal scales the heights and leaves the ends
    hit, seg, h = _pair([(0, 0, 0), (0, 0, 8)], tri)
    assert hit and h == [-8, 8, 8] and seg == [[0, 1, 0], [1, 0, 0]]
    # the plane's point may be anywhere in the plane; a cut away from the middle
    hit, seg, h = _pair([(16, -4, 0.5), (0, 0, 2)], tri)
    assert hit and h == [-3, 1, 1] and seg == [[0, 1.5, 0.5], [1.5, 0, 0.5]]


def test_triangle_in_the_plane_is_no_pair():
    hit, seg, h = _pair(Z0, [(0, 0, 0), (1, 0, 0), (0, 1, 0)])
    assert not hit and h == [0, 0, 0] and seg == [[0, 0, 0], [0, 0, 0]]


def test_vertex_on_the_plane_from_below_and_from_above():
    hit, seg, h = _pair(Z0, [(0, 0, 0), (1, 0, -1), (0, 1, -1)])
    assert hit and h == [0, -1, -1] and seg == [[0, 0, 0], [0, 0, 0]]        # a zero-length segment at the vertex
    for k in (1, 2):                                                        # whichever vertex of the cycle touches
        t = np.roll(np.array([(4, 8, 0), (1, 0, -1), (0, 1, -1)], F32), k, axis=0)
        hit, seg, _h = _pair(Z0, t)
        assert hit and seg == [[4, 8, 0], [4, 8, 0]]
    assert not _pair(Z0, [(0, 0, 0), (1, 0, 1), (0, 1, 1)])[0]


def test_edge_in_the_plane_with_the_third_vertex_below_and_above():
    hit, seg, h = _pair(Z0, [(0, 0, 0), (1, 0, 0), (0, 1, -1)])
    assert hit and h == [0, 0, -1] and seg == [[1, 0, 0], [0, 0, 0]]        # the edge itself, B -> A
    assert not _pair(Z0, [(0, 0, 0), (1, 0, 0), (0, 1, 1)])[0]


def test_negative_zero_height_is_above():
    """every term of step 4 is -0 at X = P under a normal with three negative components, so h = -0: ABOVE"""
    hit, seg, h = sc.pair([(0, 0, 0), (-1, -1, -1)], [(0, 0, 0), (1, 0, 0), (0, 1, 0)])[:3]
    assert h[0] == 0 and np.signbit(h[0]) and h[1] == -1 and h[2] == -1
    assert hit and seg.tolist() == [[0, 0, 0], [0, 0, 0]]


def test_zero_normal_and_nan_planes(orc):
    tri = [(0, 0, -1), (2, 0, 1), (0, 2, 1)]
    assert not _pair([(0, 0, 0), (0, 0, 0)], tri)[0] and not _pair([(0, 0, 0), (-0.0, 0, -0.0)], tri)[0]
    for bad in ([(np.nan, 0, 0), (0, 0, 1)], [(0, 0, 0), (0, np.nan, 1)], [(np.inf, 0, 0), (1, 0, 0)], np.full((2, 3), np.nan)):
        assert not _pair(bad, tri)[0]
    so = _scene(orc, _cube(orc))
    try:
        planes = np.array([[(.5, .5, .5), (0, 0, 1)], [(.5, .5, .5), (0, 0, 0)], np.full((2, 3), np.nan), [(.5, .5, 5), (0, 0, 1)]], F32)
        assert sc.count_sections(so, planes).tolist() == [8, 0, 0, 0]
        r = sc.list_sections(so, planes, max_hits=3)
        assert r["count"].tolist() == [8, 0, 0, 0] and (r["triangle"][1:] == -1).all() and (r["triangle"][0] >= 0).all()
        assert (r["segment"][1:] == 0).all() and (r["normal"][1:] == 0).all()
    finally:
        so.close()


def test_degenerate_triangles():
    """A point triangle has one class: never a pair.  A segment triangle that crosses is a pair with a zero-length segment where it
    crosses; one that lies in the plane or ends on it from above is none."""
    assert not _pair(Z0, [(1, 1, 0)] * 3)[0] and not _pair(Z0, [(1, 1, -1)] * 3)[0] and not _pair(Z0, [(1, 1, 1)] * 3)[0]
    hit, seg, _h = _pair(Z0, [(0, 0, -1), (0, 0, -1), (0, 0, 1)])
    assert hit and seg == [[0, 0, 0], [0, 0, 0]]
    hit, seg, _h = _pair(Z0, [(0, 0, -1), (4, 0, 3), (4, 0, 3)])
    assert hit and seg == [[1, 0, 0], [1, 0, 0]]
    assert not _pair(Z0, [(0, 0, 0), (1, 0, 0), (1, 0, 0)])[0] and not _pair(Z0, [(0, 0, 0), (0, 0, 1), (0, 0, 1)])[0]


def _chain(seg):
    """the segments [m, 2, 3] chained end 1 -> end 0 from segment 0 -> the order visited, or None when it is not one closed loop"""
    order, used = [0], {0}
    while True:
        nxt = [j for j in range(len(seg)) if np.array_equal(seg[j, 0], seg[order[-1], 1])]
        if len(nxt) != 1:
            return None
        if nxt[0] == 0:
            return order if len(order) == len(seg) else None
        if nxt[0] in used:
            return None
        order.append(nxt[0])
        used.add(nxt[0])


def _area(seg, order, normal):
    """the signed area of the loop seen from the side `normal` points to (> 0: counter-clockwise)"""
    p = seg[order, 0].astype(np.float64)
    return 0.5 * np.dot(np.cross(p, np.roll(p, -1, axis=0)).sum(0), np.asarray(normal, np.float64))


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_cube_contour_is_one_closed_counter_clockwise_loop(orc, axis):
    """The unit cube cut through its middle by an axis plane: 8 of 12 triangles; every end is exact (the cuts are at t = 1/2 of
    power-of-two edges), so the segments chain end 1 -> end 0 bit for bit into one loop of area 1, counter-clockwise seen from N;
    reversing N reverses it; so does a mirrored instance."""
    n = np.zeros(3, F32)
    n[axis] = 1
    mid = np.full(3, 0.5, F32)
    so = _scene(orc, _cube(orc))
    mirror = np.ones(3, F32)
    mirror[(axis + 1) % 3] = -1                                               # mirrored in an axis that lies in the plane
    sm = _scene(orc, _cube(orc), [(0, 0, (0.0,) * 6, tuple(float(x) for x in mirror))])
    try:
        r = sc.list_sections(so, np.array([[mid, n], [mid, -n]], F32))
        assert r["count"].tolist() == [8, 8]
        for j, (nn, want) in enumerate(((n, 1.0), (-n, 1.0))):
            seg = r["segment"][r["offsets"][j]:r["offsets"][j + 1]]
            assert (seg[:, :, axis] == 0.5).all()
            order = _chain(seg)
            assert order is not None, seg
            assert _area(seg, order, nn) == want                            # counter-clockwise seen from the plane's own normal
        assert sorted(r["triangle"][:8].tolist()) == r["triangle"][:8].tolist() and len(set(r["triangle"][:8].tolist())) == 8
        # end 0 -> end 1 runs along cross(N, face normal)
        a, b = r["offsets"][0], r["offsets"][1]
        d = r["segment"][a:b, 1] - r["segment"][a:b, 0]
        assert (np.einsum("ij,ij->i", d, np.cross(n, r["normal"][a:b])) > 0).all()
        m = sc.list_sections(sm, np.array([[mid * mirror, n]], F32))
        assert m["count"].tolist() == [8]
        order = _chain(m["segment"])
        assert order is not None and _area(m["segment"] - (mid * mirror), order, n) == -1.0        # clockwise: the mirror reverses it
    finally:
        so.close()
        sm.close()


def test_rooms_truncate_and_pad(orc):
    so = _scene(orc, _cube(orc))
    try:
        planes = np.array([[(.5, .5, .5), (0, 0, 1)], [(.5, .5, 2), (0, 0, 1)], [(.25, .5, .5), (1, 1, 0)]], F32)
        r = sc.list_sections(so, planes)
        assert r["count"].tolist()[:2] == [8, 0] and r["count"][2] > 0
        for K in (1, 3, 16):
            k = sc.list_sections(so, planes, max_hits=K)
            assert np.array_equal(k["count"], r["count"])
            for j in range(len(planes)):
                a, b = r["offsets"][j], r["offsets"][j + 1]
                m = min(b - a, K)
                for f in sc.FIELDS:
                    assert np.array_equal(k[f][j, :m], r[f][a:a + m]), (K, j, f)
                assert (k["instance"][j, m:] == -1).all() and (k["triangle"][j, m:] == -1).all()
                assert (k["segment"][j, m:] == 0).all() and (k["normal"][j, m:] == 0).all()
    finally:
        so.close()


@pytest.mark.parametrize("pose,scale", [((0.3, -0.2, 0.5, 0.4, -0.3, 0.2), (1.5, 0.7, 1.2)),
                                        ((-0.1, 0.4, 0.0, -0.6, 0.1, 0.9), (1.0, -1.3, 0.8))])
def test_posed_scaled_mirrored_instance_matches_world_copy(orc, pose, scale):
    """A posed, non-uniformly scaled (and mirrored) instance of a mesh and the same triangles placed in world space as an identity
    instance: the same pairs wherever every float64 world height is clear of the plane (1e-4 of |N|_1 times the largest coordinate),
    and the same world segment ends as far as the cut is conditioned (coordinates are within 3), in the same order: the mirror
    reverses the world triangle and the segment with it, in both scenes alike."""
    tris = sd.random_triangles(60, seed=3, spread=1.0, size=0.4)
    a = _scene(orc, tris, [(0, 0, tuple(pose), tuple(scale))])
    b = _scene(orc, _world_copy(orc, tris, pose, scale))
    try:
        world = _verts(orc, _world_copy(orc, tris, pose, scale)).astype(np.float64)
        rng = np.random.default_rng(9)
        planes = np.stack([rng.uniform(-1.2, 1.2, (300, 3)), rng.normal(size=(300, 3))], axis=1).astype(F32)
        ra, rb = sc.list_sections(a, planes), sc.list_sections(b, planes)
        P, N = planes[:, 0].astype(np.float64), planes[:, 1].astype(np.float64)
        h = np.einsum("jc,jtvc->jtv", N, world[None] - P[:, None, None, :])         # [planes, triangles, vertices]
        clear = (np.abs(h) > 1e-4 * np.abs(N).sum(1)[:, None, None] * 3.0).all(2)
        want = (h >= 0).any(2) & (h < 0).any(2)
        assert clear.mean() > 0.95
        both = 0
        for j in range(len(planes)):
            segs = []
            for r in (ra, rb):
                s0, s1 = r["offsets"][j], r["offsets"][j + 1]
                got = np.zeros(len(world), bool)
                got[r["triangle"][s0:s1]] = True
                assert np.array_equal(got[clear[j]], want[j][clear[j]]), j
                segs.append(dict(zip(r["triangle"][s0:s1].tolist(), r["segment"][s0:s1])))
                # every end lies in the world plane
                hs = np.einsum("c,tec->te", N[j], r["segment"][s0:s1].astype(np.float64) - P[j])
                assert (np.abs(hs) <= 1e-5 * np.abs(N[j]).sum()).all(), j
            for t in set(segs[0]) & set(segs[1]):
                if clear[j][t]:
                    # both ends lie within 1e-5 |N|_1 of the plane in height (just asserted) and on the same edge to rounding, so
                    # along an edge of unit direction e they differ by at most 2e-5 |N|_1 / |N.e|: the cut's own conditioning
                    e = world[t] - np.roll(world[t], -1, axis=0)
                    cross = (h[j, t] >= 0) != (np.roll(h[j, t], -1) >= 0)
                    ne = np.abs(e @ N[j])[cross] / np.linalg.norm(e, axis=1)[cross]
                    tol = 2e-5 * np.abs(N[j]).sum() / ne.min() + 1e-5
                    assert np.abs(segs[0][t] - segs[1][t]).max() <= tol, (j, t)
                    both += 1
        assert both > 100
    finally:
        a.close()
        b.close()


def test_agrees_with_float64(orc):
    """20 000 random posed planes against random triangles (coordinates within +-5, normals from 1e-3 to 1e3 long).  With p' and n'
    as the shim mapped them, in float64: the pair decision is the float64 one wherever every |height| exceeds 1e-4 of |n'|_1 times
    the largest coordinate magnitude (fp32 error there is below 1e-6 of it), and each cut point Q satisfies |H64(Q)| <= 2^-19 |n'|_1 M
    with M the largest magnitude among the coordinates of X, Y, X - p', Y - p' of its edge: 32u, where step 4's rounding of both
    heights (4u each, of which t passes on at most the larger), the division (2u) and the three roundings of Q (5u) come to 11u."""
    rng = np.random.default_rng(12)
    n = 20000
    pose = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.uniform(-np.pi, np.pi, (n, 3))], axis=1).astype(F32)
    plane = np.stack([rng.uniform(-5, 5, (n, 3)), rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))], axis=1).astype(F32)
    tri = np.zeros((n, 3, 3), F32)
    got = np.zeros(n, bool)
    seg = np.zeros((n, 2, 3), F32)
    mapped = np.zeros((n, 2, 3), F32)
    h32 = np.zeros((n, 3), F32)
    for j in range(n):
        # the triangle near p' in mesh space: its centre within a few sizes of the plane's point
        m = sc.pair(plane[j], np.zeros((3, 3), F32), pose[j])[3]
        size = 10.0 ** rng.uniform(-2, 0.5)
        t = m[0].astype(np.float64) + rng.normal(size=3) * size * rng.uniform(0, 1.5) + rng.normal(size=(3, 3)) * size
        tri[j] = np.clip(t, -8, 8).astype(F32)
        got[j], seg[j], h32[j], mapped[j] = sc.pair(plane[j], tri[j], pose[j])
    p64, n64, t64 = mapped[:, 0].astype(np.float64), mapped[:, 1].astype(np.float64), tri.astype(np.float64)
    h64 = np.einsum("jc,jvc->jv", n64, t64 - p64[:, None, :])
    n1 = np.abs(n64).sum(1)
    mag = np.maximum(np.abs(t64).max((1, 2)), np.abs(p64).max(1))
    clear = (np.abs(h64) > 1e-4 * (n1 * mag)[:, None]).all(1)
    want = (h64 >= 0).any(1) & (h64 < 0).any(1)
    assert clear.sum() >= 0.9 * n, clear.sum()
    assert np.array_equal(got[clear], want[clear]), np.flatnonzero(clear & (got != want))[:10]
    assert 0.2 * n < got.sum() < 0.9 * n, got.sum()                  # (both verdicts, thousands of each)
    # the cut points, on the edges the fp32 classes name
    worst = 0.0
    for j in np.flatnonzero(got):
        above = h32[j] >= 0
        for k in range(3):
            m = (k + 1) % 3
            if above[k] == above[m]:
                continue
            q = seg[j, 0 if above[k] else 1].astype(np.float64)
            x, y = t64[j, k], t64[j, m]
            M = max(np.abs(x).max(), np.abs(y).max(), np.abs(x - p64[j]).max(), np.abs(y - p64[j]).max())
            hq = abs(np.dot(n64[j], q - p64[j]))
            worst = max(worst, hq / (n1[j] * M))
            assert hq <= 2.0 ** -19 * n1[j] * M, (j, k, hq / (n1[j] * M))
    print("largest |H64(Q)| / (|n'|_1 M): %.3g (bound %.3g)" % (worst, 2.0 ** -19))


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    b = np.zeros((10, 2, 3), F32)
    calls = (lambda a: s.count_sections(a), lambda a: s.list_sections(a), lambda a: s.list_sections(a, max_hits=2))
    for bad in (b.astype(np.float64), np.zeros((10, 3), F32), np.zeros((10, 3, 3), F32), np.zeros((3, 2, 10), F32).transpose(2, 1, 0),
                b.reshape(-1), b.tolist()):
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    for m in (0, -1, 2.0, True, "3", 2 ** 31):
        with pytest.raises(ValueError):
            s.list_sections(b, max_hits=m)
    for outs in ((), ("t",), ("occupied",), ("normal",), ("segment",)):
        with pytest.raises(ValueError):
            s.count_sections(b, outputs=outs)
    for outs in ((), ("count",), ("count", "pops"), ("any",), ("instance", "point"), ("instance", "instance")):
        with pytest.raises(ValueError):
            s.list_sections(b, outputs=outs)
    assert not touched
    assert rt.Scene.SECTION_COUNT_OUTPUTS == ("count", "any", "pops")
    assert rt.Scene.SECTION_LIST_OUTPUTS == ("instance", "triangle", "segment", "normal")
    s.close()
