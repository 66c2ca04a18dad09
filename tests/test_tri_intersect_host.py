"""Triangle intersection queries without a GPU: the brute-force shim (tests/tri_intersect_oracle.c) that test_gpu_tri_intersect.py
compares with is pinned on hand-made contacts, degenerate and underflowing cases, instance poses and skip_instance, and against an
independent float64 separating-axis test; the C-ABI and the Python wrappers reject bad arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import scene_defs as sd
import tri_intersect_oracle as ti
from test_crossing_host import _cube, _mesh, _scene

F32 = np.float32
ID = (0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))


def _verts(orc, tris18):
    """world vertices [m, 3, 3] of oracle triangle records"""
    return np.asarray(tris18, F32)[:, :9].reshape(-1, 3, 3)


def _sat64(a, b):
    """float64 separating-axis test of two triangles [3, 3] -> the largest normalised gap over the face normals and the nine edge
    cross products (> 0: disjoint, < 0: intersecting; generic, non-coplanar pairs only)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ea = [a[1] - a[0], a[2] - a[1], a[0] - a[2]]
    eb = [b[1] - b[0], b[2] - b[1], b[0] - b[2]]
    axes = [np.cross(ea[0], ea[1]), np.cross(eb[0], eb[1])] + [np.cross(u, v) for u in ea for v in eb]
    best = -np.inf
    for ax in axes:
        n = np.linalg.norm(ax)
        if n < 1e-12:
            continue
        pa, pb = a @ (ax / n), b @ (ax / n)
        best = max(best, pa.min() - pb.max(), pb.min() - pa.max())
    return best


def test_crossing_pair_segment_is_the_analytic_intersection():
    """A vertical triangle through a horizontal one: the scene triangle's edges A->B and C->A cross the query's plane inside it, so
    the segment runs from the first (test 3) to the last (test 5) crossing point, the analytic intersection to 1e-6."""
    q = np.array([(-1, -1, 0), (2, -1, 0), (-1, 2, 0)], F32)
    t = np.array([(0.25, 0, -1), (0.25, 0.5, 1), (0.25, -0.5, 1)], F32)
    hit, seg = ti.pair(q, t)
    assert hit
    assert np.allclose(seg, [(0.25, 0.25, 0), (0.25, -0.25, 0)], atol=1e-6)
    hit2, seg2 = ti.pair(t, q)                                  # swapped roles: the query's edges now do the crossing
    assert hit2 and np.allclose(seg2, seg, atol=1e-6)


def test_disjoint_with_overlapping_boxes():
    q = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F32)
    t = np.array([(0.9, 0.9, -0.5), (0.9, 0.9, 0.5), (1.0, 0.8, 0.0)], F32)
    assert (t.min(0) <= q.max(0)).all() and (q.min(0) <= t.max(0)).all()
    assert not ti.pair(q, t)[0] and not ti.pair(t, q)[0]


def test_touching_at_a_vertex_and_an_edge_and_a_t_junction():
    """Closed tests: a vertex of one triangle on the other's face, two triangles sharing a vertex, sharing an edge, and an edge lying
    on the other's face (T-junction) are all pairs; the vertex contact's segment is that vertex at both ends."""
    q = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F32)
    hit, seg = ti.pair(q, np.array([(0.2, 0.2, 0), (0.2, 0.2, 1), (0.3, 0.2, 1)], F32))
    assert hit and np.array_equal(seg, np.array([(0.2, 0.2, 0), (0.2, 0.2, 0)], F32))
    assert ti.pair(q, np.array([(0, 0, 0), (0, 0, 1), (-1, 0, 1)], F32))[0]          # a shared vertex
    assert ti.pair(q, np.array([(0, 0, 0), (1, 0, 0), (0.5, 0, 1)], F32))[0]         # a shared edge
    assert ti.pair(q, np.array([(0.2, 0.2, 0), (0.6, 0.2, 0), (0.4, 0.2, 1)], F32))[0]   # T-junction


def test_piercing_and_enclosed_triangles_against_a_cube(orc):
    so = _scene(orc, _cube(orc))
    try:
        needle = np.array([[(0.30, 0.40, -0.5), (0.31, 0.41, 1.5), (0.32, 0.40, 1.5)]], F32)
        inside = np.array([[(0.4, 0.4, 0.4), (0.6, 0.4, 0.5), (0.5, 0.6, 0.6)]], F32)
        r = ti.list_intersecting(so, np.concatenate([needle, inside]))
        assert r["count"].tolist() == [2, 0]
        assert sorted(r["triangle"].tolist()) == r["triangle"].tolist()
        z = r["segment"][:, :, 2]
        assert sorted(np.round(z.mean(1)).tolist()) == [0.0, 1.0]         # one contact on the bottom face, one on the top
    finally:
        so.close()


def test_cubes_face_to_face_report_a_contact(orc):
    """A second unit cube placed against the first's x = 1 face: its triangles report contacts through the side faces whose edges
    end on the shared plane."""
    cube = _cube(orc)
    so = _scene(orc, cube)
    try:
        other = _verts(orc, cube) + np.array([1.0, 0.0, 0.0], F32)
        c = ti.count_intersecting(so, other)
        assert c.sum() > 0
    finally:
        so.close()


def test_coplanar_pair_is_rounding_dependent():
    """Coplanar overlap rests on rounding in the sheared coordinates (rule 10's note).  These two overlapping triangles in z = 0 are
    not reported, in either role; the same pair lifted off the plane by a tilt is."""
    q = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F32)
    t = np.array([(0.2, 0.2, 0), (0.8, 0.2, 0), (0.2, 0.8, 0)], F32)
    assert not ti.pair(q, t)[0] and not ti.pair(t, q)[0]
    tilt = t.copy()
    tilt[:, 2] = [-0.1, 0.1, 0.1]
    assert ti.pair(q, tilt)[0]


def test_zero_length_edges_and_degenerate_queries():
    """A query that is a point counts nothing (every d' is zero and the scene edges meet a degenerate triangle with det = 0); one
    that is a segment (two equal vertices) still crosses through its nonzero edges."""
    t = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], F32)
    point = np.array([(0.2, 0.2, 0)] * 3, F32)
    assert not ti.pair(point, t)[0]
    seg = np.array([(0.2, 0.2, -1), (0.2, 0.2, -1), (0.3, 0.2, 1)], F32)
    hit, s = ti.pair(seg, t)
    assert hit and np.allclose(s[0], (0.25, 0.2, 0), atol=1e-6)
    flat = np.array([(0, 0, 0), (0, 0, 0), (0, 0, 0)], F32)
    assert not ti.pair(flat, flat)[0]


def test_underflowed_edge_test_counts_but_the_box_rejects():
    """Rule 10 step 3 is part of the pair rule.  A tiny scene triangle at z = 1.4 around the z axis: the query edge (0,0,0)->(0,0,1)
    stops short of it, but its U, V, W underflow to +-2^-149 in the fp64 fallback and U*az rounds to 2^-149, so the segment test
    counts at t = 1.  The boxes do not overlap (z <= 1 against z = 1.4), so the pair is not reported."""
    e = F32(1e-25)
    t = np.array([(e, 0, 1.4), (-e, e, 1.4), (-e, -e, 1.4)], F32)
    counted, tt = ti.segment((0, 0, 0), (0, 0, 1), t)
    assert counted and tt == 1.0
    q = np.array([(0, 0, 0), (0, 0, 1), (1, 0, 0.5)], F32)
    assert not ti.pair(q, t)[0]


def test_agrees_with_float64_separating_axes():
    """4000 random pairs: wherever the float64 separation is clearly nonzero (beyond 1e-4 of the triangles' size), the shim's pair
    is exactly the separating-axis verdict."""
    rng = np.random.default_rng(5)
    checked = agree = hits = 0
    for _ in range(4000):
        a = rng.uniform(-1, 1, (3, 3)).astype(F32)
        b = (rng.uniform(-0.5, 0.5, 3) + rng.uniform(-1, 1, (3, 3))).astype(F32)
        g = _sat64(a, b)
        if abs(g) < 1e-4:
            continue
        checked += 1
        hit = ti.pair(a, b)[0]
        hits += hit
        agree += hit == (g < 0)
    assert checked > 3500 and agree == checked and 0.2 * checked < hits < 0.8 * checked, (checked, agree, hits)


def _world_copy(orc, tris, pose, scale):
    """the mesh's triangles placed in world space by (pose, scale) as oracle triangle records"""
    o = orc.oracle()
    inv = o.invert_lre(np.asarray(pose, F32))
    v = _verts(orc, tris).reshape(-1, 3) * np.asarray(scale, F32)
    w = np.stack([o.apply_lre(inv, x.astype(F32)) for x in v]).astype(F32).reshape(-1, 3, 3)
    return np.stack([np.asarray(o.tri_from_vertices(x.ravel()), F32) for x in w])


@pytest.mark.parametrize("pose,scale", [((0.3, -0.2, 0.5, 0.4, -0.3, 0.2), (1.5, 0.7, 1.2)),
                                        ((-0.1, 0.4, 0.0, -0.6, 0.1, 0.9), (1.0, -1.3, 0.8))])
def test_posed_scaled_mirrored_instance_matches_world_copy(orc, pose, scale):
    """A posed, non-uniformly scaled (and mirrored) instance of a mesh and the same triangles placed in world space as an identity
    instance give the same pairs wherever the float64 separation is clear; the mirrored case flips no pair."""
    tris = sd.random_triangles(60, seed=3, spread=1.0, size=0.4)
    a = _scene(orc, tris, [(0, 0, tuple(pose), tuple(scale))])
    b = _scene(orc, _world_copy(orc, tris, pose, scale))
    try:
        world = _verts(orc, _world_copy(orc, tris, pose, scale))
        rng = np.random.default_rng(9)
        q = (rng.uniform(-1.5, 1.5, (300, 1, 3)) + rng.uniform(-0.3, 0.3, (300, 3, 3))).astype(F32)
        ra, rb = ti.list_intersecting(a, q), ti.list_intersecting(b, q)
        clear = 0
        for j in range(len(q)):
            ga = set(ra["triangle"][ra["offsets"][j]:ra["offsets"][j + 1]].tolist())
            gb = set(rb["triangle"][rb["offsets"][j]:rb["offsets"][j + 1]].tolist())
            for k in range(len(world)):
                g = _sat64(q[j], world[k])
                if abs(g) < 1e-4:
                    continue
                clear += 1
                assert (k in ga) == (g < 0) == (k in gb), (j, k, g)
        assert clear > 0.99 * len(q) * len(world) * 0.9
    finally:
        a.close()
        b.close()


def test_skip_instance_removes_that_instance(orc):
    tris = sd.random_triangles(80, seed=4, spread=1.0, size=0.5)
    inst = [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (0, 0, (0.2, 0.1, 0.0, 0.3, 0.0, 0.0), (1.0, 1.0, 1.0)),
            (0, 0, (-0.2, 0.0, 0.1, 0.0, 0.5, 0.0), (0.8, 0.8, 0.8))]
    full = _scene(orc, tris, inst)
    rng = np.random.default_rng(2)
    q = (rng.uniform(-1, 1, (200, 1, 3)) + rng.uniform(-0.3, 0.3, (200, 3, 3))).astype(F32)
    try:
        for k in range(3):
            part = _scene(orc, tris, [x for i, x in enumerate(inst) if i != k])
            try:
                got = ti.list_intersecting(full, q, np.full(len(q), k, np.int32))
                ref = ti.list_intersecting(part, q)
                remap = np.array([i for i in range(3) if i != k])
                assert np.array_equal(got["offsets"], ref["offsets"])
                assert np.array_equal(got["instance"], remap[ref["instance"]])
                for f in ("triangle", "normal", "segment"):
                    assert np.array_equal(got[f], ref[f]), f
            finally:
                part.close()
        none = ti.list_intersecting(full, q, np.full(len(q), -1, np.int32))
        assert np.array_equal(none["count"], ti.count_intersecting(full, q))
    finally:
        full.close()


def test_rooms_truncate_and_pad(orc):
    so = _scene(orc, _cube(orc))
    try:
        q = np.array([[(0.5, 0.5, -1), (0.5, 0.5, 2), (0.52, 0.49, 2)], [(5, 5, 5), (6, 5, 5), (5, 6, 5)],
                      [(-1, 0.3, 0.3), (2, 0.3, 0.3), (2, 0.7, 0.7)]], F32)
        full = ti.list_intersecting(so, q)
        for K in (1, 2, 8):
            r = ti.list_intersecting(so, q, max_hits=K)
            for j in range(3):
                a, b = full["offsets"][j], full["offsets"][j + 1]
                m = min(b - a, K)
                for f in ti.FIELDS:
                    assert np.array_equal(r[f][j, :m], full[f][a:a + m]), (K, j, f)
                assert (r["instance"][j, m:] == -1).all() and (r["triangle"][j, m:] == -1).all()
                assert (r["normal"][j, m:] == 0).all() and (r["segment"][j, m:] == 0).all()
            assert np.array_equal(r["count"], full["count"])
    finally:
        so.close()


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    h = rt.libs()[0]
    for name in ("rt_count_intersecting", "rt_intersecting_offsets_workspace_bytes", "rt_intersecting_offsets", "rt_list_intersecting"):
        assert hasattr(h, name) and name in rt.RT_HIP_SYMBOLS
    assert h.rt_intersecting_offsets_workspace_bytes(0) == 0 and h.rt_intersecting_offsets_workspace_bytes(-1) == 0
    ws = h.rt_intersecting_offsets_workspace_bytes(1000)
    assert ws >= 1000 * 4 + 8 and ws == h.rt_crossing_offsets_workspace_bytes(1000)
    p, bogus = C.c_void_p(64), C.c_void_p(16)
    cnt = rt.RtIntersectCounts(count=p)
    assert h.rt_count_intersecting(None, p, None, 3, C.byref(cnt), None, 0) == -1
    assert h.rt_count_intersecting(bogus, p, None, -1, C.byref(cnt), None, 0) == -1
    assert h.rt_count_intersecting(bogus, None, None, 3, C.byref(cnt), None, 0) == -1
    assert h.rt_count_intersecting(bogus, p, None, 3, None, None, 0) == -1
    assert h.rt_count_intersecting(bogus, p, None, 3, C.byref(rt.RtIntersectCounts()), None, 0) == -1      # no output at all
    assert h.rt_intersecting_offsets(None, p, None, 3, p, p, ws, None, 0) == -1
    assert h.rt_intersecting_offsets(bogus, p, None, -1, p, p, ws, None, 0) == -1
    assert h.rt_intersecting_offsets(bogus, None, None, 3, p, p, ws, None, 0) == -1
    assert h.rt_intersecting_offsets(bogus, p, None, 3, None, p, ws, None, 0) == -1
    assert h.rt_intersecting_offsets(bogus, p, None, 3, p, None, ws, None, 0) == -1                      # no workspace
    assert h.rt_intersecting_offsets(bogus, p, None, 1000, p, p, ws - 1, None, 0) == -1                  # workspace too small
    keys = dict(instance=C.c_void_p(64), triangle=C.c_void_p(128))
    out = rt.RtIntersectList(**keys)
    assert h.rt_list_intersecting(None, p, None, 3, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_intersecting(bogus, p, None, -1, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_intersecting(bogus, None, None, 3, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_intersecting(bogus, p, None, 3, None, 4, None, None, 0) == -1
    for missing in keys:                                                                    # every key field is required
        part = rt.RtIntersectList(**{k: v for k, v in keys.items() if k != missing}, normal=p, segment=p, count=p, pops=p)
        assert h.rt_list_intersecting(bogus, p, None, 3, None, 4, C.byref(part), None, 0) == -1, missing
    assert h.rt_list_intersecting(bogus, p, None, 3, None, 4, C.byref(rt.RtIntersectList(count=p, pops=p)), None, 0) == -1
    assert h.rt_list_intersecting(bogus, p, None, 3, p, 4, C.byref(out), None, 0) == -1           # both room forms
    assert h.rt_list_intersecting(bogus, p, None, 3, None, 0, C.byref(out), None, 0) == -1        # neither
    assert h.rt_list_intersecting(bogus, p, None, 0, p, 2, C.byref(out), None, 0) == -1


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    t = np.zeros((10, 3, 3), F32)
    skip = np.zeros(10, np.int32)
    calls = (lambda a, k=None: s.count_intersecting(a, k), lambda a, k=None: s.list_intersecting(a, k),
             lambda a, k=None: s.list_intersecting(a, k, max_hits=2))
    for bad in (t.astype(np.float64), np.zeros((10, 3), F32), t[:, :2].copy(), np.zeros((3, 3, 10), F32).transpose(2, 1, 0),
                t.reshape(-1), t.tolist()):
        for call in calls:
            with pytest.raises(ValueError):
                call(bad)
    for k in (skip.astype(np.int64), skip.astype(F32), np.zeros(9, np.int32), np.zeros((10, 1), np.int32), np.zeros(20, np.int32)[::2],
              [0] * 10):
        for call in calls:
            with pytest.raises(ValueError):
                call(t, k)
    for m in (0, -1, 2.0, True, "3", 2 ** 31):
        with pytest.raises(ValueError):
            s.list_intersecting(t, max_hits=m)
    for outs in ((), ("t",), ("distance",), ("winding",)):
        with pytest.raises(ValueError):
            s.count_intersecting(t, outputs=outs)
    for outs in ((), ("count",), ("count", "pops"), ("any",), ("instance", "distance"), ("instance", "instance")):
        with pytest.raises(ValueError):
            s.list_intersecting(t, outputs=outs)
    torch = pytest.importorskip("torch")
    tt = torch.zeros((10, 3, 3), dtype=torch.float32)
    for call in (lambda: s.count_intersecting(tt), lambda: s.list_intersecting(tt.double(), max_hits=1),
                 lambda: s.list_intersecting(tt, skip)):
        with pytest.raises(ValueError):
            call()
    assert not touched
    assert rt.Scene.INTERSECT_LIST_OUTPUTS == ("instance", "triangle", "normal", "segment")
    assert rt.Scene.INTERSECT_COUNT_OUTPUTS == ("count", "any", "pops")
    s.close()
