"""Nearby-triangle lists without a GPU: the brute-force shim (tests/nearby_oracle.c) that test_gpu_nearby.py compares with is pinned
against point_oracle's closest point, a float64 classification, hand-made ties and rooms; the C-ABI and the Python wrapper reject bad
arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import nearby_oracle as nb
import point_oracle
import scene_defs as sd
from test_crossing_host import _cube, _mesh, _scene

F32 = np.float32
FIELDS = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype != F32:
        return a
    return np.where(np.isnan(a), F32(np.nan), a).astype(F32).view(np.uint32)


def test_slot0_is_closest_point(orc, scenes, blob5k):
    """On the cube, the multi-instance blob scene and an adversarial scene, unbounded and bounded: slot 0 of every point's list is
    orcx_closest_points' winner on every field (a miss is padding in both), and each list is sorted by (d2, instance, triangle)."""
    rng = np.random.default_rng(0)
    descs = [sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", _cube(orc))], [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))]),
             sd.multi_instance_scene(scenes, blob5k), sd.adversarial_scene(scenes, np.random.default_rng(91003))[0]]
    for desc in descs:
        so = desc.build_oracle(orc)
        try:
            pts = rng.uniform(-1.5, 1.5, (200, 3)).astype(F32)
            ref = point_oracle.closest_points(so, pts)
            for md in (None, (ref["distance"] * rng.uniform(0.5, 2.0, len(pts))).astype(F32)):
                cp = ref if md is None else point_oracle.closest_points(so, pts, md)
                got = nb.list_nearby(so, pts, md, max_hits=3)
                for k in FIELDS:
                    assert np.array_equal(_bits(got[k][:, 0]), _bits(cp[k])), k
                d = got["distance"].astype(np.float64)
                assert (d[:, 1:] >= d[:, :-1]).all()
                assert ((got["count"] > 0) == (cp["instance"] >= 0)).all()
        finally:
            so.close()


def _d64(p, tris):
    """float64 distance from p to each triangle [m, 3, 3] (inside the face: the plane distance; else the nearest edge)"""
    a, b, c = (tris[:, i].astype(np.float64) for i in range(3))
    p = p.astype(np.float64)
    n = np.cross(b - a, c - a)
    nn = np.einsum("ij,ij->i", n, n)
    t = np.einsum("ij,ij->i", p - a, n) / nn
    q = p - t[:, None] * n
    inside = np.ones(len(tris), bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= np.einsum("ij,ij->i", np.cross(v - u, q - u), n) >= 0
    best = np.where(inside, np.linalg.norm(p - q, axis=1), np.inf)
    for u, v in ((a, b), (b, c), (c, a)):
        e = v - u
        s = np.clip(np.einsum("ij,ij->i", p - u, e) / np.einsum("ij,ij->i", e, e), 0, 1)
        best = np.minimum(best, np.linalg.norm(p - (u + s[:, None] * e), axis=1))
    return best


def test_counts_equal_float64_classification(orc):
    """200 random triangles, 300 points and a radius per point: each (point, triangle) whose float64 distance is clearly inside or
    outside the radius (1e-4 relative margin) is a pair exactly when inside, and the count equals the float64 count when no pair is
    near the bound."""
    rng = np.random.default_rng(1)
    desc = sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", sd.random_triangles(200, seed=5, spread=1.0, size=0.3))],
                        [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    so = desc.build_oracle(orc)
    verts = orc.oracle().mesh_dump(desc.oracle_meshes[0])["tris"][:, :9].reshape(-1, 3, 3)
    try:
        pts = rng.uniform(-1.2, 1.2, (300, 3)).astype(F32)
        md = rng.uniform(0.05, 0.6, 300).astype(F32)
        r = nb.list_nearby(so, pts, md)
        checked = 0
        for j in range(len(pts)):
            d = _d64(pts[j], verts)
            seg = slice(r["offsets"][j], r["offsets"][j + 1])
            mine = set(r["triangle"][seg].tolist())
            clear = np.abs(d - md[j]) > 1e-4 * max(float(md[j]), 1.0)
            want = set(np.flatnonzero((d <= md[j]) & clear).tolist())
            assert want <= mine and not (mine & set(np.flatnonzero((d > md[j]) & clear).tolist())), j
            if clear.all():
                assert r["count"][j] == int((d <= md[j]).sum())
                checked += 1
        assert checked > 250
    finally:
        so.close()


def test_ties_order_by_instance_then_triangle(orc):
    """A point above two coincident triangles of two overlapping instances: four pairs at one distance, ordered by (instance,
    triangle); K = 3 keeps the first three, K = 1 the closest point's winner."""
    quad = _mesh(orc, [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], [(0, 1, 2), (0, 2, 3)])
    twin = np.concatenate([quad[:1], quad[:1]])                     # triangles 0 and 1 coincide
    so = _scene(orc, twin, [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    try:
        p = np.array([[0.7, 0.2, 0.5]], F32)
        r = nb.list_nearby(so, p, np.array([1.0], F32))
        assert r["count"].tolist() == [4] and (r["distance"] == F32(0.5)).all()
        assert r["instance"].tolist() == [0, 0, 1, 1] and r["triangle"].tolist() == [0, 1, 0, 1]
        r3 = nb.list_nearby(so, p, max_hits=3)
        assert r3["instance"][0].tolist() == [0, 0, 1] and r3["triangle"][0].tolist() == [0, 1, 0]
        cp = point_oracle.closest_points(so, p)
        assert (cp["instance"][0], cp["triangle"][0]) == (0, 0)
    finally:
        so.close()


def test_bound_is_inclusive_and_special(orc):
    """The bound at a pair's distance keeps it, one float below drops it; NaN and negative bounds give no pairs; -0 keeps a point on
    the surface."""
    so = _scene(orc, _cube(orc))
    try:
        p = np.array([[0.5, 0.5, -0.25], [0.5, 0.5, 0.0]], F32)
        full = nb.list_nearby(so, p, max_hits=12)
        d = full["distance"][0, 0]
        assert nb.count_nearby(so, p[:1], np.array([d], F32))[0] == full["count"][0] - (full["distance"][0] > d).sum()
        assert nb.count_nearby(so, p[:1], np.array([np.nextafter(d, F32(0))], F32))[0] == 0
        for b in (np.nan, -1.0):
            assert nb.count_nearby(so, p, np.full(2, b, F32)).tolist() == [0, 0]
        assert nb.count_nearby(so, p[1:], np.array([-0.0], F32))[0] >= 1
    finally:
        so.close()


def test_rooms_truncate_and_pad(orc):
    """Fixed rooms of K = 1, 2, 5 hold the prefix of the CSR list and pad with (FLT_MAX, -1, -1, 0...); CSR rooms smaller than the
    count truncate; a room of 0 or less writes nothing, and slots outside every room keep their fill."""
    so = _scene(orc, _cube(orc))
    try:
        p = np.array([[0.5, 0.5, -0.1], [0.05, 0.05, 0.05], [5, 5, 5], [1.02, 0.5, 0.5]], F32)
        md = np.full(4, 0.3, F32)
        full = nb.list_nearby(so, p, md)
        assert full["count"].tolist()[2] == 0 and all(c >= 2 for c in full["count"][[0, 1, 3]])
        for K in (1, 2, 5):
            r = nb.list_nearby(so, p, md, max_hits=K)
            for j in range(4):
                a, b = full["offsets"][j], full["offsets"][j + 1]
                m = min(b - a, K)
                for k in FIELDS:
                    assert np.array_equal(r[k][j, :m], full[k][a:a + m]), (K, j, k)
                assert (r["distance"][j, m:] == np.finfo(F32).max).all() and (r["instance"][j, m:] == -1).all()
                assert (r["triangle"][j, m:] == -1).all() and (r["point"][j, m:] == 0).all() and (r["normal"][j, m:] == 0).all()
                assert (r["barycentric"][j, m:] == 0).all() and (r["uv"][j, m:] == 0).all()
            assert np.array_equal(r["count"], full["count"])
        c = full["count"]
        off = np.array([6, 7, 7, 1, 1 + c[3] - 1], np.int64)        # rooms [6, 7), [7, 7), [7, 1) (negative), [1, c3) in 16 slots
        g = nb.rooms(so, p, md, offsets=off, slots=16, fill=dict(distance=-7.0, instance=-7, triangle=-7))
        inroom = np.zeros(16, bool)
        inroom[6:7] = True
        inroom[1:off[4]] = True
        assert (g["distance"][~inroom] == -7).all() and (g["instance"][~inroom] == -7).all()
        assert g["triangle"][6] == full["triangle"][0]                                   # point 0 truncated to its nearest
        a3 = full["offsets"][3]
        assert np.array_equal(g["triangle"][1:off[4]], full["triangle"][a3:a3 + c[3] - 1])
        assert g["count"].tolist() == c.tolist()
    finally:
        so.close()


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    h = rt.libs()[0]
    for name in ("rt_nearby_offsets_workspace_bytes", "rt_nearby_offsets", "rt_list_nearby"):
        assert hasattr(h, name) and name in rt.RT_HIP_SYMBOLS
    assert h.rt_nearby_offsets_workspace_bytes(0) == 0 and h.rt_nearby_offsets_workspace_bytes(-1) == 0
    ws = h.rt_nearby_offsets_workspace_bytes(1000)
    assert ws >= 1000 * 4 + 8 and ws == h.rt_crossing_offsets_workspace_bytes(1000)
    p, bogus = C.c_void_p(64), C.c_void_p(16)
    keys = dict(distance=C.c_void_p(64), instance=C.c_void_p(128), triangle=C.c_void_p(192))
    out = rt.RtNearbyList(**keys)
    assert h.rt_nearby_offsets(None, p, None, 3, p, p, ws, None, 0) == -1
    assert h.rt_nearby_offsets(bogus, p, None, -1, p, p, ws, None, 0) == -1
    assert h.rt_nearby_offsets(bogus, None, None, 3, p, p, ws, None, 0) == -1
    assert h.rt_nearby_offsets(bogus, p, None, 3, None, p, ws, None, 0) == -1
    assert h.rt_nearby_offsets(bogus, p, None, 3, p, None, ws, None, 0) == -1
    assert h.rt_nearby_offsets(bogus, p, None, 1000, p, p, ws - 1, None, 0) == -1          # workspace too small
    assert h.rt_list_nearby(None, p, None, 3, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_nearby(bogus, p, None, -1, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_nearby(bogus, None, None, 3, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_nearby(bogus, p, None, 3, None, 4, None, None, 0) == -1
    for missing in keys:                                                                    # every key field is required
        part = rt.RtNearbyList(**{k: v for k, v in keys.items() if k != missing}, point=p, normal=p, barycentric=p, uv=p, count=p, pops=p)
        assert h.rt_list_nearby(bogus, p, None, 3, None, 4, C.byref(part), None, 0) == -1, missing
    assert h.rt_list_nearby(bogus, p, None, 3, None, 4, C.byref(rt.RtNearbyList(count=p, pops=p)), None, 0) == -1
    assert h.rt_list_nearby(bogus, p, None, 3, p, 4, C.byref(out), None, 0) == -1           # both room forms
    assert h.rt_list_nearby(bogus, p, None, 3, None, 0, C.byref(out), None, 0) == -1        # neither
    assert h.rt_list_nearby(bogus, p, None, 0, p, 2, C.byref(out), None, 0) == -1


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    p = np.zeros((10, 3), F32)
    md = np.ones(10, F32)
    for bad in (p.astype(np.float64), p[:, :2].copy(), np.zeros((3, 10), F32).T, p.reshape(-1), [[0, 0, 0]] * 10):
        for call in (lambda: s.list_nearby(bad, md), lambda: s.list_nearby(bad, max_hits=2)):
            with pytest.raises(ValueError):
                call()
    for m in (np.zeros(9, F32), np.zeros(10, np.float64), np.zeros((10, 1), F32), [1.0] * 10):
        with pytest.raises(ValueError):
            s.list_nearby(p, m)
    for k in (0, -1, 2.0, True, "3", 2 ** 31):
        with pytest.raises(ValueError):
            s.list_nearby(p, md, max_hits=k)
    for outs in ((), ("count",), ("count", "pops"), ("t",), ("distance", "sign"), ("distance", "distance"), ("winding",)):
        with pytest.raises(ValueError):
            s.list_nearby(p, md, outputs=outs)
    with pytest.raises(ValueError):                                 # n x T pairs: refused, the C-ABI allows it
        s.list_nearby(p)
    torch = pytest.importorskip("torch")
    t = torch.zeros((10, 3), dtype=torch.float32)
    for call in (lambda: s.list_nearby(t, md), lambda: s.list_nearby(t.double(), max_hits=1), lambda: s.list_nearby(t, None)):
        with pytest.raises(ValueError):
            call()
    assert not touched
    assert rt.Scene.NEARBY_LIST_OUTPUTS == ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")
    s.close()
