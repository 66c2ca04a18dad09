"""Crossing lists without a GPU: the brute-force shim (tests/crossing_list_oracle.c) that test_gpu_crossing_list.py compares with is
pinned against crossing_oracle's counts and t, float64 barycentrics, hand-made ties, rooms and signs; the C-ABI and the Python wrapper
reject bad arguments before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import crossing_list_oracle as xl
import crossing_oracle as xo
import scene_defs as sd
from test_crossing_host import _cube, _mesh, _scene

F32 = np.float32


def _rays(rng, n, lo=-1.5, hi=1.5):
    return rng.uniform(lo, hi, (n, 3)).astype(F32), rng.normal(size=(n, 3)).astype(F32)


def test_members_and_t_equal_count_crossings(orc, scenes, blob5k):
    """On the cube, the multi-instance blob scene and an adversarial scene: per ray, the list length equals count_crossings, the sign
    sum equals the winding, the t multiset equals crossing_ts, and the list is sorted by (t, instance, triangle)."""
    rng = np.random.default_rng(0)
    descs = [sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", _cube(orc))], [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))]),
             sd.multi_instance_scene(scenes, blob5k), sd.adversarial_scene(scenes, np.random.default_rng(91003))[0]]
    for desc in descs:
        so = desc.build_oracle(orc)
        try:
            o, d = _rays(rng, 300)
            got = xl.list_crossings(so, o, d)
            ref = xo.count_crossings(so, o, d)
            assert np.array_equal(got["count"], ref["count"])
            assert np.array_equal(np.diff(got["offsets"]), ref["count"])
            wsum = np.zeros(len(o), np.int64)
            np.add.at(wsum, got["ray"], got["sign"].astype(np.int64))
            assert np.array_equal(wsum, ref["winding"])
            assert (got["t"] > 0).all() and set(np.unique(got["sign"])) <= {-1, 1}
            for j in range(0, len(o), 7):
                a, b = got["offsets"][j], got["offsets"][j + 1]
                assert np.array_equal(got["t"][a:b], xo.crossing_ts(so, o[j], d[j]))
                key = list(zip(got["t"][a:b], got["instance"][a:b], got["triangle"][a:b]))
                assert key == sorted(key)
        finally:
            so.close()


def test_barycentrics_match_float64(orc):
    """b1, b2 and t of random rays through random triangles: b1, b2 in [0, 1], and each within 4 ulps of 1, times the condition
    number of the float64 system (measured: at most 1.5), of the float64 intersection with the same fp32 inputs."""
    rng = np.random.default_rng(1)
    seen = 0
    for _ in range(2000):
        A, B, Cc = (rng.uniform(-1, 1, 3).astype(F32) for _ in range(3))
        w = rng.dirichlet((1, 1, 1))
        target = w[0] * A + w[1] * B + w[2] * Cc
        o = rng.uniform(-3, 3, 3).astype(F32)
        d = (target - o).astype(F32)
        s, t, V, W, det = xl.on_triangle(o, d, A, (B - A).astype(F32), (Cc - A).astype(F32))
        if not s:
            continue
        seen += 1
        b1, b2 = V / det, W / det
        assert 0 <= b1 <= 1 and 0 <= b2 <= 1
        M = np.stack([-d.astype(np.float64), (B - A).astype(F32).astype(np.float64), (Cc - A).astype(F32).astype(np.float64)], axis=1)
        tol = 4 * 2.0 ** -24 * np.linalg.cond(M)
        t64, u64, v64 = np.linalg.solve(M, o.astype(np.float64) - A.astype(np.float64))
        assert abs(b1 - u64) <= tol and abs(b2 - v64) <= tol and abs(t - t64) <= tol, (b1, u64, b2, v64, t, t64, tol)
    assert seen > 1500


def test_ties_order_by_instance_then_triangle(orc):
    """Two coincident triangles, two overlapping instances and a ray through a shared edge: equal t, ordered by (instance, triangle)."""
    quad = _mesh(orc, [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], [(0, 1, 2), (0, 2, 3)])
    twin = np.concatenate([quad[:1], quad[:1]])                     # triangles 0 and 1 coincide
    so = _scene(orc, twin, [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    try:
        r = xl.list_crossings(so, np.array([[0.7, 0.2, -1]], F32), np.array([[0, 0, 1]], F32))
        assert r["count"].tolist() == [4] and (r["t"] == 1).all()
        assert r["instance"].tolist() == [0, 0, 1, 1] and r["triangle"].tolist() == [0, 1, 0, 1]
    finally:
        so.close()
    so = _scene(orc, quad)
    try:                                                            # the diagonal shared by triangles 0 and 1
        r = xl.list_crossings(so, np.array([[0.5, 0.5, -1]], F32), np.array([[0, 0, 1]], F32))
        assert r["count"][0] == xo.count_crossings(so, np.array([[0.5, 0.5, -1]], F32), np.array([[0, 0, 1]], F32))["count"][0]
        if r["count"][0] == 2:
            assert r["triangle"].tolist() == [0, 1] and r["t"][0] == r["t"][1]
    finally:
        so.close()


def test_rooms_truncate_and_pad(orc):
    """Fixed rooms of K = 1, 2, 5 hold the prefix of the CSR list and pad with (inf, -1, -1, 0, 0...); CSR rooms smaller than the
    count truncate; a room of 0 or less writes nothing, and slots outside every room keep their fill."""
    so = _scene(orc, _cube(orc))
    try:
        o = np.array([[-1, 0.3, 0.4], [0.5, 0.5, 0.5], [5, 5, 5], [-1, 0.6, 0.45]], F32)
        d = np.array([[1, 0.01, 0.02], [0.1, 0.2, 1], [1, 0, 0], [1, 0.02, 0.01]], F32)
        full = xl.list_crossings(so, o, d)
        assert full["count"].tolist() == [2, 1, 0, 2]
        for K in (1, 2, 5):
            r = xl.list_crossings(so, o, d, max_hits=K)
            for j in range(4):
                a, b = full["offsets"][j], full["offsets"][j + 1]
                m = min(b - a, K)
                assert np.array_equal(r["t"][j, :m], full["t"][a:a + m]) and np.array_equal(r["triangle"][j, :m], full["triangle"][a:a + m])
                assert (r["t"][j, m:] == np.inf).all() and (r["instance"][j, m:] == -1).all() and (r["triangle"][j, m:] == -1).all()
                assert (r["sign"][j, m:] == 0).all() and (r["barycentric"][j, m:] == 0).all() and (r["point"][j, m:] == 0).all()
            assert np.array_equal(r["count"], full["count"])
        off = np.array([6, 7, 7, 1, 4], np.int64)                   # rooms [6, 7), [7, 7), [7, 1) (negative), [1, 4) in 8 slots
        g = xl.rooms(so, o, d, offsets=off, slots=8, fill=dict(t=-7.0, instance=-7, triangle=-7, sign=-7))
        assert g["t"][[0, 4, 5, 7]].tolist() == [-7] * 4 and g["sign"][[0, 4, 5, 7]].tolist() == [-7] * 4
        assert g["t"][6] == full["t"][0] and g["triangle"][6] == full["triangle"][0]          # ray 0 truncated to its first hit
        assert np.array_equal(g["t"][1:3], full["t"][3:5]) and g["t"][3] == np.inf and g["instance"][3] == -1
        assert g["count"].tolist() == [2, 1, 0, 2]
    finally:
        so.close()


def test_sign_on_cube_and_mirrored_instance(orc):
    """A ray through the cube enters (-1) then leaves (+1); through a mirrored instance the signs flip; points lie on the faces."""
    tris = _cube(orc)
    for scale, want in (((1.0, 1.0, 1.0), [-1, 1]), ((-1.0, 1.0, 1.0), [1, -1])):
        so = _scene(orc, tris, [(0, 0, (0.0,) * 6, scale)])
        try:
            x0 = -2.0 if scale[0] > 0 else -3.0
            r = xl.list_crossings(so, np.array([[x0, 0.3, 0.4]], F32), np.array([[1, 0.01, 0.02]], F32))
            assert r["sign"].tolist() == want
            px = r["point"][:, 0]
            assert np.allclose(px, [0, 1] if scale[0] > 0 else [-1, 0], atol=1e-6)
        finally:
            so.close()


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    h = rt.libs()[0]
    for name in ("rt_crossing_offsets_workspace_bytes", "rt_crossing_offsets", "rt_list_crossings"):
        assert hasattr(h, name)
    assert h.rt_crossing_offsets_workspace_bytes(0) == 0 and h.rt_crossing_offsets_workspace_bytes(-1) == 0
    ws = h.rt_crossing_offsets_workspace_bytes(1000)
    assert ws >= 1000 * 4 + 8
    p, bogus = C.c_void_p(64), C.c_void_p(16)
    out, none = rt.RtCrossingList(t=C.c_void_p(64)), rt.RtCrossingList()
    assert h.rt_crossing_offsets(None, p, p, None, 3, p, p, ws, None, 0) == -1
    assert h.rt_crossing_offsets(bogus, p, p, None, -1, p, p, ws, None, 0) == -1
    assert h.rt_crossing_offsets(bogus, None, p, None, 3, p, p, ws, None, 0) == -1
    assert h.rt_crossing_offsets(bogus, p, p, None, 3, None, p, ws, None, 0) == -1
    assert h.rt_crossing_offsets(bogus, p, p, None, 3, p, None, ws, None, 0) == -1
    assert h.rt_crossing_offsets(bogus, p, p, None, 1000, p, p, ws - 1, None, 0) == -1      # workspace too small
    assert h.rt_list_crossings(None, p, p, None, 3, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_crossings(bogus, p, p, None, -1, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_crossings(bogus, None, p, None, 3, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_crossings(bogus, p, p, None, 3, None, 4, None, None, 0) == -1
    assert h.rt_list_crossings(bogus, p, p, None, 3, None, 4, C.byref(none), None, 0) == -1
    assert h.rt_list_crossings(bogus, p, p, None, 3, p, 4, C.byref(out), None, 0) == -1        # both room forms
    assert h.rt_list_crossings(bogus, p, p, None, 3, None, 0, C.byref(out), None, 0) == -1     # neither
    assert h.rt_list_crossings(bogus, p, p, None, 0, p, 2, C.byref(out), None, 0) == -1


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    p = np.zeros((10, 3), F32)
    for bad in (p.astype(np.float64), p[:, :2].copy(), np.zeros((3, 10), F32).T, p.reshape(-1), [[0, 0, 0]] * 10):
        for call in (lambda: s.list_crossings(bad, p), lambda: s.list_crossings(p, bad), lambda: s.list_crossings(bad, p, max_hits=2)):
            with pytest.raises(ValueError):
                call()
    for tm in (np.zeros(9, F32), np.zeros(10, np.float64), np.zeros((10, 1), F32)):
        with pytest.raises(ValueError):
            s.list_crossings(p, p, tm)
    for k in (0, -1, 2.0, True, "3", 2 ** 31):
        with pytest.raises(ValueError):
            s.list_crossings(p, p, max_hits=k)
    for outs in (("t", "count"), (), ("winding",)):
        with pytest.raises(ValueError):
            s.list_crossings(p, p, outputs=outs)
    torch = pytest.importorskip("torch")
    t = torch.zeros((10, 3), dtype=torch.float32)
    for call in (lambda: s.list_crossings(t, t), lambda: s.list_crossings(t, p), lambda: s.list_crossings(t.double(), t)):
        with pytest.raises(ValueError):
            call()
    assert not touched
    assert rt.Scene.CROSSING_LIST_OUTPUTS == ("t", "instance", "triangle", "sign", "barycentric", "uv", "point")
    s.close()
