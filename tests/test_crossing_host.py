"""Crossing counts, winding numbers and signed distance without a GPU: the brute-force shim (tests/crossing_oracle.c) that the GPU
tests compare with is pinned on hand-made solids and against a float64 solid-angle winding number, and the C-ABI and Python wrappers
reject bad arguments before they touch a device (the GPU side: test_gpu_crossings.py)."""
import ctypes as C

import numpy as np
import pytest

import crossing_oracle as xo
import scene_defs as sd

F32 = np.float32
DIRS = np.array([[float.fromhex(x) for x in row.split()] for row in ("0x1.24b5dcp-1 0x1.3e5c92p-2 0x1.84c2f8p-1",
                 "-0x1.3f212ep-1 0x1.6d9e84p-1 0x1.46594ap-2", "0x1.2809d4p-2 0x1.488ce8p-1 -0x1.6bac72p-1")], F32)


def _mesh(orc, verts, faces):
    o = orc.oracle()
    v = np.asarray(verts, F32)
    return np.stack([np.asarray(o.tri_from_vertices(v[list(f)].ravel()), F32) for f in faces])


def _cube(orc):
    """the unit cube [0, 1]^3, 12 triangles counter-clockwise seen from outside"""
    v = [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return _mesh(orc, v, [f for a, b, c, d in quads for f in ((a, b, c), (a, c, d))])


def _tetra(orc):
    v = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]
    return _mesh(orc, v, [(0, 2, 1), (0, 1, 3), (0, 3, 2), (1, 2, 3)])


def _scene(orc, tris, instances=((0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)),)):
    return sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", tris)], list(instances)).build_oracle(orc)


def _dirs_each(pts):
    """every point along each fixed direction, with tmax +inf -> per-direction windings [n, 3] via the ray entry point"""
    p = np.repeat(np.asarray(pts, F32), 3, axis=0)
    d = np.tile(DIRS, (len(pts), 1))
    return p, d


def test_cube_and_tetrahedron_inside_outside(orc):
    """Inside points wind +1 along each fixed direction, outside points 0; the median agrees and the ray entry point along the same
    directions gives the same windings."""
    rng = np.random.default_rng(0)
    for tris, inside in ((_cube(orc), lambda p: (p > 0).all(1) & (p < 1).all(1)),
                         (_tetra(orc), lambda p: (p > 0).all(1) & (p.sum(1) < 1))):
        so = _scene(orc, tris)
        try:
            pts = rng.uniform(-0.5, 1.5, (400, 3)).astype(F32)
            keep = np.abs(pts - np.round(pts)).min(1) > 1e-3
            pts = pts[keep & (np.abs(pts.sum(1) - 1) > 1e-3)]
            want = inside(pts).astype(np.int32)
            med, per = xo.winding_numbers(so, pts, per_direction=True)
            assert np.array_equal(med, want)
            assert np.array_equal(per, np.repeat(want[:, None], 3, axis=1))
            p, d = _dirs_each(pts)
            got = xo.count_crossings(so, p, d)
            assert np.array_equal(got["winding"].reshape(-1, 3), per)
            cnt = got["count"].reshape(-1, 3)
            assert (cnt[want == 1] == 1).all() and np.isin(cnt[want == 0], (0, 2)).all()     # from outside 0 or 2 crossings
        finally:
            so.close()


def test_segments_count_zero_one_two(orc):
    """Segments through the cube (d = b - a, tmax = 1): outside to outside across it 2 (winding 0), inside to outside 1 (+1),
    outside to inside 1 (-1), inside to inside 0, and a segment that stops short 0."""
    so = _scene(orc, _cube(orc))
    try:
        a = np.array([[-0.5, 0.3, 0.4], [0.5, 0.5, 0.5], [-0.5, 0.3, 0.4], [0.2, 0.3, 0.4], [-0.5, 0.3, 0.4]], F32)
        b = np.array([[1.5, 0.6, 0.45], [0.7, 0.4, 2.0], [0.5, 0.6, 0.45], [0.8, 0.7, 0.6], [-0.1, 0.6, 0.45]], F32)
        got = xo.count_crossings(so, a, (b - a).astype(F32), np.ones(5, F32))
        assert got["count"].tolist() == [2, 1, 1, 0, 0]
        assert got["winding"].tolist() == [0, 1, -1, 0, 0]
        unb = xo.count_crossings(so, a, (b - a).astype(F32))                 # tmax +inf: every ray leaves the cube
        assert unb["winding"].tolist() == [0, 1, 0, 1, 0]
    finally:
        so.close()


def test_mirrored_and_overlapping_instances(orc):
    """A mirrored instance (scale (-1, 1, 1)) winds -1 inside; two overlapping instances wind 2 where both hold the point; the
    nonzero rule calls both inside."""
    tris = _cube(orc)
    so = _scene(orc, tris, [(0, 0, (0.0,) * 6, (-1.0, 1.0, 1.0))])
    try:
        assert xo.winding_numbers(so, np.array([[-0.5, 0.5, 0.5], [0.5, 0.5, 0.5]], F32)).tolist() == [-1, 0]
    finally:
        so.close()
    so = _scene(orc, tris, [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (0, 0, (0.5, 0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    try:
        got = xo.winding_numbers(so, np.array([[0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [1.25, 0.5, 0.5], [1.75, 0.5, 0.5]], F32))
        assert got.tolist() == [1, 2, 1, 0]
    finally:
        so.close()


def test_t_zero_not_counted_tmax_inclusive_both_faces_zero_direction(orc):
    """An origin on a face (t = 0) is not counted; t == tmax is, its float predecessor is not; a ray hitting a triangle's back face
    counts (with the other sign); a zero direction counts nothing."""
    A, AB, AC = np.zeros(3, F32), np.array([1, 0, 0], F32), np.array([0, 1, 0], F32)
    up, down = np.array([0, 0, 1], F32), np.array([0, 0, -1], F32)
    s, t = xo.on_triangle(np.array([0.2, 0.2, 0.0], F32), up, A, AB, AC)
    assert s == 0
    s_up, t_up = xo.on_triangle(np.array([0.2, 0.2, -2.0], F32), up, A, AB, AC)
    s_dn, t_dn = xo.on_triangle(np.array([0.2, 0.2, 2.0], F32), down, A, AB, AC)
    assert (s_up, t_up) == (1, 2.0) and (s_dn, t_dn) == (-1, 2.0)          # normal +z: upward leaves (+1), downward enters (-1)
    assert xo.on_triangle(np.array([0.2, 0.2, -2.0], F32), up, A, AB, AC, tmax=2.0)[0] == 1
    assert xo.on_triangle(np.array([0.2, 0.2, -2.0], F32), up, A, AB, AC, tmax=np.nextafter(F32(2), F32(0)))[0] == 0
    assert xo.on_triangle(np.array([0.2, 0.2, -2.0], F32), np.zeros(3, F32), A, AB, AC)[0] == 0
    so = _scene(orc, _cube(orc))
    try:
        o = np.array([[0.0, 0.5, 0.5], [0.3, 0.3, 0.3]], F32)                # on the face x = 0; inside
        got = xo.count_crossings(so, o, np.array([[1, 0.01, 0.02], [0, 0, 0]], F32))
        assert got["count"].tolist() == [1, 0] and got["winding"].tolist() == [1, 0]
        ts = xo.crossing_ts(so, np.array([-1.0, 0.5, 0.5], F32), np.array([1.0, 0.01, 0.02], F32))
        assert len(ts) == 2 and np.allclose(ts, [1.0, 2.0], rtol=1e-6)
        assert xo.count_crossings(so, np.array([[-1.0, 0.5, 0.5]], F32), np.array([[1.0, 0.01, 0.02]], F32), ts[1:2])["count"][0] == 2
        assert xo.count_crossings(so, np.array([[-1.0, 0.5, 0.5]], F32), np.array([[1.0, 0.01, 0.02]], F32),
                                  np.nextafter(ts[1:2], F32(0)))["count"][0] == 1
    finally:
        so.close()


def test_fp64_signs_survive_rounding(orc):
    """Edge functions whose fp32 products underflow go to fp64, and a nonzero fp64 value below 2^-150 keeps its sign (+-2^-149): a
    triangle 2^-15 beside the line x = y = 0 (edge functions -2^-150, 2^-136, 2^-136) is not counted, its mirror image across the
    line (2^-150, 2^-136, 2^-136: the line passes through it) is."""
    o, d = np.zeros(3, F32), np.array([0, 0, 1], F32)
    e, h = F32(2.0 ** -15), F32(2.0 ** -136)
    for sx, want in ((-1, 0), (1, -1)):
        A = np.array([-1, 0, 1], F32)
        B = np.array([sx * e, h, 1], F32)
        C = np.array([sx * e, -h, 1], F32)
        s, t = xo.on_triangle(o, d, A, (B - A).astype(F32), (C - A).astype(F32))
        assert s == want, (sx, s, t)
        if want:
            assert t == 1.0


def _solid_angle_winding(p, tris):
    """float64 generalised winding number: the sum of the Van Oosterom-Strackee solid angles of the triangles over 4 pi"""
    a, b, c = (tris[:, k * 3:(k + 1) * 3].astype(np.float64)[None] - p[:, None] for k in range(3))
    la, lb, lc = (np.linalg.norm(x, axis=2) for x in (a, b, c))
    num = np.einsum("pij,pij->pi", a, np.cross(b, c))
    den = la * lb * lc + np.einsum("pij,pij->pi", a, b) * lc + np.einsum("pij,pij->pi", b, c) * la + np.einsum("pij,pij->pi", c, a) * lb
    return (2.0 * np.arctan2(num, den)).sum(axis=1) / (4.0 * np.pi)


def test_blob_median_equals_solid_angle(orc, scenes, blob5k):
    """On a few hundred points around the blob5k mesh (closed, outward winding), translated, rotated and scaled, the shim's median
    winding equals the rounded float64 solid-angle winding number of the world triangles, for points farther than 1e-4 from the
    surface."""
    import point_oracle
    o = orc.oracle()
    pose, scale = (0.2, -0.1, 0.3, 0.4, -0.2, 0.7), (1.3, 0.8, 1.1)
    desc = sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("obj", blob5k)], [(0, 0, pose, scale)])
    so = desc.build_oracle(orc)
    try:
        t = o.mesh_dump(desc.oracle_meshes[0])["tris"][:, :9].reshape(-1, 3)
        inv = o.invert_lre(np.asarray(pose, F32))
        world = np.stack([o.apply_lre(inv, (x * np.asarray(scale, F32)).astype(F32)) for x in t]).reshape(-1, 9)
        lo, hi = world.reshape(-1, 3).min(0), world.reshape(-1, 3).max(0)
        rng = np.random.default_rng(3)
        pts = (lo + (hi - lo) * rng.uniform(-0.1, 1.1, (400, 3))).astype(F32)
        d = point_oracle.closest_points(so, pts)["distance"]
        pts = pts[d > 1e-4]
        want = np.round(_solid_angle_winding(pts.astype(np.float64), world)).astype(np.int32)
        got = xo.winding_numbers(so, pts)
        assert np.array_equal(got, want), np.flatnonzero(got != want)
        assert 50 < (want == 1).sum() < len(pts) - 50 and set(np.unique(want)) <= {0, 1}
        sdf = xo.signed_distance(so, pts)
        assert np.array_equal(sdf < 0, want != 0) and np.array_equal(np.abs(sdf), point_oracle.closest_points(so, pts)["distance"])
    finally:
        so.close()


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    """librt_hip.so exports the three entry points; they refuse a NULL scene, n < 0, NULL inputs and no output before touching the
    scene."""
    h = rt.libs()[0]
    for name in ("rt_count_crossings", "rt_winding_numbers", "rt_signed_distance"):
        assert hasattr(h, name)
    p, bogus = C.c_void_p(64), C.c_void_p(16)                       # (a handle that is never dereferenced)
    out, none = rt.RtCrossings(count=C.c_void_p(64)), rt.RtCrossings()
    assert h.rt_count_crossings(None, p, p, None, 3, C.byref(out), None, 0) == -1
    assert h.rt_count_crossings(bogus, p, p, None, -1, C.byref(out), None, 0) == -1
    assert h.rt_count_crossings(bogus, None, p, None, 3, C.byref(out), None, 0) == -1
    assert h.rt_count_crossings(bogus, p, None, None, 3, C.byref(out), None, 0) == -1
    assert h.rt_count_crossings(bogus, p, p, None, 3, C.byref(none), None, 0) == -1
    assert h.rt_count_crossings(bogus, p, p, None, 3, None, None, 0) == -1
    assert h.rt_winding_numbers(None, p, 3, p, None, 0) == -1
    assert h.rt_winding_numbers(bogus, p, -1, p, None, 0) == -1
    assert h.rt_winding_numbers(bogus, None, 3, p, None, 0) == -1
    assert h.rt_winding_numbers(bogus, p, 3, None, None, 0) == -1
    assert h.rt_signed_distance(None, p, None, 3, p, None, None, 0) == -1
    assert h.rt_signed_distance(bogus, p, None, -1, p, None, None, 0) == -1
    assert h.rt_signed_distance(bogus, None, None, 3, p, None, None, 0) == -1
    assert h.rt_signed_distance(bogus, p, None, 3, None, p, None, 0) == -1


def test_python_wrappers_check_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    p = np.zeros((10, 3), F32)
    bads = (p.astype(np.float64), p[:, :2].copy(), np.zeros((3, 10), F32).T, p.reshape(-1), [[0, 0, 0]] * 10)
    for bad in bads:
        for call in (lambda: s.count_crossings(bad, p), lambda: s.count_crossings(p, bad), lambda: s.winding_numbers(bad),
                     lambda: s.signed_distance(bad)):
            with pytest.raises(ValueError):
                call()
    for tm in (np.zeros(9, F32), np.zeros(10, np.float64), np.zeros((10, 1), F32)):
        with pytest.raises(ValueError):
            s.count_crossings(p, p, tm)
        with pytest.raises(ValueError):
            s.signed_distance(p, tm)
    with pytest.raises(ValueError):
        s.count_crossings(p, np.zeros((11, 3), F32))
    for outs in (("count", "t"), (), ("distance",)):
        with pytest.raises(ValueError):
            s.count_crossings(p, p, outputs=outs)
    torch = pytest.importorskip("torch")
    t = torch.zeros((10, 3), dtype=torch.float32)
    for call in (lambda: s.count_crossings(t, t), lambda: s.count_crossings(t, p), lambda: s.winding_numbers(t),
                 lambda: s.signed_distance(t, np.zeros(10, F32)), lambda: s.winding_numbers(t.double())):
        with pytest.raises(ValueError):
            call()
    assert not touched
    assert rt.Scene.CROSSING_OUTPUTS == ("count", "winding", "pops")
    s.close()
