"""Closest-point queries without a GPU: the brute-force shim (tests/point_oracle.c) that the GPU tests compare with is pinned against a
float64 computation and hand-made cases, and the C-ABI and Python wrappers reject bad arguments before they touch a device (the GPU
side: test_gpu_point_query.py)."""
import ctypes as C

import numpy as np
import pytest

import point_oracle
import scene_defs as sd

F32 = np.float32
FLT_MAX = np.finfo(F32).max


def _closest64(p, a, b, c):
    """float64 closest point on triangle (a, b, c) to p, by the face projection when it lies inside, else the nearest edge point"""
    p, a, b, c = (np.asarray(v, np.float64) for v in (p, a, b, c))

    def seg(x, y):
        d = y - x
        dd = d @ d
        t = 0.0 if dd == 0 else min(max((p - x) @ d / dd, 0.0), 1.0)
        return x + t * d
    n = np.cross(b - a, c - a)
    cands = [seg(a, b), seg(a, c), seg(b, c)]
    if n @ n > 0:
        f = p - ((p - a) @ n) / (n @ n) * n
        if all(np.cross(y - x, f - x) @ n >= 0 for x, y in ((a, b), (b, c), (c, a))):
            cands.append(f)
    return min(cands, key=lambda q: (p - q) @ (p - q))


def _scene(orc, tris, instances):
    return sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", tris)], instances).build_oracle(orc)


def test_voronoi_regions_and_zero_distance(orc):
    """Every region of Ericson's classification on a right triangle, with the exact weights; points on a vertex, an edge or the face
    give distance 0."""
    A, AB, AC = np.zeros(3, F32), np.array([2, 0, 0], F32), np.array([0, 2, 0], F32)
    cases = [((-1, -1, 1), (0, 0)), ((3, -1, 1), (1, 0)), ((-1, 3, 1), (0, 1)), ((1, -1, 1), (0.5, 0)), ((-1, 1, 1), (0, 0.5)),
             ((2, 2, 1), (0.5, 0.5)), ((0.5, 0.5, 1), (0.25, 0.25))]
    for q, (b1, b2) in cases:
        w1, w2, d2 = point_oracle.on_triangle(np.array(q, F32), A, AB, AC)
        assert (w1, w2) == (F32(b1), F32(b2)), q
        c = A + F32(b1) * AB + F32(b2) * AC
        assert d2 == F32(((np.array(q, F32) - c) ** 2).sum()), q
    for q in ((0, 0, 0), (2, 0, 0), (0, 2, 0), (1, 0, 0), (1, 1, 0), (0.5, 0.5, 0), (0, 1.5, 0)):
        assert point_oracle.on_triangle(np.array(q, F32), A, AB, AC)[2] == 0.0, q


def test_degenerate_triangles_are_finite(orc):
    """Zero-area, collinear (either order), repeated-vertex and needle triangles never divide by zero: finite weights in [0, 1] and a
    distance within 1e-5 of the float64 segment distance."""
    rng = np.random.default_rng(1)
    tris = []
    for _ in range(200):
        a, b = rng.uniform(-1, 1, (2, 3)).astype(F32)
        kind = rng.integers(4)
        c = {0: a, 1: (a + F32(rng.choice([2.0, 0.5, -1.0])) * (b - a)).astype(F32), 2: b,
             3: (a + F32(0.4) * (b - a) + rng.uniform(-1, 1, 3).astype(F32) * F32(1e-6)).astype(F32)}[int(kind)]
        tris.append((a, b if kind else a, c))
    for a, b, c in tris:
        q = rng.uniform(-2, 2, 3).astype(F32)
        w1, w2, d2 = point_oracle.on_triangle(q, a, (b - a).astype(F32), (c - a).astype(F32))
        assert np.isfinite([w1, w2, d2]).all() and 0 <= w1 <= 1 and 0 <= w2 <= 1 and w1 + w2 <= 1 + 1e-6
        want = np.linalg.norm(q - _closest64(q, a, b, c))
        assert abs(np.sqrt(np.float64(d2)) - want) <= 1e-5 * max(1.0, want), (a, b, c, q)


def test_shim_against_float64(orc):
    """Scenes with rotation, translation, non-uniform and mirrored scale: the shim's winner is the float64 brute force's except where
    the two nearest float64 distances are within 1e-5, and its distance and world point are within 1e-5 (relative to the scene)."""
    o = orc.oracle()
    tris = sd.random_triangles(60, seed=11, spread=1.0, size=0.5)
    instances = [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (0, 0, (0.3, -0.2, 0.5, 0.4, -0.7, 1.1), (1.5, -0.5, 2.0)),
                 (0, 0, (-1.0, 0.5, 0.0, 0.0, 3.0, -0.2), (-1.0, -1.0, 0.25))]
    so = _scene(orc, tris, instances)
    try:
        rng = np.random.default_rng(2)
        pts = rng.uniform(-3, 3, (150, 3)).astype(F32)
        got = point_oracle.closest_points(so, pts)
        # float64 world triangles: the stored fp32 vertices through the instance map (apply_lre(inv_pose, v * scale), fp32)
        world = []
        for _m, _mat, pose, scale in instances:
            inv = o.invert_lre(np.asarray(pose, F32))
            v = tris[:, :9].reshape(-1, 3) * np.asarray(scale, F32)
            world.append(np.stack([o.apply_lre(inv, x.astype(F32)) for x in v]).reshape(-1, 3, 3).astype(np.float64))
        for j, p in enumerate(pts):
            d = []
            for i, w in enumerate(world):
                for k, t in enumerate(w):
                    q = _closest64(p, *t)
                    d.append((np.linalg.norm(p - q), i, k, q))
            d.sort(key=lambda e: e[0])
            assert abs(got["distance"][j] - d[0][0]) <= 1e-5 * 4, j
            assert np.abs(got["point"][j] - d[0][3]).max() <= 1e-4 or d[1][0] - d[0][0] <= 1e-5, j
            if d[1][0] - d[0][0] > 1e-5:
                assert (got["instance"][j], got["triangle"][j]) == (d[0][1], d[0][2]), j
    finally:
        so.close()


def test_tie_rule(orc):
    """Equal distances: the smaller instance index wins, then the smaller triangle index -- whatever the order of the copies."""
    t = sd.random_triangles(1, seed=3, spread=0.2, size=0.5)
    far = t.copy()
    far[:, [0, 3, 6]] += 5.0
    tris = np.concatenate([far, t, t, far])
    so = _scene(orc, tris, [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))] * 3)
    try:
        pts = np.random.default_rng(4).uniform(-0.5, 0.5, (40, 3)).astype(F32)
        got = point_oracle.closest_points(so, pts)
        assert (got["instance"] == 0).all() and (got["triangle"] == 1).all()
        alone = point_oracle.closest_points(so, pts, only_instance=2)
        assert (alone["instance"] == 2).all() and (alone["triangle"] == 1).all()
        assert np.array_equal(alone["distance"].view(np.uint32), got["distance"].view(np.uint32))
    finally:
        so.close()


def test_mirrored_and_scaled_distances_are_world_distances(orc):
    """Under mirrored and non-uniform scale the distance is the world distance: a unit triangle scaled by (-2, 3, 0.5) and a point
    straight above its scaled face, one beyond a scaled vertex and one off the scaled hypotenuse."""
    tri = np.asarray(orc.oracle().tri_from_vertices(np.array([0, 0, 0, 1, 0, 0, 0, 1, 0], F32)), F32)[None]
    so = _scene(orc, tri, [(0, 0, (0.0,) * 6, (-2.0, 3.0, 0.5))])
    try:
        got = point_oracle.closest_points(so, np.array([[-0.5, 0.5, 0.75], [1.0, 0.0, 0.0], [-2.0, 3.0, -1.0]], F32))
        assert np.allclose(got["distance"], [0.75, 1.0, np.sqrt(36 / 13 + 1)], rtol=1e-6, atol=0)
        assert np.allclose(got["point"][0], [-0.5, 0.5, 0.0], atol=1e-7)
    finally:
        so.close()


def test_max_distance_is_inclusive(orc):
    """The exact distance hits, its float predecessor misses; +inf hits; NaN and negative bounds miss (the distance then FLT_MAX)."""
    so = _scene(orc, sd.random_triangles(30, seed=6, spread=1.0, size=0.4), [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    try:
        pts = np.random.default_rng(7).uniform(-2, 2, (100, 3)).astype(F32)
        d = point_oracle.closest_points(so, pts)["distance"]
        assert (d > 0).all()
        for md, want in ((d, True), (np.nextafter(d, F32(0)), False), (np.full(100, np.inf, F32), True),
                         (np.full(100, np.nan, F32), False), (np.full(100, -1.0, F32), False)):
            got = point_oracle.closest_points(so, pts, np.asarray(md, F32))
            assert ((got["instance"] >= 0) == want).all()
            if not want:
                assert (got["distance"] == FLT_MAX).all() and (got["triangle"] == -1).all() and not got["point"].any()
    finally:
        so.close()


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    """librt_hip.so exports rt_closest_points; it refuses a NULL scene, n < 0, NULL points and no output before touching the scene."""
    h = rt.libs()[0]
    assert hasattr(h, "rt_closest_points")
    hits = rt.RtPointHits()
    out = C.c_void_p(64)
    with_out = rt.RtPointHits(distance=out)
    assert h.rt_closest_points(None, C.c_void_p(64), None, 3, C.byref(with_out), None, 0) == -1
    bogus = C.c_void_p(16)                                        # a handle that is never dereferenced
    assert h.rt_closest_points(bogus, C.c_void_p(64), None, -1, C.byref(with_out), None, 0) == -1
    assert h.rt_closest_points(bogus, None, None, 3, C.byref(with_out), None, 0) == -1
    assert h.rt_closest_points(bogus, C.c_void_p(64), None, 3, C.byref(hits), None, 0) == -1
    assert h.rt_closest_points(bogus, C.c_void_p(64), None, 3, None, None, 0) == -1


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    p = np.zeros((10, 3), F32)
    for bad in (p.astype(np.float64), p[:, :2].copy(), np.zeros((3, 10), F32).T, p.reshape(-1), [[0, 0, 0]] * 10):
        with pytest.raises(ValueError):
            s.closest_points(bad)
    for md in (np.zeros(9, F32), np.zeros(10, np.float64), np.zeros((10, 1), F32)):
        with pytest.raises(ValueError):
            s.closest_points(p, md)
    for outs in (("distance", "colour"), (), ("t",)):
        with pytest.raises(ValueError):
            s.closest_points(p, outputs=outs)
    torch = pytest.importorskip("torch")
    t = torch.zeros((10, 3), dtype=torch.float32)
    for a, md in ((t, None), (t, np.zeros(10, F32)), (t.double(), None), (torch.zeros((3, 10)).t(), None)):
        with pytest.raises(ValueError):
            s.closest_points(a, md)
    assert not touched
    assert rt.Scene.POINT_OUTPUTS == ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv", "pops")
    s.close()
