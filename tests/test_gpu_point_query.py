"""Closest-point queries on the GPU (rt_closest_points through Scene.closest_points): every output but `pops` is compared bit for bit with
the brute-force shim over the test oracle's scene (tests/point_oracle.c), on the library's scenes, the adversarial scenes of
scene_defs.adversarial_scene, after scene changes and under every call shape.  `pops` is only bounded."""
import numpy as np
import pytest

import point_oracle
import query_points as qp
import ray_oracle
import scene_defs as sd

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max
EXACT = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")
ALL = EXACT + ("pops",)
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 17, 23]


def _bits(a):
    """bit patterns, except that every NaN is one pattern: a winner at an overflowed (+inf) distance maps an infinite point to world
    space, and the GPU and the CPU spell the resulting NaN differently (the rule of the ray-query fuzz)"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.float32(np.nan), a).astype(np.float32).view(np.uint32)


def _same(got, ref, where="", keys=EXACT):
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape, (where, k, g.shape, r.shape)
        bad = np.flatnonzero((_bits(g) != _bits(r)).reshape(g.shape[0] if g.ndim else 1, -1).any(axis=-1))
        assert bad.size == 0, "%s %s: %d points differ, first %s: got %s want %s" % (where, k, bad.size, bad[:3], g[bad[:3]], r[bad[:3]])


def _product(rt, desc, for_device=False):
    """desc on the device; for_device: every mesh uploaded without a tree (num_nodes = 0), the scene builds it on the GPU"""
    if not for_device:
        sp = desc.build_product(rt)
    else:
        sp = rt.Scene()
        for mat in desc.materials:
            sp.add_material(mat[0], texture_bgr=mat[1])
        for kind, arg in desc.meshes:
            sp.add_mesh(rt.Mesh.load_obj(arg, for_device=True) if kind == "obj" else rt.Mesh.from_triangles(arg, for_device=True))
        for mesh, mat, pose, scale in desc.instances:
            sp.add_mesh_instance(mesh, mat, pose, scale)
    sp.upload_to_device()
    return sp


def _cam_rays(scenes, W, H, K, pose):
    return ray_oracle.camera_rays(W, H, K, scenes.D_REF, pose)


def _check(sp, so, pts, md=None, where=""):
    got = sp.closest_points(pts, md, outputs=ALL)
    ref = point_oracle.closest_points(so, pts, md)
    _same(got, ref, where)
    assert (got["pops"] >= 0).all(), where
    return got, ref


def _library_scene(name, scenes, blob5k, demo_objs):
    if name == "c1":
        c1 = scenes.C1
        return sd.c1_scene(scenes), (64, 64, scenes.scaled_K(64), c1["cam_pose"])
    if name == "multi":
        m = sd.MULTI_CAMERA
        return sd.multi_instance_scene(scenes, blob5k), (96, 54, scenes.scaled_K(96), m["pose"])
    if name == "demo":
        return sd.demo_scene(scenes, demo_objs), (96, 54, scenes.scaled_K(96), scenes.DEMO["cam_pose"])
    return sd.deep_stack_scene(28), (96, 64, scenes.scaled_K(96), (0.0, -1.0, 0.0, 0.0, 0.0, 0.0))


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    """Every point family on c1, the multi-instance scene (rotation, non-uniform scale, texture), the demo scene and a 28-level tree,
    unbounded and with the special bounds: equal to the shim bit for bit."""
    desc, (W, H, K, pose) = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=400))
        got, ref = _check(sp, so, pts, where=name)
        assert (ref["instance"] >= 0).all()
        md = qp.special_bounds(rng, ref["distance"])
        _check(sp, so, pts, md, where=name + " bounded")
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_adversarial_scenes_equal_oracle(rt, orc, scenes, seed):
    """The render fuzz's adversarial scenes (lattices, degenerate and needle triangles, piles above 30 per leaf, 1e18 and 1e-20
    coordinates, non-finite vertices; mirrored, tiny and huge scales): every family, unbounded and bounded, equal to the shim."""
    desc, W, H, K, pose, info = sd.adversarial_scene(scenes, np.random.default_rng(91000 + seed))
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(seed)
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300))
        got, ref = _check(sp, so, pts, where=info)
        _check(sp, so, pts, qp.special_bounds(rng, ref["distance"]), where=info + " bounded")
    finally:
        sp.close()
        so.close()


def test_max_distance_boundary(rt, orc, scenes, blob5k):
    """The bound is inclusive: the exact distance hits, its float predecessor misses; +inf hits, NaN and negative bounds miss."""
    desc, (W, H, K, pose) = _library_scene("multi", scenes, blob5k, None)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        pts = qp.flatten(qp.families(np.random.default_rng(2), orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300))
        d = sp.closest_points(pts)["distance"]
        n = len(d)
        for md, hit in ((d, True), (np.nextafter(d, np.float32(0)), None), (np.full(n, np.inf, np.float32), True),
                        (np.full(n, np.nan, np.float32), False), (np.full(n, -1.0, np.float32), False)):
            md = np.ascontiguousarray(md, np.float32)
            got, ref = _check(sp, so, pts, md, where="bound")
            if hit is not None:
                assert ((got["instance"] >= 0) == hit).all()
        # every other triangle is at least as far as the winner, so below a positive distance nothing is left (at 0 the bound is 0)
        got = sp.closest_points(pts, np.ascontiguousarray(np.nextafter(d, np.float32(0)), np.float32))
        assert (got["instance"][d > 0] < 0).all() and (got["instance"][d == 0] >= 0).all()
    finally:
        sp.close()
        so.close()


def test_tree_independence(rt, orc, scenes, blob5k):
    """The same triangles under the host-built tree and under a tree built on the device (num_nodes = 0) give identical results.
    The two builders make the same tree node for node (test_gpu_bvh_build_matches_host_builder), so this compares the two ways of
    getting one tree onto the device, not two trees: trees the library does not build are tests/test_gpu_caller_trees.py's."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    a, b = _product(rt, desc), _product(rt, desc, for_device=True)
    try:
        m = sd.MULTI_CAMERA
        pts = qp.flatten(qp.families(np.random.default_rng(4), orc.oracle(), desc, so,
                                     _cam_rays(scenes, 96, 54, scenes.scaled_K(96), m["pose"]), n=400))
        ga, gb = a.closest_points(pts, outputs=ALL), b.closest_points(pts, outputs=ALL)
        _same(ga, gb, "host tree vs device tree")
        _same(ga, point_oracle.closest_points(so, pts), "host tree vs shim")
    finally:
        a.close()
        b.close()
        so.close()


def test_queries_follow_scene_changes(rt, orc, scenes, blob5k):
    """After refit_mesh, rebuild_mesh and an async update_mesh_instance on a stream, results equal the shim of the new state."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    o = orc.oracle()
    try:
        rng = np.random.default_rng(5)
        m = sd.MULTI_CAMERA
        pts = qp.flatten(qp.families(rng, o, desc, so, _cam_rays(scenes, 96, 54, scenes.scaled_K(96), m["pose"]), n=300))
        _check(sp, so, pts, where="upload")
        tris = desc.meshes[1][1].copy()
        tris[:, [0, 3, 6]] += 0.05
        tris[:, [2, 5, 8]] -= 0.03
        sp.refit_mesh(1, tris)
        o.mesh_refit(desc.oracle_meshes[1], tris)
        _check(sp, so, pts, where="refit_mesh")
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        sp.rebuild_mesh(1, new)
        desc2 = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances)
        so2 = desc2.build_oracle(orc)
        so.close()
        so = so2
        _check(sp, so, pts, where="rebuild_mesh")
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        sp.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        with torch.cuda.stream(s):
            got = sp.closest_points(torch.from_numpy(pts).cuda(), outputs=ALL)
        s.synchronize()
        _same({k: v.cpu().numpy() for k, v in got.items()}, point_oracle.closest_points(so, pts), "update_mesh_instance(stream)")
    finally:
        sp.close()
        so.close()


def test_non_finite_points_do_not_disturb_others(rt, orc, scenes, blob5k):
    """Points with NaN / inf components mixed among finite ones: the finite points' results equal an all-finite call's."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(6)
        pts = rng.uniform(-1.5, 1.5, (1000, 3)).astype(np.float32)
        bad = pts.copy()
        sel = rng.random(1000) < 0.3
        bad[sel, rng.integers(0, 3, sel.sum())] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), sel.sum())
        a = sp.closest_points(pts, outputs=ALL)
        b = sp.closest_points(bad, outputs=ALL)
        _same({k: v[~sel] for k, v in b.items()}, {k: v[~sel] for k, v in a.items()}, "finite beside non-finite")
    finally:
        sp.close()


def test_call_shapes(rt, orc, scenes, blob5k):
    """n = 0, n = 1, n not a multiple of 64, a [.., 3] leading shape, unaligned torch views, the numpy path, a non-default stream, and
    a query overlapping a render of the same scene on another stream."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(8)
        pts = rng.uniform(-1.5, 1.5, (1001, 3)).astype(np.float32)
        ref = point_oracle.closest_points(so, pts)
        got = sp.closest_points(pts[:0], outputs=ALL)
        assert all(v.shape[0] == 0 for v in got.values())
        _same(sp.closest_points(pts[:1], outputs=EXACT), {k: v[:1] for k, v in ref.items()}, "n = 1")
        _same(sp.closest_points(pts[:77], outputs=EXACT), {k: v[:77] for k, v in ref.items()}, "n = 77")
        _same(sp.closest_points(pts[:1000].reshape(10, 100, 3), outputs=("distance", "point")),
              {k: v[:1000].reshape((10, 100) + v.shape[1:]) for k, v in ref.items()}, "[10, 100, 3]", keys=("distance", "point"))
        flat = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), pts.ravel()])).cuda()
        view = flat[1:].view(-1, 3)                             # (4 bytes past the allocation's start)
        md = torch.full((1002,), float("inf"), device="cuda")[1:]
        assert view.data_ptr() % 16 != 0
        tg = sp.closest_points(view, md, outputs=EXACT)
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in tg.items()}, ref, "unaligned torch view")
        cam = rt.Camera(640, 360, scenes.scaled_K(640), scenes.D_REF)
        cam.set_pose(sd.MULTI_CAMERA["pose"])
        want = rt.render_ids(sp, cam)
        img = rt.DeviceBuffer(width_bytes=640 * 3, height=360)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        tp = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        assert rt.libs()[0].rt_render(sp.device_handle, cam.params(), img.ptr, img.pitch, s1.cuda_stream, 0) == 0
        tq = sp.closest_points(tp, outputs=EXACT, stream=s2)
        torch.cuda.synchronize()
        _same({k: v.cpu().numpy() for k, v in tq.items()}, ref, "overlapping a render")
        assert np.array_equal(img.to_host().reshape(360, 640, 3), want["img"])
        img.free()
    finally:
        sp.close()
        so.close()


def test_pruning_is_real(rt, orc, scenes, blob70k):
    """Mean pops on c2 surface points (1e-3 of the diagonal off the surface) stays below 0.1 % of c2's interior nodes (measured: 35 of
    about 70 000 on the full 1080p frame, tools/point_query_bench.py)."""
    desc = sd.blob_scene(scenes, blob70k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        org, dirs = _cam_rays(scenes, 160, 90, scenes.scaled_K(160), scenes.C2_CAMERAS["mid"])
        hit = ray_oracle.cast_rays(so, org.reshape(-1, 3), dirs.reshape(-1, 3))
        ok = hit["instance"] >= 0
        lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
        diag = np.float32(np.linalg.norm(hi - lo))
        pts = np.ascontiguousarray((hit["location"][ok] + hit["normal"][ok] * (diag * np.float32(1e-3)))[:3000], np.float32)
        got = sp.closest_points(pts, outputs=ALL)
        _same(got, point_oracle.closest_points(so, pts), "c2 surface")
        interior = int((orc.oracle().mesh_dump(desc.oracle_meshes[0])["child"][:, 0] > 0).sum())
        assert got["pops"].mean() < 0.001 * interior, (got["pops"].mean(), interior)
    finally:
        sp.close()
        so.close()
