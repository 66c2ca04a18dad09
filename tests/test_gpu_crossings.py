"""Crossing counts, winding numbers and signed distance on the GPU (Scene.count_crossings / winding_numbers / signed_distance through
rt_count_crossings / rt_winding_numbers / rt_signed_distance): every exact output equals the brute-force shim over the test oracle's
scene (tests/crossing_oracle.c) -- integers exactly, the signed distance bit for bit -- on the library's scenes, the adversarial
scenes of scene_defs.adversarial_scene, at the tmax boundaries, under every tree, after scene changes and under every call shape.
`pops` is only bounded."""
import numpy as np
import pytest

import crossing_oracle as xo
import point_oracle
import query_points as qp
import query_rays as qr
import ray_oracle
import scene_defs as sd

pytestmark = pytest.mark.gpu
F32 = np.float32
SEEDS = [0, 1, 2, 3, 4, 5, 6, 7, 9, 12, 17, 23]


def _bits(a):
    """bit patterns, every NaN one pattern (test_gpu_point_query._bits)"""
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return a
    return np.where(np.isnan(a), np.float32(np.nan), a).astype(np.float32).view(np.uint32)


def _eq(got, ref, where):
    g, r = _bits(np.asarray(got)), _bits(np.asarray(ref))
    assert g.shape == r.shape, (where, g.shape, r.shape)
    bad = np.flatnonzero(g.reshape(-1) != r.reshape(-1))
    assert bad.size == 0, "%s: %d differ, first %s: got %s want %s" % (where, bad.size, bad[:4], np.asarray(got).reshape(-1)[bad[:4]],
                                                                        np.asarray(ref).reshape(-1)[bad[:4]])


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


def _cam(scenes, W, H, pose):
    o, d = ray_oracle.camera_rays(W, H, scenes.scaled_K(W), scenes.D_REF, pose)
    return np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))


def _check_rays(sp, so, o, d, tmax=None, where=""):
    got = sp.count_crossings(o, d, tmax, outputs=("count", "winding", "pops"))
    ref = xo.count_crossings(so, o, d, tmax)
    _eq(got["count"], ref["count"], where + " count")
    _eq(got["winding"], ref["winding"], where + " winding")
    assert (got["pops"] >= 0).all(), where
    return got, ref


def _check_points(sp, so, pts, md=None, where=""):
    w = sp.winding_numbers(pts)
    _eq(w, xo.winding_numbers(so, pts), where + " winding_numbers")
    sdf = sp.signed_distance(pts, md)
    d = sp.closest_points(pts, md)["distance"]
    _eq(sdf, np.where(w != 0, -d, d).astype(F32), where + " sdf vs closest_points")
    _eq(sdf, xo.signed_distance(so, pts, md), where + " sdf vs shim")
    return w, sdf


def _segments(rng, pts, n):
    a = pts[rng.integers(0, len(pts), n)]
    b = pts[rng.integers(0, len(pts), n)]
    return np.ascontiguousarray(a, F32), np.ascontiguousarray((b - a).astype(F32)), np.ones(n, F32)


def _library_scene(name, scenes, blob5k, atrium, demo_objs):
    if name == "c1":
        return sd.c1_scene(scenes), scenes.C1["cam_pose"]
    if name == "blob":
        return sd.blob_scene(scenes, blob5k), scenes.C2_CAMERAS["mid"]
    if name == "multi":
        return sd.multi_instance_scene(scenes, blob5k), sd.MULTI_CAMERA["pose"]
    if name == "atrium":
        return sd.atrium_scene(scenes, atrium), scenes.C4["cam_pose"]
    if name == "demo":
        return sd.demo_scene(scenes, demo_objs), scenes.DEMO["cam_pose"]
    return sd.deep_stack_scene(28), (0.0, -1.0, 0.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("name", ["c1", "blob", "multi", "atrium", "deep", "demo"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, atrium, demo_objs, name):
    """Camera rays, the ray-query families, segments between pairs of the point-query families' points (tmax = 1), and the point
    entry points on those points: equal to the shim."""
    desc, pose = _library_scene(name, scenes, blob5k, atrium, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(11)
        co, cd = _cam(scenes, 48, 27, pose)
        _check_rays(sp, so, co, cd, where=name + " camera")
        o, d = qr.flatten(qr.families(rng, so, (co, cd), n=120 if name == "atrium" else 300))
        _check_rays(sp, so, o, d, where=name + " families")
        _check_rays(sp, so, o, d, qr.special_tmax(rng, len(o)), where=name + " families, special tmax")
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, (co, cd), n=80 if name == "atrium" else 200))
        _check_rays(sp, so, *_segments(rng, pts, 1000), where=name + " segments")
        _check_points(sp, so, pts, where=name + " points")
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_adversarial_scenes_equal_oracle(rt, orc, scenes, seed):
    """The render fuzz's adversarial scenes (lattices, degenerate and needle triangles, piles above 30 per leaf, 1e18 and 1e-20
    coordinates, non-finite vertices; mirrored, tiny and huge scales): rays, segments and points equal to the shim."""
    desc, W, H, K, pose, info = sd.adversarial_scene(scenes, np.random.default_rng(91000 + seed))
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(seed)
        cam = ray_oracle.camera_rays(W, H, K, scenes.D_REF, pose)
        o, d = qr.flatten(qr.families(rng, so, cam, n=250))
        _check_rays(sp, so, o, d, where=info)
        _check_rays(sp, so, o, d, qr.special_tmax(rng, len(o)), where=info + " special tmax")
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, cam, n=150))
        _check_rays(sp, so, *_segments(rng, pts, 800), where=info + " segments")
        _check_points(sp, so, pts, qp.special_bounds(rng, sp.closest_points(pts)["distance"]), where=info)
    finally:
        sp.close()
        so.close()


def test_underflowed_edge_functions(rt, orc):
    """A triangle 2^-15 beside the ray's line whose edge functions underflow in fp32 (-2^-150, 2^-136, 2^-136 in fp64) is not counted,
    and its mirror image across the line is: the fp64 fallback keeps the signs, so the shim and the pruned traversal agree.  Each
    sits alone in a leaf of a mesh of 40 triangles far away, so its own box is tested (and rejected when it misses)."""
    o_ = orc.oracle()
    e, h = 2.0 ** -15, 2.0 ** -136
    far = sd.random_triangles(40, seed=21, spread=1.0, size=0.3)
    far[:, [0, 3, 6]] += 8.0
    meshes = []
    for sx in (-1.0, 1.0):
        tri = np.asarray(o_.tri_from_vertices(np.array([-1, 0, 1, sx * e, h, 1, sx * e, -h, 1], F32)), F32)[None]
        meshes.append(("tris", np.concatenate([tri, far]).astype(F32)))
    desc = sd.SceneDesc([((1.0, 1.0, 1.0), None)], meshes,
                        [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (1, 0, (0.0, 3.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        o = np.array([[0, 0, 0], [0, 3, 0], [0, 0, 2], [0, 3, 2], [0, 0, 0], [0, 3, 0]], F32)
        d = np.array([[0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 0, -1], [0, 0, 3], [0, 0, 3]], F32)
        got, ref = _check_rays(sp, so, o, d, where="underflowed edge functions")
        assert ref["count"].tolist() == [0, 1, 0, 1, 0, 1]
        got, ref = _check_rays(sp, so, np.repeat(o, 64, axis=0), np.repeat(d, 64, axis=0), where="underflowed, whole waves")
    finally:
        sp.close()
        so.close()


def test_tmax_at_counted_t(rt, orc, scenes, blob5k):
    """tmax set to every counted t of a ray and to its float neighbours (query_points.ulp_steps): the crossing at t counts exactly
    when t <= tmax."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        co, cd = _cam(scenes, 32, 18, sd.MULTI_CAMERA["pose"])
        rng = np.random.default_rng(2)
        pick = rng.choice(len(co), 300, replace=False)
        o, d, tm = [], [], []
        for j in pick:
            for t in xo.crossing_ts(so, co[j], cd[j]):
                for k in (-2, -1, 0, 1, 2):
                    o.append(co[j]); d.append(cd[j]); tm.append(qp.ulp_steps(t, k))
        o, d, tm = (np.ascontiguousarray(np.asarray(a), F32) for a in (o, d, tm))
        assert len(o) > 400
        _check_rays(sp, so, o, d, tm, where="tmax at counted t")
    finally:
        sp.close()
        so.close()


def test_tree_independence(rt, orc, scenes, blob5k):
    """The host-built tree, a tree built on the device (num_nodes = 0) and the host trees of every mesh refitted to the same vertices
    give identical counts, windings and signed distances.  The two builders make the same tree node for node
    (test_gpu_bvh_build_matches_host_builder) and a refit to the same vertices changes no box, so these are three ways to one tree
    on the device, not three trees: trees the library does not build are tests/test_gpu_caller_trees.py's."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    a, b, c = _product(rt, desc), _product(rt, desc, for_device=True), _product(rt, desc)
    try:
        for k, (kind, arg) in enumerate(desc.meshes):              # every mesh, the OBJ ones with the triangles they loaded
            c.refit_mesh(k, arg if kind == "tris" else rt.Mesh.load_obj(arg).dump()["tris"])
        rng = np.random.default_rng(4)
        co, cd = _cam(scenes, 48, 27, sd.MULTI_CAMERA["pose"])
        o, d = qr.flatten(qr.families(rng, so, (co, cd), n=300))
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, (co, cd), n=200))
        res = []
        for sp in (a, b, c):
            g = sp.count_crossings(o, d)
            res.append((g["count"], g["winding"], sp.winding_numbers(pts), sp.signed_distance(pts)))
        for other, label in ((res[1], "device tree"), (res[2], "refitted tree")):
            for x, y, what in zip(res[0], other, ("count", "winding", "winding_numbers", "sdf")):
                _eq(y, x, "%s %s" % (label, what))
        ref = xo.count_crossings(so, o, d)
        _eq(res[0][0], ref["count"], "host tree vs shim")
    finally:
        for sp in (a, b, c):
            sp.close()
        so.close()


def test_queries_follow_scene_changes(rt, orc, scenes, blob5k):
    """After refit_mesh, rebuild_mesh and an async update_mesh_instance on a stream, results equal the shim of the new state."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    o_ = orc.oracle()
    try:
        rng = np.random.default_rng(5)
        co, cd = _cam(scenes, 48, 27, sd.MULTI_CAMERA["pose"])
        o, d = qr.flatten(qr.families(rng, so, (co, cd), n=200))
        pts = qp.flatten(qp.families(rng, o_, desc, so, (co, cd), n=150))
        _check_rays(sp, so, o, d, where="upload")
        tris = desc.meshes[1][1].copy()
        tris[:, [0, 3, 6]] += 0.05
        tris[:, [2, 5, 8]] -= 0.03
        sp.refit_mesh(1, tris)
        o_.mesh_refit(desc.oracle_meshes[1], tris)
        _check_rays(sp, so, o, d, where="refit_mesh")
        _check_points(sp, so, pts, where="refit_mesh")
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        sp.rebuild_mesh(1, new)
        desc2 = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances)
        so2 = desc2.build_oracle(orc)
        so.close()
        so = so2
        _check_rays(sp, so, o, d, where="rebuild_mesh")
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        sp.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        with torch.cuda.stream(s):
            g = sp.count_crossings(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
            w = sp.winding_numbers(torch.from_numpy(pts).cuda())
        s.synchronize()
        ref = xo.count_crossings(so, o, d)
        _eq(g["count"].cpu().numpy(), ref["count"], "update_mesh_instance(stream) count")
        _eq(g["winding"].cpu().numpy(), ref["winding"], "update_mesh_instance(stream) winding")
        _eq(w.cpu().numpy(), xo.winding_numbers(so, pts), "update_mesh_instance(stream) winding_numbers")
    finally:
        sp.close()
        so.close()


def test_blob_winding_numbers_and_signed_distance(rt, orc, scenes, blob70k):
    """On points in blob70k's box: winding numbers are 0 or 1, equal to the shim, 0 outside the box; the signed distance is bit for
    bit where(winding != 0, -d, d) with d from closest_points (also under max_distance), and negative on points sampled inside."""
    desc = sd.blob_scene(scenes, blob70k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
        rng = np.random.default_rng(6)
        pts = (lo + (hi - lo) * rng.uniform(-0.15, 1.15, (3000, 3))).astype(F32)
        w, sdf = _check_points(sp, so, pts, where="blob70k")
        assert set(np.unique(w)) <= {0, 1} and 0 < (w == 1).sum() < len(w)
        out = ((pts < lo) | (pts > hi)).any(axis=1)
        assert (w[out] == 0).all()
        md = qp.special_bounds(rng, np.abs(sdf))
        _check_points(sp, so, pts, md, where="blob70k bounded")
        inner = (lo + hi) * F32(0.5) + (rng.uniform(-0.15, 0.15, (500, 3)) * (hi - lo)).astype(F32)
        inner = inner.astype(F32)
        assert (sp.signed_distance(inner) < 0).all()
    finally:
        sp.close()
        so.close()


def test_non_finite_inputs_do_not_disturb_others(rt, orc, scenes, blob5k):
    """Rays and points with NaN / inf components beside finite ones: the finite ones' results equal an all-finite call's."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        o = rng.uniform(-1.5, 1.5, (1000, 3)).astype(F32)
        d = rng.normal(size=(1000, 3)).astype(F32)
        sel = rng.random(1000) < 0.3
        bo, bd = o.copy(), d.copy()
        bad = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), sel.sum())
        which = rng.integers(0, 2, sel.sum())
        bo[np.flatnonzero(sel)[which == 0], rng.integers(0, 3, (which == 0).sum())] = bad[which == 0]
        bd[np.flatnonzero(sel)[which == 1], rng.integers(0, 3, (which == 1).sum())] = bad[which == 1]
        a, b = sp.count_crossings(o, d, outputs=("count", "winding")), sp.count_crossings(bo, bd, outputs=("count", "winding"))
        for k in ("count", "winding"):
            _eq(b[k][~sel], a[k][~sel], "finite rays beside non-finite " + k)
        _eq(sp.winding_numbers(bo)[~sel], sp.winding_numbers(o)[~sel], "finite points beside non-finite")
        _eq(sp.signed_distance(bo)[~sel], sp.signed_distance(o)[~sel], "finite sdf beside non-finite")
    finally:
        sp.close()


def test_call_shapes(rt, orc, scenes, blob5k):
    """n = 0, n = 1, n not a multiple of 64, a [.., 3] leading shape, output subsets, the numpy and torch paths, a side stream."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(8)
        o = rng.uniform(-1.5, 1.5, (1001, 3)).astype(F32)
        d = rng.normal(size=(1001, 3)).astype(F32)
        ref = xo.count_crossings(so, o, d)
        wref = xo.winding_numbers(so, o)
        sref = xo.signed_distance(so, o)
        g = sp.count_crossings(o[:0], d[:0], outputs=("count", "winding", "pops"))
        assert all(v.shape == (0,) for v in g.values())
        assert sp.winding_numbers(o[:0]).shape == (0,) and sp.signed_distance(o[:0]).shape == (0,)
        for n in (1, 77):
            g = sp.count_crossings(o[:n], d[:n])
            _eq(g["count"], ref["count"][:n], "n = %d count" % n)
            _eq(g["winding"], ref["winding"][:n], "n = %d winding" % n)
            _eq(sp.winding_numbers(o[:n]), wref[:n], "n = %d winding_numbers" % n)
            _eq(sp.signed_distance(o[:n]), sref[:n], "n = %d sdf" % n)
        g = sp.count_crossings(o[:1000].reshape(10, 100, 3), d[:1000].reshape(10, 100, 3), outputs=("winding",))
        assert list(g) == ["winding"] and g["winding"].shape == (10, 100)
        _eq(g["winding"], ref["winding"][:1000].reshape(10, 100), "[10, 100, 3]")
        assert set(sp.count_crossings(o, d, outputs=("pops",))) == {"pops"}
        _eq(sp.winding_numbers(o[:1000].reshape(10, 100, 3)), wref[:1000].reshape(10, 100), "points [10, 100, 3]")
        to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        g = sp.count_crossings(to, td, torch.full((1001,), float("inf"), device="cuda"), stream=s)
        w = sp.winding_numbers(to, stream=s)
        sd_ = sp.signed_distance(to, torch.full((1001,), float("inf"), device="cuda"), stream=s)
        s.synchronize()
        _eq(g["count"].cpu().numpy(), ref["count"], "torch side stream count")
        _eq(g["winding"].cpu().numpy(), ref["winding"], "torch side stream winding")
        _eq(w.cpu().numpy(), wref, "torch side stream winding_numbers")
        _eq(sd_.cpu().numpy(), sref, "torch side stream sdf")
        g = sp.count_crossings(to, td)
        torch.cuda.synchronize()
        _eq(g["winding"].cpu().numpy(), ref["winding"], "torch current stream")
    finally:
        sp.close()
        so.close()


def test_pruning_is_real(rt, orc, scenes, blob70k):
    """Mean pops of c2 camera rays in count_crossings stays below 1 % of c2's interior nodes (measured: 64.9 of about 70 000 on the
    full 1080p frame, against 31.8 for trace_rays on the same rays, tools/crossing_bench.py), and the counts equal the shim."""
    desc = sd.blob_scene(scenes, blob70k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        o, d = _cam(scenes, 160, 90, scenes.C2_CAMERAS["mid"])
        got, _ref = _check_rays(sp, so, o, d, where="c2 camera")
        interior = int((orc.oracle().mesh_dump(desc.oracle_meshes[0])["child"][:, 0] > 0).sum())
        assert got["pops"].mean() < 0.01 * interior, (got["pops"].mean(), interior)
    finally:
        sp.close()
        so.close()
