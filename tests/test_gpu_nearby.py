"""Nearby-triangle lists on the GPU (Scene.list_nearby through rt_nearby_offsets / rt_list_nearby): every field equals the brute-force
shim (tests/nearby_oracle.c) bit for bit, NaN patterns unified, on the library's and adversarial scenes, under every tree and scene
change, in CSR and fixed rooms with and without count (k-nearest pruning), and nothing outside a room is ever written."""
import ctypes as C

import numpy as np
import pytest

import nearby_oracle as nb
import query_points as qp
import ray_oracle
import scene_defs as sd
from test_gpu_crossings import _bits, _eq
from test_gpu_point_query import SEEDS, _cam_rays, _library_scene, _product

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")


def _bounds(rng, dist, diag):
    """finite per-point radii for the CSR form: multiples of the closest distance, its float neighbours, 0, a fraction of the scene
    diagonal, NaN and negative"""
    n = len(dist)
    d = np.where(dist < np.finfo(F32).max, dist, F32(1.0)).astype(F32)
    kinds = rng.integers(0, 7, n)
    out = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3, kinds == 4, kinds == 5],
                    [d, np.nextafter(d, F32(np.inf)), F32(0.0), F32(diag * 0.02), F32(np.nan), F32(-1.0)],
                    (d * rng.uniform(1.0, 3.0, n) + F32(diag * 1e-3)).astype(F32))
    return np.ascontiguousarray(out, F32)


def _check(sp, so, pts, md=None, kmd=None, where="", ks=(1, 3, 64)):
    """CSR (bound md) and fixed rooms K (bound kmd) against the shim; slot 0 against closest_points; count and offsets; fixed rooms
    with count (pruning by the bound) and without (pruning by the K-th key) identical"""
    if md is not None:
        got = sp.list_nearby(pts, md, outputs=FIELDS + ("pops",))
        ref = nb.list_nearby(so, pts, md)
        for k in FIELDS + ("offsets", "point_index", "count"):
            _eq(got[k], ref[k], "%s CSR %s" % (where, k))
        assert int(got["offsets"][-1]) == int(got["count"].astype(np.int64).sum()) and (got["pops"] >= 0).all()
        cp = sp.closest_points(pts, md, outputs=FIELDS)
        has = got["count"] > 0
        for k in FIELDS:
            _eq(got[k][got["offsets"][:-1][has]], cp[k][has], "%s slot 0 vs closest_points %s" % (where, k))
        assert (cp["instance"][~has] == -1).all(), where
    for K in ks:
        r = nb.list_nearby(so, pts, kmd, max_hits=K)
        g = sp.list_nearby(pts, kmd, max_hits=K, outputs=FIELDS + ("count",))
        g2 = sp.list_nearby(pts, kmd, max_hits=K, outputs=FIELDS)
        assert set(g2) == set(FIELDS)
        for k in FIELDS:
            _eq(g[k], r[k], "%s K=%d %s" % (where, K, k))
            _eq(g2[k], r[k], "%s K=%d without count %s" % (where, K, k))
        _eq(g["count"], r["count"], "%s K=%d count" % (where, K))


def _diag(orc, desc):
    lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
    return float(np.linalg.norm((hi - lo).astype(np.float64)))


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    desc, (W, H, K, pose) = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(17)
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=150))
        dist = sp.closest_points(pts)["distance"]
        _check(sp, so, pts, _bounds(rng, dist, _diag(orc, desc)), qp.special_bounds(rng, dist), where=name)
        _check(sp, so, pts, None, None, where=name + " unbounded", ks=(3,))
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_adversarial_scenes_equal_oracle(rt, orc, scenes, seed):
    desc, W, H, K, pose, info = sd.adversarial_scene(scenes, np.random.default_rng(91000 + seed))
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(seed)
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=120))
        dist = sp.closest_points(pts)["distance"]
        diag = _diag(orc, desc)
        _check(sp, so, pts, _bounds(rng, dist, diag if np.isfinite(diag) else 1.0), qp.special_bounds(rng, dist), where=info,
               ks=(1, 3))
    finally:
        sp.close()
        so.close()


def test_bound_at_pair_distances(rt, orc, scenes, blob5k):
    """max_distance at a listed pair's distance and 1, 2 float steps either side: the pair is in exactly when the bound is not
    below its distance; everything equals the shim."""
    desc, (W, H, K, pose) = _library_scene("multi", scenes, blob5k, None)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(2)
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=100))
        g = sp.list_nearby(pts, max_hits=4)
        pick = rng.integers(0, 4, len(pts))
        d = g["distance"][np.arange(len(pts)), pick]
        ok = d < np.finfo(F32).max
        p, d = np.ascontiguousarray(pts[ok]), d[ok]
        for k in (-2, -1, 0, 1, 2):
            md = np.ascontiguousarray(qp.ulp_steps(d, k), F32)
            _check(sp, so, p, md, md, where="bound %+d ulps" % k, ks=(2,))
    finally:
        sp.close()
        so.close()


def test_trees_and_scene_changes(rt, orc, scenes, blob5k):
    """Host-built, device-built and refitted trees give the same lists; after refit, rebuild and an async instance update on a
    stream the lists equal the shim of the new state."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    a, b, c = _product(rt, desc), _product(rt, desc, for_device=True), _product(rt, desc)
    try:
        for k, (kind, arg) in enumerate(desc.meshes):
            c.refit_mesh(k, arg if kind == "tris" else rt.Mesh.load_obj(arg).dump()["tris"])
        rng = np.random.default_rng(4)
        m = sd.MULTI_CAMERA
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, 96, 54, scenes.scaled_K(96), m["pose"]), n=150))
        md = _bounds(rng, a.closest_points(pts)["distance"], _diag(orc, desc))
        res = [sp.list_nearby(pts, md) for sp in (a, b, c)]
        res8 = [sp.list_nearby(pts, max_hits=8) for sp in (a, b, c)]
        for j, label in ((1, "device tree"), (2, "refitted tree")):
            for k in FIELDS[:3] + ("offsets",):
                _eq(res[j][k], res[0][k], "%s %s" % (label, k))
            for k in FIELDS[:3]:
                _eq(res8[j][k], res8[0][k], "%s K=8 %s" % (label, k))
        _check(a, so, pts, md, None, where="host tree", ks=(8,))
        tris = desc.meshes[1][1].copy()
        tris[:, [0, 3, 6]] += 0.05
        a.refit_mesh(1, tris)
        orc.oracle().mesh_refit(desc.oracle_meshes[1], tris)
        _check(a, so, pts, md, md, where="refit_mesh", ks=(2,))
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        a.rebuild_mesh(1, new)
        so.close()
        so = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances).build_oracle(orc)
        _check(a, so, pts, md, None, where="rebuild_mesh", ks=(2,))
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        a.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        tp, tm = torch.from_numpy(pts).cuda(), torch.from_numpy(md).cuda()
        with torch.cuda.stream(s):
            g = a.list_nearby(tp, tm, outputs=FIELDS)
            g4 = a.list_nearby(tp, max_hits=4, outputs=FIELDS)
        s.synchronize()
        ref, ref4 = nb.list_nearby(so, pts, md), nb.list_nearby(so, pts, max_hits=4)
        for k in FIELDS + ("offsets", "point_index", "count"):
            _eq(g[k].cpu().numpy(), ref[k], "update_mesh_instance(stream) " + k)
        for k in FIELDS:
            _eq(g4[k].cpu().numpy(), ref4[k], "update_mesh_instance(stream) K=4 " + k)
    finally:
        for sp in (a, b, c):
            sp.close()
        so.close()


def _raw(rt, sp, pts, md, offsets, max_hits, slots, fields=FIELDS, with_count=True, guard=0x5A):
    """rt_list_nearby straight through the C-ABI into buffers pre-filled with a guard byte -> (dict of the slot arrays, count)"""
    import torch
    n = len(pts)
    shapes = dict(distance=(), instance=(), triangle=(), point=(3,), normal=(3,), barycentric=(2,), uv=(2,))
    dt = dict(distance=torch.float32, instance=torch.int32, triangle=torch.int32, point=torch.float32, normal=torch.float32,
              barycentric=torch.float32, uv=torch.float32)
    out = {}
    for k in fields:
        b = torch.full((slots * int(np.prod(shapes[k], dtype=np.int64)) * 4,), guard, dtype=torch.uint8, device="cuda")
        out[k] = b.view(dt[k]).reshape((slots,) + shapes[k])
    cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    tp = torch.from_numpy(pts).cuda()
    tm = None if md is None else torch.from_numpy(md).cuda()
    ot = None if offsets is None else torch.from_numpy(offsets).cuda()
    lst = rt.RtNearbyList(*[out[k].data_ptr() if k in out else None for k in FIELDS], cnt.data_ptr() if with_count else None, None)
    h = rt.libs()[0]
    torch.cuda.synchronize()
    rc = h.rt_list_nearby(sp.device_handle, tp.data_ptr(), None if tm is None else tm.data_ptr(), n,
                          None if ot is None else ot.data_ptr(), max_hits, C.byref(lst), None, 1)
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}, cnt.cpu().numpy()


def test_rooms_never_written_outside(rt, orc, scenes, blob5k):
    """Offsets taken with a smaller bound than the fill call truncate each list, rooms are placed with gaps between them (some of 0
    and negative size), and non-finite points and bounds sit between finite ones: every slot outside a room keeps its guard word,
    every finite point's room equals the shim's, and finite points' lists do not depend on the non-finite ones.  Fixed rooms with
    and without count write the same."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        pts = rng.uniform(-1.5, 1.5, (400, 3)).astype(F32)
        md = rng.uniform(0.02, 0.3, 400).astype(F32)
        bad = rng.random(len(pts)) < 0.2
        idx = np.flatnonzero(bad)
        pts[idx[0::4], 0] = np.nan
        pts[idx[1::4], 2] = np.inf
        md[idx[2::4]] = np.nan
        md[idx[3::4]] = np.inf
        md_ok = np.where(np.isfinite(md), md, F32(0.1)).astype(F32)
        small = nb.count_nearby(so, np.where(np.isfinite(pts), pts, F32(0)), md_ok * F32(0.5)).astype(np.int64)
        small[rng.random(len(pts)) < 0.1] = 0                   # (rooms of 0)
        room = small + rng.integers(0, 3, len(pts))
        offsets = np.concatenate([[3], 3 + np.cumsum(room)]).astype(np.int64)
        offsets[-1] = offsets[-2] - 2                           # the last point's room is negative
        slots = int(offsets[-2]) + 5                            # slots 0-2 and the last 5 belong to no room
        fin = ~bad
        got, cnt = _raw(rt, sp, pts, md, offsets, 0, slots)
        ref = nb.rooms(so, np.where(fin[:, None], pts, F32(0)), np.where(fin, md, F32(0)), offsets=offsets, slots=slots)
        inroom = np.zeros(slots, bool)
        for i in range(len(pts)):
            inroom[offsets[i]:max(offsets[i], offsets[i + 1])] = True
        for k in FIELDS:
            outside = got[k][~inroom].reshape(-1)
            guard = np.frombuffer(bytes([0x5A]) * 4, got[k].dtype)[0]
            assert _bits(outside).tolist() == _bits(np.full(outside.shape, guard)).tolist(), "%s: guard changed" % k
            for i in np.flatnonzero(fin):
                a, b = offsets[i], max(offsets[i], offsets[i + 1])
                _eq(got[k][a:b], ref[k][a:b], "point %d %s" % (i, k))
        _eq(cnt[fin], ref["count"][fin], "count")
        for with_count in (True, False):                        # fixed rooms of 5, guarded on both ends
            g, c = _raw(rt, sp, pts, md, None, 5, len(pts) * 5, with_count=with_count)
            r = nb.rooms(so, np.ascontiguousarray(pts[fin]), np.ascontiguousarray(md[fin]), max_hits=5)
            for k in FIELDS:
                _eq(g[k].reshape((len(pts), 5) + g[k].shape[1:])[fin], r[k].reshape((fin.sum(), 5) + r[k].shape[1:]),
                    "fixed K=5 (count %s) %s" % (with_count, k))
            assert (c[fin] == r["count"]).all() if with_count else (c == -9).all()
        g1 = sp.list_nearby(pts, md, max_hits=3, outputs=FIELDS + ("count",))
        g2 = sp.list_nearby(np.ascontiguousarray(pts[fin]), np.ascontiguousarray(md[fin]), max_hits=3, outputs=FIELDS + ("count",))
        for k in FIELDS + ("count",):
            _eq(g1[k][fin], g2[k], "finite points beside non-finite " + k)
    finally:
        sp.close()
        so.close()


def test_fan_of_thousand_triangles(rt, orc):
    """1200 triangles sharing one vertex (a fan, in shuffled order): points at and near the apex are within reach of all of them,
    many at one distance -- the worst case of the insertion; CSR and fixed rooms of 1, 64 and 2000 equal the shim."""
    o_ = orc.oracle()
    rng = np.random.default_rng(3)
    ang = rng.permutation(1200).astype(np.float64) * (2 * np.pi / 1200)
    tris = []
    for a0 in ang:
        a1 = a0 + 2 * np.pi / 1200
        v = np.array([(0, 0, 0), (np.cos(a0), np.sin(a0), 0.1 * np.sin(3 * a0)), (np.cos(a1), np.sin(a1), 0.1 * np.sin(3 * a1))], F32)
        tris.append(np.asarray(o_.tri_from_vertices(v.ravel()), F32))
    desc = sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", np.stack(tris))], [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        pts = np.concatenate([np.zeros((64, 3)), rng.normal(scale=1e-3, size=(64, 3)), [[0, 0, 0.5]] * 8]).astype(F32)
        md = np.full(len(pts), 2.0, F32)
        _check(sp, so, pts, md, md, where="fan", ks=(1, 64, 2000))
        g = sp.list_nearby(pts, md)
        assert (g["count"] == 1200).all()
    finally:
        sp.close()
        so.close()


def test_call_shapes(rt, orc, scenes, blob5k):
    """n = 0, all points missing (total 0), a [10, 100, 3] leading shape, output subsets, numpy against torch, torch on a side
    stream."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(8)
        pts = rng.uniform(-1.5, 1.5, (1000, 3)).astype(F32)
        md = rng.uniform(0.0, 0.2, 1000).astype(F32)
        ref = nb.list_nearby(so, pts, md)
        g = sp.list_nearby(pts[:0], md[:0])
        assert g["offsets"].tolist() == [0] and all(g[k].shape[0] == 0 for k in ("distance", "instance", "triangle", "point_index", "count"))
        g = sp.list_nearby(pts[:0], max_hits=2, outputs=("distance", "point"))
        assert g["distance"].shape == (0, 2) and g["point"].shape == (0, 2, 3)
        far = np.full((70, 3), 50.0, F32)
        g = sp.list_nearby(far, md[:70])
        assert g["offsets"].tolist() == [0] * 71 and g["distance"].shape == (0,) and (g["count"] == 0).all()
        g = sp.list_nearby(pts.reshape(10, 100, 3), md.reshape(10, 100), max_hits=3, outputs=("distance", "normal", "count"))
        assert set(g) == {"distance", "normal", "count"} and g["distance"].shape == (10, 100, 3) and g["normal"].shape == (10, 100, 3, 3)
        r3 = nb.list_nearby(so, pts, md, max_hits=3)
        _eq(g["distance"], r3["distance"].reshape(10, 100, 3), "[10, 100, 3] distance")
        _eq(g["count"], ref["count"].reshape(10, 100), "[10, 100, 3] count")
        g = sp.list_nearby(pts, md, outputs=("uv", "instance"))
        assert set(g) == {"uv", "instance", "offsets", "point_index", "count"}
        _eq(g["uv"], ref["uv"], "uv only")
        tp, tm = torch.from_numpy(pts).cuda(), torch.from_numpy(md).cuda()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        gt = sp.list_nearby(tp, tm, outputs=FIELDS, stream=s)
        gk = sp.list_nearby(tp, max_hits=2, outputs=FIELDS + ("count", "pops"), stream=s)
        s.synchronize()
        assert gt["offsets"].dtype == torch.int64 and gt["point_index"].dtype == torch.int32 and gt["count"].dtype == torch.int32
        for k in FIELDS + ("offsets", "point_index", "count"):
            _eq(gt[k].cpu().numpy(), ref[k], "torch side stream " + k)
        r2 = nb.list_nearby(so, pts, max_hits=2)
        for k in FIELDS + ("count",):
            _eq(gk[k].cpu().numpy(), r2[k], "torch side stream K=2 " + k)
        assert (gk["pops"].cpu().numpy() >= 0).all()
        g = sp.list_nearby(tp, max_hits=1)
        cp = sp.closest_points(tp)
        torch.cuda.synchronize()
        for k in ("distance", "instance", "triangle"):
            _eq(g[k][:, 0].cpu().numpy(), cp[k].cpu().numpy(), "K=1 vs closest_points " + k)
    finally:
        sp.close()
        so.close()


def test_pruning_is_real(rt, orc, scenes, blob70k):
    """On c2 surface points (1e-3 of the diagonal off the surface): a radius of 2e-3 of the diagonal visits under 0.1 % of c2's
    interior nodes per point; with no radius, max_hits = 8 without count (pruning by the 8th key) visits strictly fewer nodes in total
    than with count, and the rooms are identical."""
    desc = sd.blob_scene(scenes, blob70k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        org, dirs = _cam_rays(scenes, 160, 90, scenes.scaled_K(160), scenes.C2_CAMERAS["mid"])
        hit = ray_oracle.cast_rays(so, org.reshape(-1, 3), dirs.reshape(-1, 3))
        ok = hit["instance"] >= 0
        lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
        diag = np.float32(np.linalg.norm(hi - lo))
        pts = np.ascontiguousarray((hit["location"][ok] + hit["normal"][ok] * (diag * np.float32(1e-3)))[:3000], F32)
        md = np.full(len(pts), diag * F32(2e-3), F32)
        got = sp.list_nearby(pts, md, outputs=FIELDS + ("pops",))
        ref = nb.list_nearby(so, pts[:300], md[:300])
        for k in FIELDS:
            _eq(got[k][:ref["offsets"][-1]], ref[k], "c2 radius " + k)
        interior = int((orc.oracle().mesh_dump(desc.oracle_meshes[0])["child"][:, 0] > 0).sum())
        assert got["pops"].mean() < 0.001 * interior, (got["pops"].mean(), interior)
        a = sp.list_nearby(pts, max_hits=8, outputs=FIELDS + ("count", "pops"))
        b = sp.list_nearby(pts, max_hits=8, outputs=FIELDS + ("pops",))
        for k in FIELDS:
            _eq(b[k], a[k], "K=8 with and without count " + k)
        assert (a["count"] == a["count"][0]).all() and a["count"][0] > 8       # (unbounded: every triangle is a pair)
        assert b["pops"].astype(np.int64).sum() < a["pops"].astype(np.int64).sum(), (b["pops"].sum(), a["pops"].sum())
        r8 = nb.list_nearby(so, pts[:100], max_hits=8)
        for k in FIELDS:
            _eq(b[k][:100], r8[k], "K=8 vs shim " + k)
    finally:
        sp.close()
        so.close()
