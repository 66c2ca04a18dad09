"""Triangle intersection queries on the GPU (Scene.count_intersecting / Scene.list_intersecting through rt_count_intersecting /
rt_intersecting_offsets / rt_list_intersecting): every field equals the brute-force shim (tests/tri_intersect_oracle.c) bit for bit, NaN
patterns unified, on the library's and adversarial scenes, under every tree and scene change, in CSR and fixed rooms with and without
count, with skip_instance, and nothing outside a room is ever written."""
import ctypes as C

import numpy as np
import pytest

import query_points as qp
import ray_oracle
import scene_defs as sd
import tri_intersect_oracle as ti
from test_gpu_crossings import _bits, _eq
from test_gpu_point_query import SEEDS, _cam_rays, _library_scene, _product

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("instance", "triangle", "normal", "segment")


def _rot(rng, deg):
    """a random rotation of `deg` degrees (float64 [3, 3])"""
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    a = np.radians(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def families(rng, o, desc, n=120):
    """-> list of (name, world triangles [m, 3, 3] float32), all finite.  o: orc.oracle(); desc after desc.build_oracle."""
    lo, hi = qp.scene_box(o, desc, desc.oracle_meshes)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-3)
    own = []
    for mesh, _mat, pose, scale in desc.instances:
        t = o.mesh_dump(desc.oracle_meshes[mesh])["tris"][:, :9].reshape(-1, 3, 3)
        t = t[np.isfinite(t).all(axis=(1, 2))]
        if len(t):
            t = t[rng.choice(len(t), min(len(t), n // 3), replace=False)]
            own.append(qp._world(o, pose, scale, t.reshape(-1, 3)).reshape(-1, 3, 3))
    fams = []
    if own:
        w = np.concatenate(own).astype(np.float64)
        w = w[np.isfinite(w).all(axis=(1, 2)) & (np.abs(w) < 1e30).all(axis=(1, 2))]
    if own and len(w):
        c = w.mean(axis=1, keepdims=True)
        moved = np.stack([(x - cc) @ _rot(rng, rng.uniform(1, 6)).T + cc + rng.normal(size=3) * 1e-2 * diag for x, cc in zip(w, c)])
        fams.append(("own_moved", moved))
        fams.append(("own_exact", w))
        # a vertex, then an edge, placed exactly on scene vertices
        far = w[:, :1] + rng.normal(size=(len(w), 2, 3)) * 0.05 * diag
        fams.append(("on_vertex", np.concatenate([w[:, :1], far], axis=1)))
        fams.append(("on_edge", np.concatenate([w[:, :2], w[:, 2:] + rng.normal(size=(len(w), 1, 3)) * 0.05 * diag], axis=1)))
    span = np.maximum(hi - lo, 1e-3)
    cen = lo + span * rng.uniform(-0.1, 1.1, (n, 1, 3))
    size = diag * 10.0 ** rng.uniform(-4, np.log10(0.5), (n, 1, 1))
    fams.append(("random", cen + rng.normal(size=(n, 3, 3)) * size))
    a = lo + span * rng.uniform(0, 1, (n // 4, 1, 3))
    d = rng.normal(size=(n // 4, 1, 3)) * 0.3 * diag
    fams.append(("slivers", np.concatenate([a, a + d, a + d * 0.5 + rng.normal(size=(n // 4, 1, 3)) * 1e-6 * diag], axis=1)))
    fams.append(("points", np.repeat(lo + span * rng.uniform(0, 1, (n // 8, 1, 3)), 3, axis=1)))
    mid = (lo + hi) * 0.5
    fams.append(("huge", mid + rng.normal(size=(n // 8, 3, 3)) * 2 * diag))
    out = [(k, np.ascontiguousarray(v, F32)) for k, v in fams if len(v)]
    return [(k, v[np.isfinite(v).all(axis=(1, 2))]) for k, v in out]


def _flat(fams):
    return np.ascontiguousarray(np.concatenate([f[1] for f in fams]), F32)


def _check(sp, so, tris, skip=None, where="", ks=(1, 3, 64)):
    """CSR and fixed rooms K against the shim; count, any and pops; offsets; fixed rooms with and without count identical"""
    got = sp.list_intersecting(tris, skip, outputs=FIELDS + ("pops",))
    ref = ti.list_intersecting(so, tris, skip)
    for k in FIELDS + ("offsets", "query_index", "count"):
        _eq(got[k], ref[k], "%s CSR %s" % (where, k))
    assert int(got["offsets"][-1]) == int(ref["count"].astype(np.int64).sum()) and (got["pops"] >= 0).all()
    c = sp.count_intersecting(tris, skip, outputs=("count", "any", "pops"))
    _eq(c["count"], ref["count"], where + " count_intersecting")
    assert c["any"].dtype == np.bool_ and np.array_equal(c["any"], ref["count"] > 0), where
    a = sp.count_intersecting(tris, skip, outputs=("any", "pops"))
    assert np.array_equal(a["any"], ref["count"] > 0), where + " any only"
    assert (a["pops"] <= c["pops"]).all(), where + " pops(any only) <= pops(count)"
    for K in ks:
        r = ti.list_intersecting(so, tris, skip, max_hits=K)
        g = sp.list_intersecting(tris, skip, max_hits=K, outputs=FIELDS + ("count",))
        g2 = sp.list_intersecting(tris, skip, max_hits=K, outputs=FIELDS)
        assert set(g2) == set(FIELDS)
        for k in FIELDS:
            _eq(g[k], r[k], "%s K=%d %s" % (where, K, k))
            _eq(g2[k], r[k], "%s K=%d without count %s" % (where, K, k))
        _eq(g["count"], r["count"], "%s K=%d count" % (where, K))
    return ref


def test_full_traversals_visit_the_same_nodes(rt, orc, scenes, blob5k):
    """The count call, the CSR list call and the fixed-room list call with count all visit every pair of every instance, so their
    pops are equal element-wise (one full wave and a single-lane wave)."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(65)
        tris = _flat(families(rng, orc.oracle(), desc))
        tris = np.ascontiguousarray(tris[rng.choice(len(tris), 65, replace=False)])
        c = sp.count_intersecting(tris, outputs=("count", "pops"))
        assert (c["count"] > 3).any() and c["pops"].max() > 0
        _eq(sp.list_intersecting(tris, outputs=FIELDS + ("pops",))["pops"], c["pops"], "pops(CSR list) == pops(count)")
        _eq(sp.list_intersecting(tris, max_hits=3, outputs=FIELDS + ("count", "pops"))["pops"], c["pops"], "pops(K=3 with count) == pops(count)")
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    desc, _cam = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(23)
        tris = _flat(families(rng, orc.oracle(), desc))
        ref = _check(sp, so, tris, where=name)
        assert (ref["count"] > 0).sum() > 10, name
        skip = rng.integers(-1, len(desc.instances), len(tris)).astype(np.int32)
        _check(sp, so, tris, skip, where=name + " skip_instance", ks=(3,))
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
        _check(sp, so, _flat(families(rng, orc.oracle(), desc, n=90)), where=info, ks=(1, 3))
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
        tris = _flat(families(rng, orc.oracle(), desc))
        res = [sp.list_intersecting(tris, outputs=FIELDS) for sp in (a, b, c)]
        res8 = [sp.list_intersecting(tris, max_hits=8, outputs=FIELDS) for sp in (a, b, c)]
        for j, label in ((1, "device tree"), (2, "refitted tree")):
            for k in FIELDS + ("offsets",):
                _eq(res[j][k], res[0][k], "%s %s" % (label, k))
            for k in FIELDS:
                _eq(res8[j][k], res8[0][k], "%s K=8 %s" % (label, k))
        _check(a, so, tris, where="host tree", ks=(8,))
        new_tris = desc.meshes[1][1].copy()
        new_tris[:, [0, 3, 6]] += 0.05
        a.refit_mesh(1, new_tris)
        orc.oracle().mesh_refit(desc.oracle_meshes[1], new_tris)
        _check(a, so, tris, where="refit_mesh", ks=(2,))
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        a.rebuild_mesh(1, new)
        so.close()
        so = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances).build_oracle(orc)
        _check(a, so, tris, where="rebuild_mesh", ks=(2,))
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        a.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        tt = torch.from_numpy(tris).cuda()
        with torch.cuda.stream(s):
            g = a.list_intersecting(tt, outputs=FIELDS)
            g4 = a.list_intersecting(tt, max_hits=4, outputs=FIELDS)
            gc = a.count_intersecting(tt, outputs=("count", "any"))
        s.synchronize()
        ref, ref4 = ti.list_intersecting(so, tris), ti.list_intersecting(so, tris, max_hits=4)
        for k in FIELDS + ("offsets", "query_index", "count"):
            _eq(g[k].cpu().numpy(), ref[k], "update_mesh_instance(stream) " + k)
        for k in FIELDS:
            _eq(g4[k].cpu().numpy(), ref4[k], "update_mesh_instance(stream) K=4 " + k)
        _eq(gc["count"].cpu().numpy(), ref["count"], "update_mesh_instance(stream) count")
        assert gc["any"].dtype == torch.bool and np.array_equal(gc["any"].cpu().numpy(), ref["count"] > 0)
    finally:
        for sp in (a, b, c):
            sp.close()
        so.close()


def _raw(rt, sp, tris, offsets, max_hits, slots, with_count=True, guard=0x5A):
    """rt_list_intersecting straight through the C-ABI into buffers pre-filled with a guard byte -> (dict of the slot arrays, count)"""
    import torch
    n = len(tris)
    shapes = dict(instance=(), triangle=(), normal=(3,), segment=(2, 3))
    dt = dict(instance=torch.int32, triangle=torch.int32, normal=torch.float32, segment=torch.float32)
    out = {}
    for k in FIELDS:
        b = torch.full((slots * int(np.prod(shapes[k], dtype=np.int64)) * 4,), guard, dtype=torch.uint8, device="cuda")
        out[k] = b.view(dt[k]).reshape((slots,) + shapes[k])
    cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    tt = torch.from_numpy(tris).cuda()
    ot = None if offsets is None else torch.from_numpy(offsets).cuda()
    lst = rt.RtIntersectList(*[out[k].data_ptr() for k in FIELDS], cnt.data_ptr() if with_count else None, None)
    h = rt.libs()[0]
    torch.cuda.synchronize()
    rc = h.rt_list_intersecting(sp.device_handle, tt.data_ptr(), None, n, None if ot is None else ot.data_ptr(), max_hits, C.byref(lst),
                                None, 1)
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}, cnt.cpu().numpy()


def test_rooms_never_written_outside(rt, orc, scenes, blob5k):
    """Rooms sized below each count truncate, gaps lie between them (some rooms of 0 and a negative one), and non-finite triangles
    sit between finite ones: every slot outside a room keeps its guard word, every finite query's room equals the shim's, and finite
    queries' results do not depend on the non-finite ones.  Fixed rooms with and without count write the same."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        tris = _flat(families(rng, orc.oracle(), desc, n=150))
        bad = rng.random(len(tris)) < 0.2
        idx = np.flatnonzero(bad)
        tris[idx[0::3], 0, 0] = np.nan
        tris[idx[1::3], 1, 2] = np.inf
        tris[idx[2::3]] = -np.inf
        fin = ~bad
        full = ti.count_intersecting(so, np.where(fin[:, None, None], tris, F32(0))).astype(np.int64)
        room = np.maximum(full - rng.integers(0, 3, len(tris)), 0) + rng.integers(0, 2, len(tris))
        room[rng.random(len(tris)) < 0.1] = 0
        offsets = np.concatenate([[3], 3 + np.cumsum(room)]).astype(np.int64)
        offsets[-1] = offsets[-2] - 2                           # the last query's room is negative
        slots = int(offsets[-2]) + 5                            # slots 0-2 and the last 5 belong to no room
        got, cnt = _raw(rt, sp, tris, offsets, 0, slots)
        ref = ti.rooms(so, np.where(fin[:, None, None], tris, F32(0)), offsets=offsets, slots=slots)
        inroom = np.zeros(slots, bool)
        for i in range(len(tris)):
            inroom[offsets[i]:max(offsets[i], offsets[i + 1])] = True
        for k in FIELDS:
            outside = got[k][~inroom].reshape(-1)
            guard = np.frombuffer(bytes([0x5A]) * 4, got[k].dtype)[0]
            assert _bits(outside).tolist() == _bits(np.full(outside.shape, guard)).tolist(), "%s: guard changed" % k
            for i in np.flatnonzero(fin):
                a, b = offsets[i], max(offsets[i], offsets[i + 1])
                _eq(got[k][a:b], ref[k][a:b], "query %d %s" % (i, k))
        _eq(cnt[fin], ref["count"][fin], "count")
        assert (room[fin] < full[fin]).any(), "no room truncated"
        for with_count in (True, False):                        # fixed rooms of 3
            g, c = _raw(rt, sp, tris, None, 3, len(tris) * 3, with_count=with_count)
            r = ti.rooms(so, np.ascontiguousarray(tris[fin]), max_hits=3)
            for k in FIELDS:
                _eq(g[k].reshape((len(tris), 3) + g[k].shape[1:])[fin], r[k].reshape((fin.sum(), 3) + r[k].shape[1:]),
                    "fixed K=3 (count %s) %s" % (with_count, k))
            assert (c[fin] == r["count"]).all() if with_count else (c == -9).all()
        g1 = sp.list_intersecting(tris, max_hits=3, outputs=FIELDS + ("count",))
        g2 = sp.list_intersecting(np.ascontiguousarray(tris[fin]), max_hits=3, outputs=FIELDS + ("count",))
        for k in FIELDS + ("count",):
            _eq(g1[k][fin], g2[k], "finite queries beside non-finite " + k)
        c1 = sp.count_intersecting(tris, outputs=("count", "any"))
        _eq(c1["count"][fin], full[fin].astype(np.int32), "count_intersecting beside non-finite")
    finally:
        sp.close()
        so.close()


def test_instance_against_the_rest(rt, orc, scenes, blob5k):
    """Each instance's own world triangles with skip_instance = that instance: "what does it touch?" equals the shim, and the
    skipped instance never appears."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        o = orc.oracle()
        rng = np.random.default_rng(5)
        for k, (mesh, _mat, pose, scale) in enumerate(desc.instances):
            t = o.mesh_dump(desc.oracle_meshes[mesh])["tris"][:, :9].reshape(-1, 3, 3)
            t = t[rng.choice(len(t), min(len(t), 300), replace=False)]
            w = np.ascontiguousarray(qp._world(o, pose, scale, t.reshape(-1, 3)).reshape(-1, 3, 3), F32)
            skip = np.full(len(w), k, np.int32)
            ref = _check(sp, so, w, skip, where="instance %d vs the rest" % k, ks=(2,))
            assert not (ref["instance"] == k).any()
    finally:
        sp.close()
        so.close()


def test_call_shapes(rt, orc, scenes, blob5k):
    """n = 0, queries without pairs (total 0), a [10, 20, 3, 3] leading shape, output subsets, numpy against torch, torch on a side
    stream."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(8)
        tris = _flat(families(rng, orc.oracle(), desc, n=200))
        tris = np.ascontiguousarray(tris[rng.choice(len(tris), 200, replace=False)])
        ref = ti.list_intersecting(so, tris)
        g = sp.list_intersecting(tris[:0])
        assert g["offsets"].tolist() == [0] and all(g[k].shape[0] == 0 for k in ("instance", "triangle", "query_index", "count"))
        g = sp.list_intersecting(tris[:0], max_hits=2, outputs=("instance", "segment"))
        assert g["instance"].shape == (0, 2) and g["segment"].shape == (0, 2, 2, 3)
        c = sp.count_intersecting(tris[:0], outputs=("count", "any"))
        assert c["count"].shape == (0,) and c["any"].shape == (0,)
        far = np.full((70, 3, 3), 50.0, F32)
        far[:, 1, 0] = 51.0
        far[:, 2, 1] = 51.0
        g = sp.list_intersecting(far)
        assert g["offsets"].tolist() == [0] * 71 and g["instance"].shape == (0,) and (g["count"] == 0).all()
        g = sp.list_intersecting(tris.reshape(10, 20, 3, 3), max_hits=3, outputs=("instance", "segment", "count"))
        assert set(g) == {"instance", "segment", "count"} and g["instance"].shape == (10, 20, 3) and g["segment"].shape == (10, 20, 3, 2, 3)
        r3 = ti.list_intersecting(so, tris, max_hits=3)
        _eq(g["segment"], r3["segment"].reshape(10, 20, 3, 2, 3), "[10, 20, 3, 3] segment")
        _eq(g["count"], ref["count"].reshape(10, 20), "[10, 20, 3, 3] count")
        c = sp.count_intersecting(tris.reshape(10, 20, 3, 3), outputs=("count",))
        assert set(c) == {"count"} and c["count"].shape == (10, 20)
        g = sp.list_intersecting(tris, outputs=("normal", "triangle"))
        assert set(g) == {"normal", "triangle", "offsets", "query_index", "count"}
        _eq(g["normal"], ref["normal"], "normal only")
        tt = torch.from_numpy(tris).cuda()
        sk = torch.full((200,), -1, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        gt = sp.list_intersecting(tt, sk, outputs=FIELDS, stream=s)
        gk = sp.list_intersecting(tt, max_hits=2, outputs=FIELDS + ("count", "pops"), stream=s)
        gc = sp.count_intersecting(tt, sk, outputs=("count", "any", "pops"), stream=s)
        s.synchronize()
        assert gt["offsets"].dtype == torch.int64 and gt["query_index"].dtype == torch.int32 and gt["count"].dtype == torch.int32
        for k in FIELDS + ("offsets", "query_index", "count"):
            _eq(gt[k].cpu().numpy(), ref[k], "torch side stream " + k)
        r2 = ti.list_intersecting(so, tris, max_hits=2)
        for k in FIELDS + ("count",):
            _eq(gk[k].cpu().numpy(), r2[k], "torch side stream K=2 " + k)
        assert (gk["pops"].cpu().numpy() >= 0).all()
        _eq(gc["count"].cpu().numpy(), ref["count"], "torch side stream count_intersecting")
        assert np.array_equal(gc["any"].cpu().numpy(), ref["count"] > 0)
    finally:
        sp.close()
        so.close()


def test_pruning_is_real(rt, orc, scenes, blob70k):
    """On c2: triangles 1e-3 of the diagonal in size centred on surface points visit on average under 1 % of c2's interior nodes, and
    their lists equal the shim."""
    desc = sd.blob_scene(scenes, blob70k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        org, dirs = _cam_rays(scenes, 160, 90, scenes.scaled_K(160), scenes.C2_CAMERAS["mid"])
        hit = ray_oracle.cast_rays(so, org.reshape(-1, 3), dirs.reshape(-1, 3))
        ok = hit["instance"] >= 0
        lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
        diag = np.float32(np.linalg.norm(hi - lo))
        rng = np.random.default_rng(6)
        c = hit["location"][ok][:3000]
        tris = np.ascontiguousarray(c[:, None, :] + rng.normal(size=(len(c), 3, 3)).astype(F32) * (diag * F32(1e-3) / F32(2)), F32)
        got = sp.list_intersecting(tris, outputs=FIELDS + ("pops",))
        ref = ti.list_intersecting(so, tris[:300])
        for k in FIELDS:
            _eq(got[k][:ref["offsets"][-1]], ref[k], "c2 small triangles " + k)
        assert (got["count"] > 0).mean() > 0.5
        interior = int((orc.oracle().mesh_dump(desc.oracle_meshes[0])["child"][:, 0] > 0).sum())
        assert got["pops"].mean() < 0.01 * interior, (got["pops"].mean(), interior)
    finally:
        sp.close()
        so.close()
