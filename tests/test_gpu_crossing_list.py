"""Crossing lists on the GPU (Scene.list_crossings through rt_crossing_offsets / rt_list_crossings): every field equals the
brute-force shim (tests/crossing_list_oracle.c) bit for bit, NaN patterns unified, on the library's and adversarial scenes, under
every tree and scene change, in CSR and fixed rooms, and nothing outside a room is ever written."""
import ctypes as C

import numpy as np
import pytest

import crossing_list_oracle as xl
import crossing_oracle as xo
import query_points as qp
import query_rays as qr
import ray_oracle
import scene_defs as sd
from test_gpu_crossings import SEEDS, _bits, _cam, _eq, _library_scene, _product, _segments

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("t", "instance", "triangle", "sign", "barycentric", "uv", "point")


def _check(sp, so, o, d, tmax=None, where="", ks=(1, 3, 64)):
    """CSR and fixed rooms against the shim; count against count_crossings; each fixed row the prefix of the CSR segment."""
    got = sp.list_crossings(o, d, tmax)
    ref = xl.list_crossings(so, o, d, tmax)
    for k in FIELDS + ("offsets", "ray", "count"):
        _eq(got[k], ref[k], "%s CSR %s" % (where, k))
    cnt = sp.count_crossings(o, d, tmax, outputs=("count",))["count"]
    _eq(got["count"], cnt, where + " count vs count_crossings")
    assert int(got["offsets"][-1]) == int(cnt.astype(np.int64).sum())
    for K in ks:
        g = sp.list_crossings(o, d, tmax, max_hits=K)
        r = xl.list_crossings(so, o, d, tmax, max_hits=K)
        for k in FIELDS + ("count",):
            _eq(g[k], r[k], "%s K=%d %s" % (where, K, k))
    return got


@pytest.mark.parametrize("name", ["c1", "blob", "multi", "atrium", "deep", "demo"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, atrium, demo_objs, name):
    desc, pose = _library_scene(name, scenes, blob5k, atrium, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(11)
        co, cd = _cam(scenes, 48, 27, pose)
        _check(sp, so, co, cd, where=name + " camera")
        o, d = qr.flatten(qr.families(rng, so, (co, cd), n=120 if name == "atrium" else 300))
        _check(sp, so, o, d, where=name + " families")
        _check(sp, so, o, d, qr.special_tmax(rng, len(o)), where=name + " families, special tmax", ks=(3,))
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, (co, cd), n=80 if name == "atrium" else 200))
        _check(sp, so, *_segments(rng, pts, 1000), where=name + " segments", ks=(1,))
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
        cam = ray_oracle.camera_rays(W, H, K, scenes.D_REF, pose)
        o, d = qr.flatten(qr.families(rng, so, cam, n=250))
        _check(sp, so, o, d, where=info, ks=(1, 3))
        _check(sp, so, o, d, qr.special_tmax(rng, len(o)), where=info + " special tmax", ks=(2,))
        pts = qp.flatten(qp.families(rng, orc.oracle(), desc, so, cam, n=150))
        _check(sp, so, *_segments(rng, pts, 800), where=info + " segments", ks=(1,))
    finally:
        sp.close()
        so.close()


def test_tmax_at_counted_t(rt, orc, scenes, blob5k):
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        co, cd = _cam(scenes, 32, 18, sd.MULTI_CAMERA["pose"])
        rng = np.random.default_rng(2)
        o, d, tm = [], [], []
        for j in rng.choice(len(co), 200, replace=False):
            for t in xo.crossing_ts(so, co[j], cd[j]):
                for k in (-2, -1, 0, 1, 2):
                    o.append(co[j]); d.append(cd[j]); tm.append(qp.ulp_steps(t, k))
        o, d, tm = (np.ascontiguousarray(np.asarray(a), F32) for a in (o, d, tm))
        assert len(o) > 300
        _check(sp, so, o, d, tm, where="tmax at counted t", ks=(2,))
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
        co, cd = _cam(scenes, 48, 27, sd.MULTI_CAMERA["pose"])
        o, d = qr.flatten(qr.families(rng, so, (co, cd), n=300))
        res = [sp.list_crossings(o, d) for sp in (a, b, c)]
        for other, label in ((res[1], "device tree"), (res[2], "refitted tree")):
            for k in FIELDS + ("offsets",):
                _eq(other[k], res[0][k], "%s %s" % (label, k))
        _check(a, so, o, d, where="host tree", ks=(2,))
        tris = desc.meshes[1][1].copy()
        tris[:, [0, 3, 6]] += 0.05
        a.refit_mesh(1, tris)
        orc.oracle().mesh_refit(desc.oracle_meshes[1], tris)
        _check(a, so, o, d, where="refit_mesh", ks=(2,))
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        a.rebuild_mesh(1, new)
        so.close()
        so = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances).build_oracle(orc)
        _check(a, so, o, d, where="rebuild_mesh", ks=(2,))
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        a.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        with torch.cuda.stream(s):
            g = a.list_crossings(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
            g4 = a.list_crossings(torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda(), max_hits=4)
        s.synchronize()
        ref, ref4 = xl.list_crossings(so, o, d), xl.list_crossings(so, o, d, max_hits=4)
        for k in FIELDS + ("offsets", "ray", "count"):
            _eq(g[k].cpu().numpy(), ref[k], "update_mesh_instance(stream) " + k)
        for k in FIELDS + ("count",):
            _eq(g4[k].cpu().numpy(), ref4[k], "update_mesh_instance(stream) K=4 " + k)
    finally:
        for sp in (a, b, c):
            sp.close()
        so.close()


def _raw(rt, sp, o, d, tmax, offsets, max_hits, slots, fields=FIELDS, guard=0x5A):
    """rt_list_crossings straight through the C-ABI into buffers pre-filled with a guard byte -> (dict of the slot arrays, count)"""
    import torch
    n = len(o)
    shapes = dict(t=(), instance=(), triangle=(), sign=(), barycentric=(2,), uv=(2,), point=(3,))
    dt = dict(t=torch.float32, instance=torch.int32, triangle=torch.int32, sign=torch.int8, barycentric=torch.float32,
              uv=torch.float32, point=torch.float32)
    out = {}
    for k in fields:
        b = torch.full((slots * int(np.prod(shapes[k], dtype=np.int64)) * torch.empty((), dtype=dt[k]).element_size(),), guard,
                       dtype=torch.uint8, device="cuda")
        out[k] = b.view(dt[k]).reshape((slots,) + shapes[k])
    cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tt = None if tmax is None else torch.from_numpy(tmax).cuda()
    ot = None if offsets is None else torch.from_numpy(offsets).cuda()
    lst = rt.RtCrossingList(*[out[k].data_ptr() if k in out else None for k in FIELDS], cnt.data_ptr())
    h = rt.libs()[0]
    torch.cuda.synchronize()
    rc = h.rt_list_crossings(sp.device_handle, to.data_ptr(), td.data_ptr(), None if tt is None else tt.data_ptr(), n,
                             None if ot is None else ot.data_ptr(), max_hits, C.byref(lst), None, 1)
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}, cnt.cpu().numpy()


def _guard_of(k):
    dt = {"t": F32, "instance": np.int32, "triangle": np.int32, "sign": np.int8, "barycentric": F32, "uv": F32, "point": F32}[k]
    return np.frombuffer(bytes([0x5A]) * np.dtype(dt).itemsize, dt)[0]


def test_rooms_never_written_outside(rt, orc, scenes, blob5k):
    """Offsets taken with a smaller tmax than the fill call truncate each list, rooms are placed with gaps between them (some of
    0 and negative size), and non-finite rays sit between finite ones: every slot outside a room keeps its guard word, every room
    equals the shim's, and the finite rays' lists do not depend on the non-finite ones.  The selection path (no t / instance /
    triangle given) fills the same rooms."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        co, cd = _cam(scenes, 32, 18, sd.MULTI_CAMERA["pose"])
        pick = rng.choice(len(co), 400, replace=False)
        o, d = co[pick].copy(), cd[pick].copy()
        bad = rng.random(len(o)) < 0.2
        o[np.flatnonzero(bad)[::2], 0] = np.nan
        d[np.flatnonzero(bad)[1::2], 1] = np.inf
        small = xo.count_crossings(so, o, d, np.full(len(o), 1.5, F32))["count"].astype(np.int64)
        small[rng.random(len(o)) < 0.1] = 0                      # (rooms of 0)
        room = small + rng.integers(0, 3, len(o))               # below, at or above the count taken with tmax 1.5
        offsets = np.concatenate([[3], 3 + np.cumsum(room)]).astype(np.int64)
        offsets[-1] = offsets[-2] - 2                           # the last ray's room is negative
        slots = int(offsets[-2]) + 5                            # slots 0-2 and the last 5 belong to no room
        fin = ~bad
        for fields in (FIELDS, ("sign", "point", "uv")):
            got, cnt = _raw(rt, sp, o, d, None, offsets, 0, slots, fields)
            ref = xl.rooms(so, o, d, offsets=offsets, slots=slots)
            inroom = np.zeros(slots, bool)
            for i in range(len(o)):
                inroom[offsets[i]:max(offsets[i], offsets[i + 1])] = True
            for k in fields:
                g = got[k]
                guard = _guard_of(k)
                outside = g[~inroom].reshape(-1)
                assert _bits(outside).tolist() == _bits(np.full(outside.shape, guard)).tolist(), "%s: guard changed" % k
                for i in np.flatnonzero(fin):
                    a, b = offsets[i], max(offsets[i], offsets[i + 1])
                    _eq(g[a:b], ref[k][a:b], "ray %d %s (%s)" % (i, k, "insert" if "t" in fields else "select"))
            _eq(cnt[fin], ref["count"][fin], "count")
        # the fixed form on the same rays: finite rays equal to an all-finite call's rows
        g1 = sp.list_crossings(o, d, max_hits=3)
        g2 = sp.list_crossings(np.ascontiguousarray(o[fin]), np.ascontiguousarray(d[fin]), max_hits=3)
        for k in FIELDS + ("count",):
            _eq(g1[k][fin], g2[k], "finite rays beside non-finite " + k)
    finally:
        sp.close()
        so.close()


def test_thousand_crossings_sorted(rt, orc):
    """A stack of 1200 parallel quads (2400 triangles, in shuffled order): rays through it cross 1200 of them, in t order, in CSR and
    in fixed rooms of 1, 64 and 2000; the selection path agrees."""
    o_ = orc.oracle()
    rng = np.random.default_rng(3)
    zs = rng.permutation(1200).astype(F32) * F32(0.01)
    tris = []
    for z in zs:
        for f in ((0, 1, 2), (0, 2, 3)):
            v = np.array([(0, 0, z), (1, 0, z), (1, 1, z), (0, 1, z)], F32)[list(f)]
            tris.append(np.asarray(o_.tri_from_vertices(v.ravel()), F32))
    desc = sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", np.stack(tris))], [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        o = np.concatenate([rng.uniform(0.2, 0.8, (70, 2)), np.full((70, 1), -1.0)], axis=1).astype(F32)
        d = np.concatenate([rng.uniform(-0.01, 0.01, (70, 2)), np.ones((70, 1))], axis=1).astype(F32)
        got = _check(sp, so, o, d, where="1200 quads", ks=(1, 64, 2000))
        assert (got["count"] >= 1200).all() and (np.diff(got["t"])[np.diff(got["ray"]) == 0] >= 0).all()
        sel, cnt = _raw(rt, sp, o[:8], d[:8], None, None, 16, 8 * 16, ("sign", "barycentric"))
        ref = xl.list_crossings(so, o[:8], d[:8], max_hits=16)
        _eq(sel["sign"].reshape(8, 16), ref["sign"], "selection sign")
        _eq(sel["barycentric"].reshape(8, 16, 2), ref["barycentric"], "selection barycentric")
    finally:
        sp.close()
        so.close()


def test_call_shapes(rt, orc, scenes, blob5k):
    """n = 0, all rays missing (total 0), a [10, 100, 3] leading shape, output subsets, numpy against torch, torch on a side stream."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(8)
        o = rng.uniform(-1.5, 1.5, (1000, 3)).astype(F32)
        d = rng.normal(size=(1000, 3)).astype(F32)
        ref = xl.list_crossings(so, o, d)
        g = sp.list_crossings(o[:0], d[:0])
        assert g["offsets"].tolist() == [0] and all(g[k].shape[0] == 0 for k in FIELDS + ("ray", "count"))
        g = sp.list_crossings(o[:0], d[:0], max_hits=2)
        assert g["t"].shape == (0, 2) and g["point"].shape == (0, 2, 3)
        miss = np.full((70, 3), 50.0, F32)
        g = sp.list_crossings(miss, d[:70])
        assert g["offsets"].tolist() == [0] * 71 and g["t"].shape == (0,) and (g["count"] == 0).all()
        g = sp.list_crossings(o.reshape(10, 100, 3), d.reshape(10, 100, 3), max_hits=3, outputs=("t", "point"))
        assert set(g) == {"t", "point", "count"} and g["t"].shape == (10, 100, 3) and g["point"].shape == (10, 100, 3, 3)
        r3 = xl.list_crossings(so, o, d, max_hits=3)
        _eq(g["t"], r3["t"].reshape(10, 100, 3), "[10, 100, 3] t")
        _eq(g["count"], ref["count"].reshape(10, 100), "[10, 100, 3] count")
        g = sp.list_crossings(o, d, outputs=("uv",))
        assert set(g) == {"uv", "offsets", "ray", "count"}
        _eq(g["uv"], ref["uv"], "uv only")
        to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        gt = sp.list_crossings(to, td, torch.full((1000,), float("inf"), device="cuda"), stream=s)
        gk = sp.list_crossings(to, td, max_hits=2, stream=s)
        s.synchronize()
        assert gt["offsets"].dtype == torch.int64 and gt["ray"].dtype == torch.int32 and gt["sign"].dtype == torch.int8
        for k in FIELDS + ("offsets", "ray", "count"):
            _eq(gt[k].cpu().numpy(), ref[k], "torch side stream " + k)
        r2 = xl.list_crossings(so, o, d, max_hits=2)
        for k in FIELDS + ("count",):
            _eq(gk[k].cpu().numpy(), r2[k], "torch side stream K=2 " + k)
        g = sp.list_crossings(to, td, max_hits=1)
        torch.cuda.synchronize()
        _eq(g["t"].cpu().numpy(), ref_first(ref, 1000), "torch current stream nearest")
    finally:
        sp.close()
        so.close()


def ref_first(ref, n):
    """the nearest crossing of each ray from a CSR result (inf where none) [n, 1]"""
    t = np.full((n, 1), np.inf, F32)
    has = ref["count"] > 0
    t[has, 0] = ref["t"][ref["offsets"][:-1][has]]
    return t
