"""Box queries on the GPU (Scene.count_in_boxes / Scene.list_in_boxes / Scene.occupancy_grid through rt_count_in_boxes / rt_box_offsets /
rt_list_in_boxes / rt_occupancy_grid): every field equals the brute-force shim (tests/box_oracle.c) bit for bit on the library's and
adversarial scenes, under every tree and scene change, in CSR and fixed rooms with and without count, nothing outside a room is ever
written, and the grid equals count_in_boxes on its cells.  Sizes are small here: the scan's edges, rooms at slots past 2^31, grids of
more than 65536 bricks and the 2^24 axis are test_gpu_query_scale.py's, threads test_gpu_query_threads.py's."""
import ctypes as C

import numpy as np
import pytest

import box_oracle as bo
import query_points as qp
import scene_defs as sd
from test_gpu_crossings import _bits, _eq
from test_gpu_point_query import SEEDS, _library_scene, _product

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("instance", "triangle")


def _scene_vertices(rng, o, desc, m):
    """up to m finite world vertices of the scene's triangles"""
    pts = []
    for mesh, _mat, pose, scale in desc.instances:
        t = o.mesh_dump(desc.oracle_meshes[mesh])["tris"][:, :9].reshape(-1, 3)
        t = t[np.isfinite(t).all(axis=1) & (np.abs(t) < 1e30).all(axis=1)]
        if len(t):
            pts.append(qp._world(o, pose, scale, t[rng.choice(len(t), min(len(t), m), replace=False)]))
    p = np.concatenate(pts) if pts else np.zeros((0, 3), F32)
    p = p[np.isfinite(p).all(axis=1)]
    return p[rng.choice(len(p), min(len(p), m), replace=False)] if len(p) else p


def families(rng, o, desc, n=100):
    """-> list of (name, world boxes [m, 2, 3] float32), all finite.  o: orc.oracle(); desc after desc.build_oracle."""
    lo, hi = qp.scene_box(o, desc, desc.oracle_meshes)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    span = np.maximum(hi - lo, 1e-3)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-3)
    fams = []
    g = bo.grid_boxes(lo - 0.05 * span, 1.1 * span / (5, 5, 4), (5, 5, 4)).reshape(-1, 2, 3)       # cells of a coarse grid
    fams.append(("grid", g))
    v = _scene_vertices(rng, o, desc, n).astype(np.float64)
    if len(v):
        e = diag * 10.0 ** rng.uniform(-3, -1, (len(v), 3))
        fams.append(("lo_at_vertex", np.stack([v, v + e], axis=1)))
        fams.append(("hi_at_vertex", np.stack([v - e, v], axis=1)))
    c = lo + span * rng.uniform(-0.1, 1.1, (n, 3))
    e = diag * 10.0 ** rng.uniform(-4, np.log10(0.5), (n, 3))
    fams.append(("random", np.stack([c - e / 2, c + e / 2], axis=1)))
    flat = np.stack([c - e / 2, c + e / 2], axis=1)[: n // 2].copy()
    ax = rng.integers(0, 3, len(flat))
    flat[np.arange(len(flat)), 1, ax] = flat[np.arange(len(flat)), 0, ax]
    fams.append(("flat", flat))
    if len(v):
        fams.append(("point_at_vertex", np.stack([v[: n // 4], v[: n // 4]], axis=1)))
    p = lo + span * rng.uniform(0, 1, (n // 4, 3))
    fams.append(("point", np.stack([p, p], axis=1)))
    fams.append(("whole", np.stack([lo - span, hi + span])[None]))
    inv = np.stack([c - e / 2, c + e / 2], axis=1)[: n // 4].copy()
    ax = rng.integers(0, 3, len(inv))
    inv[np.arange(len(inv)), 0, ax], inv[np.arange(len(inv)), 1, ax] = inv[np.arange(len(inv)), 1, ax] + 1e-3 * diag, inv[np.arange(len(inv)), 0, ax]
    fams.append(("inverted", inv))
    out = [(k, np.ascontiguousarray(b, F32)) for k, b in fams if len(b)]
    return [(k, b[np.isfinite(b).all(axis=(1, 2))]) for k, b in out]


def _flat(fams):
    return np.ascontiguousarray(np.concatenate([f[1] for f in fams]), F32)


def _check(sp, so, boxes, where="", ks=(1, 3, 64)):
    """CSR and fixed rooms K against the shim; count, any and pops; offsets; fixed rooms with and without count identical"""
    got = sp.list_in_boxes(boxes, outputs=FIELDS + ("pops",))
    ref = bo.list_in_boxes(so, boxes)
    for k in FIELDS + ("offsets", "query_index", "count"):
        _eq(got[k], ref[k], "%s CSR %s" % (where, k))
    assert int(got["offsets"][-1]) == int(ref["count"].astype(np.int64).sum()) and (got["pops"] >= 0).all()
    c = sp.count_in_boxes(boxes, outputs=("count", "any", "pops"))
    _eq(c["count"], ref["count"], where + " count_in_boxes")
    assert c["any"].dtype == np.bool_ and np.array_equal(c["any"], ref["count"] > 0), where
    a = sp.count_in_boxes(boxes, outputs=("any", "pops"))
    assert np.array_equal(a["any"], ref["count"] > 0), where + " any only"
    assert (a["pops"] <= c["pops"]).all(), where + " pops(any only) <= pops(count)"
    for K in ks:
        r = bo.list_in_boxes(so, boxes, max_hits=K)
        g = sp.list_in_boxes(boxes, max_hits=K, outputs=FIELDS + ("count",))
        g2 = sp.list_in_boxes(boxes, max_hits=K, outputs=FIELDS)
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
        boxes = _flat(families(rng, orc.oracle(), desc))
        boxes = np.ascontiguousarray(boxes[rng.choice(len(boxes), 65, replace=False)])
        c = sp.count_in_boxes(boxes, outputs=("count", "pops"))
        assert (c["count"] > 3).any() and c["pops"].max() > 0
        _eq(sp.list_in_boxes(boxes, outputs=FIELDS + ("pops",))["pops"], c["pops"], "pops(CSR list) == pops(count)")
        _eq(sp.list_in_boxes(boxes, max_hits=3, outputs=FIELDS + ("count", "pops"))["pops"], c["pops"], "pops(K=3 with count) == pops(count)")
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    desc, _cam = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(29)
        fams = families(rng, orc.oracle(), desc)
        assert {k for k, _b in fams} >= {"grid", "random", "flat", "point", "whole", "inverted"}
        boxes = _flat(fams)
        ref = _check(sp, so, boxes, where=name)
        assert (ref["count"] > 0).sum() > 10, name
        inv = np.concatenate([np.zeros(len(b), bool) + (k == "inverted") for k, b in fams])
        assert (ref["count"][inv] == 0).all()
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
        _check(sp, so, _flat(families(rng, orc.oracle(), desc, n=80)), where=info, ks=(1, 3))
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_partial_waves_on_the_deep_tree(rt, orc, scenes, blob5k, demo_objs, n):
    desc, _cam = _library_scene("deep", scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(n)
        boxes = _flat(families(rng, orc.oracle(), desc))
        boxes = np.ascontiguousarray(boxes[rng.choice(len(boxes), n, replace=False)])
        lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
        boxes[0] = np.stack([lo - 1, hi + 1])                   # (the whole scene is always among them)
        ref = _check(sp, so, boxes, where="deep n=%d" % n, ks=(3,))
        assert ref["count"][0] > 0
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
        boxes = _flat(families(rng, orc.oracle(), desc))
        res = [sp.list_in_boxes(boxes, outputs=FIELDS) for sp in (a, b, c)]
        res8 = [sp.list_in_boxes(boxes, max_hits=8, outputs=FIELDS) for sp in (a, b, c)]
        for j, label in ((1, "device tree"), (2, "refitted tree")):
            for k in FIELDS + ("offsets",):
                _eq(res[j][k], res[0][k], "%s %s" % (label, k))
            for k in FIELDS:
                _eq(res8[j][k], res8[0][k], "%s K=8 %s" % (label, k))
        _check(a, so, boxes, where="host tree", ks=(8,))
        new_tris = desc.meshes[1][1].copy()
        new_tris[:, [0, 3, 6]] += 0.05
        a.refit_mesh(1, new_tris)
        orc.oracle().mesh_refit(desc.oracle_meshes[1], new_tris)
        _check(a, so, boxes, where="refit_mesh", ks=(2,))
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        a.rebuild_mesh(1, new)
        so.close()
        so = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances).build_oracle(orc)
        _check(a, so, boxes, where="rebuild_mesh", ks=(2,))
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        a.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        bt = torch.from_numpy(boxes).cuda()
        with torch.cuda.stream(s):
            g = a.list_in_boxes(bt, outputs=FIELDS)
            g4 = a.list_in_boxes(bt, max_hits=4, outputs=FIELDS)
            gc = a.count_in_boxes(bt, outputs=("count", "any"))
        s.synchronize()
        ref, ref4 = bo.list_in_boxes(so, boxes), bo.list_in_boxes(so, boxes, max_hits=4)
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


def _raw(rt, sp, boxes, offsets, max_hits, slots, with_count=True, guard=0x5A):
    """rt_list_in_boxes straight through the C-ABI into buffers pre-filled with a guard byte -> (dict of the slot arrays, count)"""
    import torch
    n = len(boxes)
    out = {k: torch.full((slots * 4,), guard, dtype=torch.uint8, device="cuda").view(torch.int32) for k in FIELDS}
    cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    bt = torch.from_numpy(boxes).cuda()
    ot = None if offsets is None else torch.from_numpy(offsets).cuda()
    lst = rt.RtBoxList(*[out[k].data_ptr() for k in FIELDS], cnt.data_ptr() if with_count else None, None)
    torch.cuda.synchronize()
    rc = rt.libs()[0].rt_list_in_boxes(sp.device_handle, bt.data_ptr(), n, None if ot is None else ot.data_ptr(), max_hits, C.byref(lst),
                                       None, 1)
    assert rc == 0
    return {k: v.cpu().numpy() for k, v in out.items()}, cnt.cpu().numpy()


def test_rooms_never_written_outside(rt, orc, scenes, blob5k):
    """Rooms sized below each count truncate, gaps lie between them (some rooms of 0 and a negative one), and non-finite boxes sit
    between finite ones: every slot outside a room keeps its guard word, every finite box's room equals the shim's, and finite
    boxes' results do not depend on the non-finite ones.  Fixed rooms with and without count write the same."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        boxes = _flat(families(rng, orc.oracle(), desc, n=120))
        bad = rng.random(len(boxes)) < 0.2
        idx = np.flatnonzero(bad)
        boxes[idx[0::4], 0, 0] = np.nan
        boxes[idx[1::4], 1, 2] = np.inf                         # (hi = +inf: a valid, unbounded box -- results unspecified)
        boxes[idx[2::4], 0] = -np.inf
        boxes[idx[3::4]] = np.array([[-np.inf] * 3, [np.inf] * 3], F32)
        fin = ~bad
        zeroed = np.where(fin[:, None, None], boxes, F32(0))
        full = bo.count_in_boxes(so, zeroed).astype(np.int64)
        full[bad] = 0
        room = np.maximum(full - rng.integers(0, 3, len(boxes)), 0) + rng.integers(0, 2, len(boxes))
        room[rng.random(len(boxes)) < 0.1] = 0
        offsets = np.concatenate([[3], 3 + np.cumsum(room)]).astype(np.int64)
        offsets[-1] = offsets[-2] - 2                           # the last box's room is negative
        slots = int(offsets[-2]) + 5                            # slots 0-2 and the last 5 belong to no room
        got, cnt = _raw(rt, sp, boxes, offsets, 0, slots)
        ref = bo.rooms(so, zeroed, offsets=offsets, slots=slots)
        inroom = np.zeros(slots, bool)
        for i in range(len(boxes)):
            inroom[offsets[i]:max(offsets[i], offsets[i + 1])] = True
        guard = np.frombuffer(bytes([0x5A]) * 4, np.int32)[0]
        for k in FIELDS:
            assert (got[k][~inroom] == guard).all(), "%s: guard changed" % k
            for i in np.flatnonzero(fin):
                a, b = offsets[i], max(offsets[i], offsets[i + 1])
                _eq(got[k][a:b], ref[k][a:b], "box %d %s" % (i, k))
        _eq(cnt[fin], ref["count"][fin], "count")
        assert (room[fin] < full[fin]).any(), "no room truncated"
        for with_count in (True, False):                        # fixed rooms of 3
            g, c = _raw(rt, sp, boxes, None, 3, len(boxes) * 3, with_count=with_count)
            r = bo.rooms(so, np.ascontiguousarray(boxes[fin]), max_hits=3)
            for k in FIELDS:
                _eq(g[k].reshape(len(boxes), 3)[fin], r[k].reshape(fin.sum(), 3), "fixed K=3 (count %s) %s" % (with_count, k))
            assert (c[fin] == r["count"]).all() if with_count else (c == -9).all()
        g1 = sp.list_in_boxes(boxes, max_hits=3, outputs=FIELDS + ("count",))
        g2 = sp.list_in_boxes(np.ascontiguousarray(boxes[fin]), max_hits=3, outputs=FIELDS + ("count",))
        for k in FIELDS + ("count",):
            _eq(g1[k][fin], g2[k], "finite boxes beside non-finite " + k)
        c1 = sp.count_in_boxes(boxes, outputs=("count", "any"))
        _eq(c1["count"][fin], full[fin].astype(np.int32), "count_in_boxes beside non-finite")
    finally:
        sp.close()
        so.close()


def test_call_shapes_and_streams(rt, orc, scenes, blob5k):
    """n = 0, boxes without pairs (total 0), a [10, 20, 2, 3] leading shape, output subsets, numpy against torch, torch on a
    torch.cuda.Stream and on its raw handle."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(8)
        boxes = _flat(families(rng, orc.oracle(), desc, n=120))
        boxes = np.ascontiguousarray(boxes[rng.choice(len(boxes), 200, replace=False)])
        ref = bo.list_in_boxes(so, boxes)
        g = sp.list_in_boxes(boxes[:0])
        assert g["offsets"].tolist() == [0] and all(g[k].shape[0] == 0 for k in ("instance", "triangle", "query_index", "count"))
        g = sp.list_in_boxes(boxes[:0], max_hits=2, outputs=("instance",))
        assert g["instance"].shape == (0, 2)
        c = sp.count_in_boxes(boxes[:0], outputs=("count", "any"))
        assert c["count"].shape == (0,) and c["any"].shape == (0,)
        far = np.tile(np.array([[50, 50, 50], [51, 51, 51]], F32), (70, 1, 1))
        g = sp.list_in_boxes(far)
        assert g["offsets"].tolist() == [0] * 71 and g["instance"].shape == (0,) and (g["count"] == 0).all()
        g = sp.list_in_boxes(boxes.reshape(10, 20, 2, 3), max_hits=3, outputs=("triangle", "count"))
        assert set(g) == {"triangle", "count"} and g["triangle"].shape == (10, 20, 3)
        r3 = bo.list_in_boxes(so, boxes, max_hits=3)
        _eq(g["triangle"], r3["triangle"].reshape(10, 20, 3), "[10, 20, 2, 3] triangle")
        _eq(g["count"], ref["count"].reshape(10, 20), "[10, 20, 2, 3] count")
        c = sp.count_in_boxes(boxes.reshape(10, 20, 2, 3), outputs=("count",))
        assert set(c) == {"count"} and c["count"].shape == (10, 20)
        g = sp.list_in_boxes(boxes, outputs=("triangle",))
        assert set(g) == {"triangle", "offsets", "query_index", "count"}
        bt = torch.from_numpy(boxes).cuda()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        r2 = bo.list_in_boxes(so, boxes, max_hits=2)
        for stream in (s, s.cuda_stream):
            gt = sp.list_in_boxes(bt, outputs=FIELDS, stream=stream)
            gk = sp.list_in_boxes(bt, max_hits=2, outputs=FIELDS + ("count", "pops"), stream=stream)
            gc = sp.count_in_boxes(bt, outputs=("count", "any", "pops"), stream=stream)
            s.synchronize()
            assert gt["offsets"].dtype == torch.int64 and gt["query_index"].dtype == torch.int32 and gt["count"].dtype == torch.int32
            for k in FIELDS + ("offsets", "query_index", "count"):
                _eq(gt[k].cpu().numpy(), ref[k], "torch side stream " + k)
            for k in FIELDS + ("count",):
                _eq(gk[k].cpu().numpy(), r2[k], "torch side stream K=2 " + k)
            assert (gk["pops"].cpu().numpy() >= 0).all()
            _eq(gc["count"].cpu().numpy(), ref["count"], "torch side stream count_in_boxes")
            assert gc["any"].dtype == torch.bool and np.array_equal(gc["any"].cpu().numpy(), ref["count"] > 0)
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("name", ["multi", "deep"])
@pytest.mark.parametrize("dims", [(1, 1, 1), (4, 4, 4), (5, 3, 2), (9, 7, 5)])
def test_occupancy_grid_equals_count_in_boxes_on_its_cells(rt, orc, scenes, blob5k, demo_objs, name, dims):
    """The grid outputs are count_in_boxes on the cells made in numpy float32 by the header's formula (the spacing, 0.1 of the extent
    or so, is not representable) and the shim's; occupied alone (which stops at the first pair) and with count; torch and numpy; a
    zero dimension launches nothing; a negative spacing gives all zeros."""
    import torch
    desc, _cam = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
        span = np.maximum(hi - lo, F32(1e-3)).astype(F32)
        origin = (lo - F32(0.05) * span).astype(F32)
        spacing = (F32(1.1) * span / np.asarray(dims, F32)).astype(F32)
        if dims == (9, 7, 5):
            spacing = (F32(0.1) * span).astype(F32)
        cells = bo.grid_boxes(origin, spacing, dims)
        ref = bo.count_in_boxes(so, cells).reshape(dims[::-1])
        g = sp.occupancy_grid(origin, spacing, dims, outputs=("occupied", "count"), as_numpy=True)
        assert g["occupied"].dtype == np.bool_ and g["occupied"].shape == dims[::-1] and g["count"].dtype == np.int32
        _eq(g["count"], ref, "%s %s grid count" % (name, dims))
        assert np.array_equal(g["occupied"], ref > 0)
        c = sp.count_in_boxes(cells, outputs=("count", "any"))
        _eq(g["count"], c["count"], "grid against count_in_boxes")
        assert np.array_equal(g["occupied"], c["any"])
        o = sp.occupancy_grid(origin, spacing, dims, as_numpy=True)
        assert set(o) == {"occupied"} and np.array_equal(o["occupied"], ref > 0)
        s = torch.cuda.Stream()
        t = sp.occupancy_grid(tuple(origin), tuple(spacing), list(dims), outputs=("count", "occupied"), stream=s)
        s.synchronize()
        assert t["occupied"].dtype == torch.bool and t["count"].is_cuda
        _eq(t["count"].cpu().numpy(), ref, "torch grid count")
        assert ref.sum() > 0
        neg = sp.occupancy_grid(origin + spacing, -spacing, dims, outputs=("occupied", "count"), as_numpy=True)
        assert not neg["occupied"].any() and not neg["count"].any()
        for a in range(3):
            d0 = list(dims)
            d0[a] = 0
            z = sp.occupancy_grid(origin, spacing, d0, outputs=("occupied", "count"), as_numpy=True)
            assert z["occupied"].shape == tuple(d0[::-1]) and z["count"].size == 0
    finally:
        sp.close()
        so.close()


def test_grid_writes_only_its_cells(rt, orc, scenes, blob5k):
    """A (5, 3, 2) grid (partial bricks on every axis) written into guarded buffers: exactly the 30 cells change."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    sp = _product(rt, desc)
    try:
        occ = torch.full((30 + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        cnt = torch.full((30 + 64,), -9, dtype=torch.int32, device="cuda")
        o, s, d = (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(0.4, 0.7, 1.0), (C.c_int32 * 3)(5, 3, 2)
        torch.cuda.synchronize()
        assert rt.libs()[0].rt_occupancy_grid(sp.device_handle, o, s, d, occ.data_ptr() + 32, cnt.data_ptr() + 4 * 32, None, 1) == 0
        occ, cnt = occ.cpu().numpy(), cnt.cpu().numpy()
        assert (occ[:32] == 0x5A).all() and (occ[62:] == 0x5A).all() and (occ[32:62] <= 1).all()
        assert (cnt[:32] == -9).all() and (cnt[62:] == -9).all() and (cnt[32:62] >= 0).all()
        assert np.array_equal(occ[32:62] == 1, cnt[32:62] > 0) and cnt[32:62].sum() > 0
    finally:
        sp.close()
