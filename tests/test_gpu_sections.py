"""Plane sections on the GPU (Scene.count_sections / Scene.list_sections through rt_count_sections / rt_section_offsets /
rt_list_sections): every field equals the brute-force shim (tests/section_oracle.c) bit for bit on the library's and adversarial
scenes, under every tree and scene change, in CSR and fixed rooms with and without count, on streams and from several host threads,
and nothing outside a room is ever written."""
import ctypes as C
import threading

import numpy as np
import pytest

import query_points as qp
import scene_defs as sd
import section_oracle as sc
from test_gpu_crossings import _eq
from test_gpu_point_query import SEEDS, _library_scene, _product

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("instance", "triangle", "segment", "normal")
WIDTH = dict(instance=1, triangle=1, segment=6, normal=3)


def _scene_triangles(rng, o, desc, m):
    """m finite world triangles [m, 3, 3] of the scene (a scene with fewer gives some twice); none when it has none"""
    out = []
    for mesh, _mat, pose, scale in desc.instances:
        t = o.mesh_dump(desc.oracle_meshes[mesh])["tris"][:, :9]
        t = t[np.isfinite(t).all(axis=1) & (np.abs(t) < 1e30).all(axis=1)]
        if len(t):
            t = t[rng.choice(len(t), min(len(t), m), replace=False)]
            out.append(qp._world(o, pose, scale, t.reshape(-1, 3)).reshape(-1, 3, 3))
    w = np.concatenate(out) if out else np.zeros((0, 3, 3), F32)
    w = w[np.isfinite(w).all(axis=(1, 2))]
    return w[rng.choice(len(w), m, replace=len(w) < m)] if len(w) else w


def _unit(rng, m):
    u = rng.normal(size=(m, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def families(rng, o, desc, n=80):
    """-> list of (name, world planes [m, 2, 3] float32, point then normal), all finite.  o: orc.oracle(); desc after build_oracle."""
    lo, hi = qp.scene_box(o, desc, desc.oracle_meshes)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    span = np.maximum(hi - lo, 1e-3)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-3)
    mid = (lo + hi) / 2
    fams = []
    grid = []
    for a in range(3):                                          # axis planes at the faces of a coarse grid over the scene box
        for k in range(6):
            p, nn = mid.copy(), np.zeros(3)
            p[a] = lo[a] - 0.05 * span[a] + k * 1.1 * span[a] / 5
            nn[a] = 1.0 if k % 2 else -1.0
            grid.append([p, nn])
    fams.append(("grid", np.array(grid)))
    tw = _scene_triangles(rng, o, desc, n).astype(np.float64)
    if len(tw):
        v = tw[np.arange(len(tw)), rng.integers(0, 3, len(tw))]
        half = len(v) // 2
        ax = np.zeros((half, 3))
        ax[np.arange(half), rng.integers(0, 3, half)] = rng.choice([-1.0, 1.0], half)
        fams.append(("vertex_axis", np.stack([v[:half], ax], axis=1)))
        fams.append(("vertex_random", np.stack([v[half:], _unit(rng, len(v) - half) * 10.0 ** rng.uniform(-2, 2, (len(v) - half, 1))], axis=1)))
        t32 = np.unique(tw[: n // 2].astype(F32), axis=0)
        fn = np.cross(t32[:, 1] - t32[:, 0], t32[:, 2] - t32[:, 0]).astype(F32)     # the fp32 face normal
        fams.append(("contains_triangle", np.stack([t32[:, 0], fn], axis=1)))
    p = lo + span * rng.uniform(0, 1, (n, 3))
    fams.append(("random", np.stack([p, _unit(rng, n)], axis=1)))
    q = n // 4
    fams.append(("tiny_normal", np.stack([p[:q], _unit(rng, q) * 1e-10], axis=1)))
    fams.append(("huge_normal", np.stack([p[q:2 * q], _unit(rng, q) * 1e10], axis=1)))
    u = _unit(rng, q)
    fams.append(("outside", np.stack([mid + u * diag * rng.uniform(1.5, 4, (q, 1)), u * rng.choice([-1.0, 1.0], (q, 1))], axis=1)))
    zero = np.stack([p[: n // 8], np.zeros((n // 8, 3))], axis=1)
    zero[0, 1] = -0.0
    fams.append(("zero_normal", zero))
    out = [(k, np.ascontiguousarray(b, F32)) for k, b in fams if len(b)]
    return [(k, b[np.isfinite(b).all(axis=(1, 2))]) for k, b in out]


def _flat(fams):
    return np.ascontiguousarray(np.concatenate([f[1] for f in fams]), F32)


def _check(sp, so, planes, where="", ks=(1, 3, 64)):
    """CSR and fixed rooms K against the shim; count, any and pops; offsets; fixed rooms with and without count identical"""
    got = sp.list_sections(planes, outputs=FIELDS + ("pops",))
    ref = sc.list_sections(so, planes)
    for k in FIELDS + ("offsets", "query_index", "count"):
        _eq(got[k], ref[k], "%s CSR %s" % (where, k))
    assert int(got["offsets"][-1]) == int(ref["count"].astype(np.int64).sum()) and (got["pops"] >= 0).all()
    keys = sp.list_sections(planes, outputs=("instance", "triangle"))         # (no slot travels with the keys)
    for k in ("instance", "triangle", "offsets"):
        _eq(keys[k], ref[k], "%s CSR keys alone %s" % (where, k))
    nrm = sp.list_sections(planes, outputs=("normal",))                        # (the slot travels in the normal)
    _eq(nrm["normal"], ref["normal"], where + " CSR normal alone")
    c = sp.count_sections(planes, outputs=("count", "any", "pops"))
    _eq(c["count"], ref["count"], where + " count_sections")
    assert c["any"].dtype == np.bool_ and np.array_equal(c["any"], ref["count"] > 0), where
    a = sp.count_sections(planes, outputs=("any", "pops"))
    assert np.array_equal(a["any"], ref["count"] > 0), where + " any only"
    assert (a["pops"] <= c["pops"]).all(), where + " pops(any only) <= pops(count)"
    for K in ks:
        r = sc.list_sections(so, planes, max_hits=K)
        g = sp.list_sections(planes, max_hits=K, outputs=FIELDS + ("count",))
        g2 = sp.list_sections(planes, max_hits=K, outputs=FIELDS)
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
        planes = _flat(families(rng, orc.oracle(), desc))
        planes = np.ascontiguousarray(planes[rng.choice(len(planes), 65, replace=False)])
        c = sp.count_sections(planes, outputs=("count", "pops"))
        assert (c["count"] > 3).any() and c["pops"].max() > 0
        _eq(sp.list_sections(planes, outputs=FIELDS + ("pops",))["pops"], c["pops"], "pops(CSR list) == pops(count)")
        _eq(sp.list_sections(planes, max_hits=3, outputs=FIELDS + ("count", "pops"))["pops"], c["pops"], "pops(K=3 with count) == pops(count)")
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    desc, _cam = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(31)
        fams = families(rng, orc.oracle(), desc)
        assert {k for k, _b in fams} >= {"grid", "vertex_axis", "vertex_random", "contains_triangle", "random", "tiny_normal",
                                         "huge_normal", "outside", "zero_normal"}
        planes = _flat(fams)
        assert 240 <= len(planes) <= 350
        ref = _check(sp, so, planes, where=name)
        assert (ref["count"] > 0).sum() > 10, name
        label = np.concatenate([np.full(len(b), k, dtype=object) for k, b in fams])
        assert (ref["count"][(label == "outside") | (label == "zero_normal")] == 0).all()
        for k in ("tiny_normal", "huge_normal", "vertex_axis", "vertex_random"):
            assert (ref["count"][label == k] > 0).any(), (name, k)
        if name in ("multi", "demo"):                           # (c1 is a single triangle, deep a stack of 28 separate ones)
            assert ref["count"].max() > 64, name                # K = 64 truncates
            assert (ref["count"][label == "contains_triangle"] > 0).any(), name     # (the triangle's neighbours, not the triangle)
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
        _check(sp, so, _flat(families(rng, orc.oracle(), desc)), where=info, ks=(1, 3))
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
        planes = _flat(families(rng, orc.oracle(), desc))
        planes = np.ascontiguousarray(planes[rng.choice(len(planes), n, replace=False)])
        lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
        planes[0] = np.stack([(lo + hi) / 2, [0.3, -0.5, 0.8]])              # (a plane through the middle is always among them)
        ref = _check(sp, so, planes, where="deep n=%d" % n, ks=(3,))
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
        planes = _flat(families(rng, orc.oracle(), desc))
        res = [sp.list_sections(planes, outputs=FIELDS) for sp in (a, b, c)]
        res8 = [sp.list_sections(planes, max_hits=8, outputs=FIELDS) for sp in (a, b, c)]
        for j, label in ((1, "device tree"), (2, "refitted tree")):
            for k in FIELDS + ("offsets",):
                _eq(res[j][k], res[0][k], "%s %s" % (label, k))
            for k in FIELDS:
                _eq(res8[j][k], res8[0][k], "%s K=8 %s" % (label, k))
        _check(a, so, planes, where="host tree", ks=(8,))
        new_tris = desc.meshes[1][1].copy()
        new_tris[:, [0, 3, 6]] += 0.05
        a.refit_mesh(1, new_tris)
        orc.oracle().mesh_refit(desc.oracle_meshes[1], new_tris)
        _check(a, so, planes, where="refit_mesh", ks=(2,))
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        a.rebuild_mesh(1, new)
        so.close()
        so = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances).build_oracle(orc)
        _check(a, so, planes, where="rebuild_mesh", ks=(2,))
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        a.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        bt = torch.from_numpy(planes).cuda()
        with torch.cuda.stream(s):
            g = a.list_sections(bt, outputs=FIELDS)
            g4 = a.list_sections(bt, max_hits=4, outputs=FIELDS)
            gc = a.count_sections(bt, outputs=("count", "any"))
        s.synchronize()
        ref, ref4 = sc.list_sections(so, planes), sc.list_sections(so, planes, max_hits=4)
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


def _raw(rt, sp, planes, offsets, max_hits, slots, with_count=True, guard=0x5A):
    """rt_list_sections straight through the C-ABI into buffers pre-filled with a guard byte -> (dict of the slot arrays as int32
    words, count)"""
    import torch
    n = len(planes)
    out = {k: torch.full((slots * WIDTH[k] * 4,), guard, dtype=torch.uint8, device="cuda").view(torch.int32) for k in FIELDS}
    cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    bt = torch.from_numpy(planes).cuda()
    ot = None if offsets is None else torch.from_numpy(offsets).cuda()
    lst = rt.RtSectionList(*[out[k].data_ptr() for k in FIELDS], cnt.data_ptr() if with_count else None, None)
    torch.cuda.synchronize()
    rc = rt.libs()[0].rt_list_sections(sp.device_handle, bt.data_ptr(), n, None if ot is None else ot.data_ptr(), max_hits, C.byref(lst),
                                       None, 1)
    assert rc == 0
    return {k: v.cpu().numpy().reshape(slots, WIDTH[k]) for k, v in out.items()}, cnt.cpu().numpy()


def _words(a, k):
    """a shim field as int32 words [slots, width], as _raw gives the product's"""
    return np.ascontiguousarray(a).view(np.int32).reshape(-1, WIDTH[k])


def test_rooms_never_written_outside(rt, orc, scenes, blob5k):
    """Rooms sized below each count truncate, gaps lie between them (some rooms of 0 and a negative one), and non-finite planes sit
    between finite ones: every slot outside a room keeps its guard word in every field, every finite plane's room equals the shim's,
    and finite planes' results do not depend on the non-finite ones.  Fixed rooms with and without count write the same."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        planes = _flat(families(rng, orc.oracle(), desc, n=120))
        bad = rng.random(len(planes)) < 0.2
        idx = np.flatnonzero(bad)
        planes[idx[0::4], 0, 0] = np.nan
        planes[idx[1::4], 1, 2] = np.inf
        planes[idx[2::4], 1] = np.array([3e38, -3e38, 3e38], F32)           # (finite, the heights overflow)
        planes[idx[3::4]] = np.nan
        fin = ~bad
        zeroed = np.where(fin[:, None, None], planes, F32(0))
        full = sc.count_sections(so, zeroed).astype(np.int64)
        room = np.maximum(full - rng.integers(0, 3, len(planes)), 0) + rng.integers(0, 2, len(planes))
        room[bad] = rng.integers(0, 4, bad.sum())
        room[rng.random(len(planes)) < 0.1] = 0
        offsets = np.concatenate([[3], 3 + np.cumsum(room)]).astype(np.int64)
        offsets[-1] = offsets[-2] - 2                           # the last plane's room is negative
        slots = int(offsets[-2]) + 5                            # slots 0-2 and the last 5 belong to no room
        got, cnt = _raw(rt, sp, planes, offsets, 0, slots)
        ref = sc.rooms(so, zeroed, offsets=offsets, slots=slots)
        inroom = np.zeros(slots, bool)
        for i in range(len(planes)):
            inroom[offsets[i]:max(offsets[i], offsets[i + 1])] = True
        guard = np.frombuffer(bytes([0x5A]) * 4, np.int32)[0]
        for k in FIELDS:
            assert (got[k][~inroom] == guard).all(), "%s: guard changed" % k
            want = _words(ref[k], k)
            for i in np.flatnonzero(fin):
                a, b = offsets[i], max(offsets[i], offsets[i + 1])
                assert np.array_equal(got[k][a:b], want[a:b]), "plane %d %s" % (i, k)
        _eq(cnt[fin], ref["count"][fin], "count")
        assert (room[fin] < full[fin]).any(), "no room truncated"
        for with_count in (True, False):                        # fixed rooms of 3
            g, c = _raw(rt, sp, planes, None, 3, len(planes) * 3, with_count=with_count)
            r = sc.rooms(so, np.ascontiguousarray(planes[fin]), max_hits=3)
            for k in FIELDS:
                assert np.array_equal(g[k].reshape(len(planes), 3 * WIDTH[k])[fin], _words(r[k], k).reshape(fin.sum(), 3 * WIDTH[k])), \
                    "fixed K=3 (count %s) %s" % (with_count, k)
            assert (c[fin] == r["count"]).all() if with_count else (c == -9).all()
        g1 = sp.list_sections(planes, max_hits=3, outputs=FIELDS + ("count",))
        g2 = sp.list_sections(np.ascontiguousarray(planes[fin]), max_hits=3, outputs=FIELDS + ("count",))
        for k in FIELDS + ("count",):
            _eq(g1[k][fin], g2[k], "finite planes beside non-finite " + k)
        c1 = sp.count_sections(planes, outputs=("count", "any"))
        _eq(c1["count"][fin], full[fin].astype(np.int32), "count_sections beside non-finite")
    finally:
        sp.close()
        so.close()


def test_call_shapes_streams_and_threads(rt, orc, scenes, blob5k):
    """n = 0, planes without pairs (total 0), a [10, 20, 2, 3] leading shape, output subsets, numpy against torch, torch on a
    torch.cuda.Stream and on its raw handle; two streams with calls in flight at once on one scene; four host threads, each with a
    stream of its own, on one scene.  Every result equals the shim's."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(8)
        planes = _flat(families(rng, orc.oracle(), desc, n=120))
        planes = np.ascontiguousarray(planes[rng.choice(len(planes), 200, replace=False)])
        ref = sc.list_sections(so, planes)
        g = sp.list_sections(planes[:0])
        assert g["offsets"].tolist() == [0] and all(g[k].shape[0] == 0 for k in ("instance", "triangle", "segment", "query_index", "count"))
        assert g["segment"].shape == (0, 2, 3)
        g = sp.list_sections(planes[:0], max_hits=2, outputs=("segment",))
        assert g["segment"].shape == (0, 2, 2, 3)
        c = sp.count_sections(planes[:0], outputs=("count", "any"))
        assert c["count"].shape == (0,) and c["any"].shape == (0,)
        far = np.tile(np.array([[50, 50, 50], [1, 1, 1]], F32), (70, 1, 1))
        g = sp.list_sections(far)
        assert g["offsets"].tolist() == [0] * 71 and g["instance"].shape == (0,) and (g["count"] == 0).all()
        g = sp.list_sections(planes.reshape(10, 20, 2, 3), max_hits=3, outputs=("segment", "count"))
        assert set(g) == {"segment", "count"} and g["segment"].shape == (10, 20, 3, 2, 3)
        r3 = sc.list_sections(so, planes, max_hits=3)
        _eq(g["segment"], r3["segment"].reshape(10, 20, 3, 2, 3), "[10, 20, 2, 3] segment")
        _eq(g["count"], ref["count"].reshape(10, 20), "[10, 20, 2, 3] count")
        g = sp.list_sections(planes)
        assert set(g) == {"instance", "triangle", "segment", "offsets", "query_index", "count"}
        bt = torch.from_numpy(planes).cuda()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        r2 = sc.list_sections(so, planes, max_hits=2)

        def same(gt, gk, gc, where):
            for k in FIELDS + ("offsets", "query_index", "count"):
                _eq(gt[k].cpu().numpy(), ref[k], "%s CSR %s" % (where, k))
            for k in FIELDS + ("count",):
                _eq(gk[k].cpu().numpy(), r2[k], "%s K=2 %s" % (where, k))
            assert (gk["pops"].cpu().numpy() >= 0).all()
            _eq(gc["count"].cpu().numpy(), ref["count"], where + " count_sections")
            assert gc["any"].dtype == torch.bool and np.array_equal(gc["any"].cpu().numpy(), ref["count"] > 0)

        def ask(stream):
            return (sp.list_sections(bt, outputs=FIELDS, stream=stream),
                    sp.list_sections(bt, max_hits=2, outputs=FIELDS + ("count", "pops"), stream=stream),
                    sp.count_sections(bt, outputs=("count", "any", "pops"), stream=stream))
        for stream in (s, s.cuda_stream):
            got = ask(stream)
            s.synchronize()
            assert got[0]["offsets"].dtype == torch.int64 and got[0]["query_index"].dtype == torch.int32
            same(*got, "torch side stream")
        s2 = torch.cuda.Stream()                                # two streams, nothing waited for in between
        g1, g2 = ask(s), ask(s2)
        s.synchronize()
        s2.synchronize()
        same(*g1, "first of two streams")
        same(*g2, "second of two streams")
        results, errors = [None] * 4, []

        def worker(j):
            try:
                st = torch.cuda.Stream()
                results[j] = ask(st)
                st.synchronize()
            except Exception as e:                              # (reported by the main thread)
                errors.append((j, repr(e)))
        threads = [threading.Thread(target=worker, args=(j,)) for j in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(120)
        assert not any(t.is_alive() for t in threads) and not errors, errors
        for j in range(4):
            same(*results[j], "thread %d" % j)
    finally:
        sp.close()
        so.close()
