"""Region queries on the GPU (Scene.count_in_regions / Scene.list_in_regions through rt_count_in_regions / rt_region_offsets /
rt_list_in_regions): every field equals the brute-force shim (tests/region_oracle.c) bit for bit on the library's and adversarial
scenes, for every plane capacity of the kernels and plane counts below them, under every tree and scene change, in CSR and fixed
rooms with and without count, on streams and from several host threads, and nothing outside a room is ever written."""
import ctypes as C
import threading

import numpy as np
import pytest

import query_points as qp
import region_oracle as ro
import scene_defs as sd
from test_gpu_crossings import _eq
from test_gpu_point_query import SEEDS, _library_scene, _product
from test_gpu_sections import _scene_triangles, _unit

pytestmark = pytest.mark.gpu
F32 = np.float32
FIELDS = ("instance", "triangle", "inside", "normal")
WIDTH = dict(instance=4, triangle=4, inside=1, normal=12)              # bytes per slot
KS = (1, 2, 3, 6, 8)                                                    # every plane capacity (2, 4, 6, 8) and a K below its capacity


def _frames(rng, m):
    return np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(m)]) if m else np.zeros((0, 3, 3))


def _obbs(rt, c, q, half):
    return rt.regions_from_obbs(np.ascontiguousarray(c, F32), np.ascontiguousarray(q, F32), np.ascontiguousarray(half, F32))


def families(rt, rng, o, desc, n=40):
    """-> dict K -> list of (name, world regions [m, K, 2, 3] float32), all finite.  o: orc.oracle(); desc after build_oracle."""
    lo, hi = qp.scene_box(o, desc, desc.oracle_meshes)
    lo, hi = lo.astype(np.float64), hi.astype(np.float64)
    span = np.maximum(hi - lo, 1e-3)
    diag = max(float(np.linalg.norm(hi - lo)), 1e-3)
    mid = (lo + hi) / 2
    tw = _scene_triangles(rng, o, desc, n).astype(np.float64)
    v = tw[np.arange(len(tw)), rng.integers(0, 3, len(tw))] if len(tw) else np.zeros((0, 3))
    fams = {K: [] for K in KS}
    # K = 6: the cells of a coarse grid as box regions (neighbours share their faces), and the whole scene
    e = [np.linspace(lo[a] - 0.02 * span[a], hi[a] + 0.02 * span[a], 4) for a in range(3)]
    cells = np.array([[(e[0][i], e[1][j], e[2][k]), (e[0][i + 1], e[1][j + 1], e[2][k + 1])] for i in range(3) for j in range(3) for k in range(3)])
    fams[6].append(("grid", rt.regions_from_boxes(cells.astype(F32))))
    fams[6].append(("whole", rt.regions_from_boxes(np.array([[lo - 0.1 * span, hi + 0.1 * span]], F32))))
    # oriented boxes of 1e-4 to 0.5 of the diagonal: anywhere, and with a face through a scene vertex
    size = diag * 10.0 ** rng.uniform(-4, np.log10(0.5), n)
    half = 0.5 * size[:, None] * rng.uniform(0.4, 1.0, (n, 3))
    fams[6].append(("obb", _obbs(rt, lo + span * rng.uniform(0, 1, (n, 3)), _frames(rng, n), half)))
    if len(v):
        q = _frames(rng, len(v))
        size = diag * 10.0 ** rng.uniform(-2, np.log10(0.5), len(v))
        half = 0.5 * size[:, None] * rng.uniform(0.4, 1.0, (len(v), 3))
        c = v + q[:, 0] * half[:, :1] * rng.choice([-1.0, 1.0], (len(v), 1))       # the face across axis 0 passes through the vertex
        fams[6].append(("obb_vertex", _obbs(rt, c, q, half)))
    # frusta from points outside the scene that look at it
    m = n // 4
    u = _unit(rng, m)
    eye = mid + u * diag * rng.uniform(0.8, 2.0, (m, 1))
    q = _frames(rng, m)
    q[:, 2] = u                                                                    # the view direction is -u: towards the middle
    q[:, 0] = np.cross(q[:, 1], u)
    q[:, 0] /= np.linalg.norm(q[:, 0], axis=1, keepdims=True)
    q[:, 1] = np.cross(u, q[:, 0])
    tan = rng.uniform(0.02, 0.25, (m, 2))
    cam = np.stack([np.stack([sx * tan[:, 0], sy * tan[:, 1], -np.ones(m)], 1) for sx, sy in ((1, -1), (1, 1), (-1, 1), (-1, -1))], 1)
    corners = eye[:, None] + diag * np.einsum("nkc,ncd->nkd", cam, q)
    fams[6].append(("frustum", rt.regions_from_frusta(eye.astype(F32), corners.astype(F32), F32(0.1 * diag), (diag * rng.uniform(1, 3, m)).astype(F32))))
    # normals scaled by 1e-10 and 1e10; empty (two opposite faces swapped) and invalid (a zero normal in one plane) regions
    base = _obbs(rt, lo + span * rng.uniform(0.2, 0.8, (n, 3)), _frames(rng, n), 0.15 * diag * rng.uniform(0.5, 1, (n, 3)))
    q4 = n // 4
    tiny, huge, empty, zero = base[:q4].copy(), base[q4:2 * q4].copy(), base[2 * q4:3 * q4].copy(), base[3 * q4:].copy()
    tiny[:, :, 1] *= F32(1e-10)
    huge[:, :, 1] *= F32(1e10)
    empty[:, [0, 1], 0] = empty[:, [1, 0], 0]
    zero[np.arange(len(zero)), rng.integers(0, 6, len(zero)), 1] = 0
    zero[0, 3, 1] = -0.0
    fams[6] += [("tiny_normal", tiny), ("huge_normal", huge), ("empty", empty), ("zero_normal", zero)]
    if len(tw):
        # K = 2: thin slabs that contain a scene triangle's plane (P = A on both faces: zero thickness; and a few ulps thick)
        t32 = np.unique(tw.astype(F32), axis=0)
        fn = np.cross(t32[:, 1] - t32[:, 0], t32[:, 2] - t32[:, 0]).astype(F32)     # the fp32 face normal
        flat = np.stack([np.stack([t32[:, 0], fn], 1), np.stack([t32[:, 0], -fn], 1)], 1)
        thick = flat.copy()
        nn = fn.astype(np.float64) / np.maximum(np.linalg.norm(fn.astype(np.float64), axis=1, keepdims=True), 1e-30)
        thick[:, 0, 0] = (t32[:, 0] - nn * 1e-3 * diag).astype(F32)
        thick[:, 1, 0] = (t32[:, 0] + nn * 1e-3 * diag).astype(F32)
        fams[2] += [("slab_flat", flat), ("slab_thin", thick)]
        # K = 1: half-spaces through scene vertices; K = 3: corners at scene vertices (a few: each holds a large part of the scene)
        vq = v[:q4]
        fams[1].append(("half_vertex", np.stack([vq, _unit(rng, len(vq)) * 10.0 ** rng.uniform(-2, 2, (len(vq), 1))], 1)[:, None].astype(F32)))
        fams[3].append(("corner_vertex", np.stack([np.stack([vq, _unit(rng, len(vq))], 1) for _ in range(3)], 1).astype(F32)))
    p = lo + span * rng.uniform(0, 1, (q4, 3))
    fams[1].append(("half_random", np.stack([p, _unit(rng, q4)], 1)[:, None].astype(F32)))
    w = _unit(rng, q4)                                                             # (a slab 0.05 diagonals thick)
    fams[2].append(("slab_random", np.stack([np.stack([p, w], 1), np.stack([p + 0.05 * diag * w, -w], 1)], 1).astype(F32)))
    fams[3].append(("wedge", np.stack([np.stack([p, _unit(rng, q4)], 1) for _ in range(3)], 1).astype(F32)))
    # K = 8: an oriented box cut by two more planes through points of it
    box = _obbs(rt, lo + span * rng.uniform(0.1, 0.9, (n, 3)), _frames(rng, n), 0.15 * diag * rng.uniform(0.3, 1, (n, 3)))
    centre = box[:, :, 0].astype(np.float64).mean(1)
    cuts = np.stack([np.stack([centre + 0.05 * diag * rng.normal(size=(n, 3)), _unit(rng, n)], 1) for _ in range(2)], 1).astype(F32)
    fams[8].append(("box_cut", np.concatenate([box, cuts], 1)))
    out = {}
    for K, fs in fams.items():
        fs = [(k, np.ascontiguousarray(b, F32)) for k, b in fs if len(b)]
        out[K] = [(k, b[np.isfinite(b).all(axis=(1, 2, 3))]) for k, b in fs]
        assert all(b.shape[1:] == (K, 2, 3) for _k, b in out[K])
    return out


def _flat(fams):
    return np.ascontiguousarray(np.concatenate([f[1] for f in fams]), F32)


def _check(sp, so, regions, where="", ms=(1, 3, 64)):
    """CSR and fixed rooms against the shim; count, inside, any and pops; offsets; fixed rooms with and without count identical"""
    got = sp.list_in_regions(regions, outputs=FIELDS + ("pops",))
    ref = ro.list_in_regions(so, regions)
    for k in FIELDS + ("offsets", "query_index", "count"):
        _eq(got[k], ref[k], "%s CSR %s" % (where, k))
    assert int(got["offsets"][-1]) == int(ref["count"].astype(np.int64).sum()) and (got["pops"] >= 0).all()
    assert got["inside"].dtype == np.uint8
    keys = sp.list_in_regions(regions, outputs=("instance", "triangle"))      # (nothing travels with the keys)
    for k in ("instance", "triangle", "offsets"):
        _eq(keys[k], ref[k], "%s CSR keys alone %s" % (where, k))
    rc = ro.count_in_regions(so, regions)
    _eq(rc["count"], ref["count"], where + " shim count")
    c = sp.count_in_regions(regions, outputs=("count", "inside", "any", "pops"))
    _eq(c["count"], rc["count"], where + " count_in_regions")
    _eq(c["inside"], rc["inside"], where + " count_in_regions inside")
    assert c["any"].dtype == np.bool_ and np.array_equal(c["any"], rc["count"] > 0), where
    assert (c["inside"] <= c["count"]).all(), where
    a = sp.count_in_regions(regions, outputs=("any", "pops"))
    assert np.array_equal(a["any"], rc["count"] > 0), where + " any only"
    assert (a["pops"] <= c["pops"]).all(), where + " pops(any only) <= pops(count)"
    i = sp.count_in_regions(regions, outputs=("inside", "any"))               # (inside wanted: no early end)
    _eq(i["inside"], rc["inside"], where + " inside and any")
    assert np.array_equal(i["any"], rc["count"] > 0), where
    for M in ms:
        r = ro.list_in_regions(so, regions, max_hits=M)
        g = sp.list_in_regions(regions, max_hits=M, outputs=FIELDS + ("count",))
        g2 = sp.list_in_regions(regions, max_hits=M, outputs=FIELDS)
        assert set(g2) == set(FIELDS)
        for k in FIELDS:
            _eq(g[k], r[k], "%s M=%d %s" % (where, M, k))
            _eq(g2[k], r[k], "%s M=%d without count %s" % (where, M, k))
        _eq(g["count"], r["count"], "%s M=%d count" % (where, M))
        for k in ("inside", "normal"):                                        # (the flag, or the slot, travels alone)
            _eq(sp.list_in_regions(regions, max_hits=M, outputs=(k,))[k], r[k], "%s M=%d %s alone" % (where, M, k))
    ref["inside_count"] = rc["inside"]
    return ref


def test_full_traversals_visit_the_same_nodes(rt, orc, scenes, blob5k):
    """The count call, the CSR list call and the fixed-room list call with count all visit every pair of every instance, so their
    pops are equal element-wise (one full wave and a single-lane wave)."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(65)
        box8 = _flat(families(rt, rng, orc.oracle(), desc)[8])                 # (40 boxes cut by two more planes: some twice)
        box8 = np.ascontiguousarray(box8[rng.choice(len(box8), 65, replace=len(box8) < 65)])
        for K in (2, 4, 6, 8):                                  # every plane capacity of the kernels: a region's first K planes are a region
            regions = np.ascontiguousarray(box8[:, :K])
            c = sp.count_in_regions(regions, outputs=("count", "pops"))
            assert (c["count"] > 3).any() and c["pops"].max() > 0, K
            _eq(sp.list_in_regions(regions, outputs=FIELDS + ("pops",))["pops"], c["pops"], "K=%d pops(CSR list) == pops(count)" % K)
            _eq(sp.list_in_regions(regions, max_hits=3, outputs=FIELDS + ("count", "pops"))["pops"], c["pops"],
                "K=%d pops(M=3 with count) == pops(count)" % K)
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    desc, _cam = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(53)
        fams = families(rt, rng, orc.oracle(), desc)
        assert set(fams) == set(KS)
        assert {k for k, _b in fams[6]} >= {"grid", "whole", "obb", "obb_vertex", "frustum", "tiny_normal", "huge_normal", "empty", "zero_normal"}
        assert {k for k, _b in fams[2]} >= {"slab_flat", "slab_thin"}
        assert 240 <= sum(len(b) for fs in fams.values() for _k, b in fs) <= 400
        partial = whole = most = 0
        for K in KS:
            regions = _flat(fams[K])
            ref = _check(sp, so, regions, where="%s K=%d" % (name, K))
            label = np.concatenate([np.full(len(b), k, dtype=object) for k, b in fams[K]])
            partial += int(((ref["count"] - ref["inside_count"]) > 0).sum())
            whole += int((ref["inside_count"] > 0).sum())
            most = max(most, int(ref["count"].max()))
            if K == 6:
                assert (ref["count"][(label == "empty") | (label == "zero_normal")] == 0).all()
                assert (ref["inside_count"][label == "whole"] > 0).all() and (ref["count"][label == "whole"] == ref["inside_count"][label == "whole"]).all()
                for k in ("grid", "tiny_normal", "huge_normal", "obb_vertex") + (("frustum",) if name in ("multi", "demo") else ()):
                    assert (ref["count"][label == k] > 0).any(), (name, k)
            if K == 2:
                assert (ref["count"][label == "slab_flat"] > 0).any(), name     # (closed: the triangle in the slab's plane counts)
        if name in ("multi", "demo"):                           # (c1 is a single triangle, deep a stack of 28 separate ones)
            assert partial > 10 and whole > 10 and most > 64, (name, partial, whole, most)
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
        fams = families(rt, rng, orc.oracle(), desc, n=24)
        for K in KS:
            _check(sp, so, _flat(fams[K]), where="%s K=%d" % (info, K), ms=(1, 3))
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
        regions = _flat(families(rt, rng, orc.oracle(), desc, n=60)[6])
        regions = np.ascontiguousarray(regions[rng.choice(len(regions), n, replace=False)])
        lo, hi = qp.scene_box(orc.oracle(), desc, desc.oracle_meshes)
        regions[0] = rt.regions_from_boxes(np.stack([lo - 1, hi + 1]).astype(F32))   # (the whole scene is always among them)
        ref = _check(sp, so, regions, where="deep n=%d" % n, ms=(3,))
        assert ref["count"][0] > 0
    finally:
        sp.close()
        so.close()


def _mixed(rt, rng, o, desc, n=40):
    """the K = 6 families with the K = 8 ones beside them as two arrays (a test that needs one K uses the first)"""
    fams = families(rt, rng, o, desc, n=n)
    return _flat(fams[6]), _flat(fams[8])


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
        regions, regions8 = _mixed(rt, rng, orc.oracle(), desc)
        for rg in (regions, regions8):
            res = [sp.list_in_regions(rg, outputs=FIELDS) for sp in (a, b, c)]
            res8 = [sp.list_in_regions(rg, max_hits=8, outputs=FIELDS) for sp in (a, b, c)]
            for j, label in ((1, "device tree"), (2, "refitted tree")):
                for k in FIELDS + ("offsets",):
                    _eq(res[j][k], res[0][k], "%s %s" % (label, k))
                for k in FIELDS:
                    _eq(res8[j][k], res8[0][k], "%s M=8 %s" % (label, k))
        _check(a, so, regions, where="host tree", ms=(8,))
        new_tris = desc.meshes[1][1].copy()
        new_tris[:, [0, 3, 6]] += 0.05
        a.refit_mesh(1, new_tris)
        orc.oracle().mesh_refit(desc.oracle_meshes[1], new_tris)
        _check(a, so, regions, where="refit_mesh", ms=(2,))
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        a.rebuild_mesh(1, new)
        so.close()
        so = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances).build_oracle(orc)
        _check(a, so, regions8, where="rebuild_mesh", ms=(2,))
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        a.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        bt = torch.from_numpy(regions).cuda()
        with torch.cuda.stream(s):
            g = a.list_in_regions(bt, outputs=FIELDS)
            g4 = a.list_in_regions(bt, max_hits=4, outputs=FIELDS)
            gc = a.count_in_regions(bt, outputs=("count", "inside", "any"))
        s.synchronize()
        ref, ref4, rc = ro.list_in_regions(so, regions), ro.list_in_regions(so, regions, max_hits=4), ro.count_in_regions(so, regions)
        for k in FIELDS + ("offsets", "query_index", "count"):
            _eq(g[k].cpu().numpy(), ref[k], "update_mesh_instance(stream) " + k)
        for k in FIELDS:
            _eq(g4[k].cpu().numpy(), ref4[k], "update_mesh_instance(stream) M=4 " + k)
        _eq(gc["count"].cpu().numpy(), ref["count"], "update_mesh_instance(stream) count")
        _eq(gc["inside"].cpu().numpy(), rc["inside"], "update_mesh_instance(stream) inside")
        assert gc["any"].dtype == torch.bool and np.array_equal(gc["any"].cpu().numpy(), ref["count"] > 0)
    finally:
        for sp in (a, b, c):
            sp.close()
        so.close()


def _raw(rt, sp, regions, offsets, max_hits, slots, with_count=True, guard=0x5A):
    """rt_list_in_regions straight through the C-ABI into buffers pre-filled with a guard byte -> (dict of the slot arrays as bytes
    [slots, width], count)"""
    import torch
    n, K = regions.shape[:2]
    out = {k: torch.full((slots * WIDTH[k],), guard, dtype=torch.uint8, device="cuda") for k in FIELDS}
    cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    bt = torch.from_numpy(regions).cuda()
    ot = None if offsets is None else torch.from_numpy(offsets).cuda()
    lst = rt.RtRegionList(*[out[k].data_ptr() for k in FIELDS], cnt.data_ptr() if with_count else None, None)
    torch.cuda.synchronize()
    rc = rt.libs()[0].rt_list_in_regions(sp.device_handle, bt.data_ptr(), n, K, None if ot is None else ot.data_ptr(), max_hits,
                                         C.byref(lst), None, 1)
    assert rc == 0
    return {k: v.cpu().numpy().reshape(slots, WIDTH[k]) for k, v in out.items()}, cnt.cpu().numpy()


def _bytes(a, k):
    """a shim field as bytes [slots, width], as _raw gives the product's"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, WIDTH[k])


@pytest.mark.parametrize("K", [6, 8])
def test_rooms_never_written_outside(rt, orc, scenes, blob5k, K):
    """Rooms sized below each count truncate, gaps lie between them (some rooms of 0 and a negative one), and non-finite regions sit
    between finite ones: every slot outside a room keeps its guard byte in every field, every finite region's room equals the shim's,
    and finite regions' results do not depend on the non-finite ones.  Fixed rooms with and without count write the same."""
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        regions = _mixed(rt, rng, orc.oracle(), desc, n=60)[0 if K == 6 else 1]
        bad = rng.random(len(regions)) < 0.2
        idx = np.flatnonzero(bad)
        regions[idx[0::4], 0, 0, 0] = np.nan
        regions[idx[1::4], K - 1, 1, 2] = np.inf
        regions[idx[2::4], 2, 1] = np.array([3e38, -3e38, 3e38], F32)       # (finite, the heights overflow)
        regions[idx[3::4]] = np.nan
        fin = ~bad
        zeroed = np.where(fin[:, None, None, None], regions, F32(0))
        full = ro.count_in_regions(so, zeroed)["count"].astype(np.int64)
        room = np.maximum(full - rng.integers(0, 3, len(regions)), 0) + rng.integers(0, 2, len(regions))
        room[bad] = rng.integers(0, 4, bad.sum())
        room[rng.random(len(regions)) < 0.1] = 0
        offsets = np.concatenate([[3], 3 + np.cumsum(room)]).astype(np.int64)
        offsets[-1] = offsets[-2] - 2                           # the last region's room is negative
        slots = int(offsets[-2]) + 5                            # slots 0-2 and the last 5 belong to no room
        got, cnt = _raw(rt, sp, regions, offsets, 0, slots)
        ref = ro.rooms(so, zeroed, offsets=offsets, slots=slots)
        inroom = np.zeros(slots, bool)
        for i in range(len(regions)):
            inroom[offsets[i]:max(offsets[i], offsets[i + 1])] = True
        for k in FIELDS:
            assert (got[k][~inroom] == 0x5A).all(), "%s: guard changed" % k
            want = _bytes(ref[k], k)
            for i in np.flatnonzero(fin):
                a, b = offsets[i], max(offsets[i], offsets[i + 1])
                assert np.array_equal(got[k][a:b], want[a:b]), "region %d %s" % (i, k)
        _eq(cnt[fin], ref["count"][fin], "count")
        assert (room[fin] < full[fin]).any(), "no room truncated"
        for with_count in (True, False):                        # fixed rooms of 3
            g, c = _raw(rt, sp, regions, None, 3, len(regions) * 3, with_count=with_count)
            r = ro.rooms(so, np.ascontiguousarray(regions[fin]), max_hits=3)
            for k in FIELDS:
                assert np.array_equal(g[k].reshape(len(regions), 3 * WIDTH[k])[fin], _bytes(r[k], k).reshape(fin.sum(), 3 * WIDTH[k])), \
                    "fixed M=3 (count %s) %s" % (with_count, k)
            assert (c[fin] == r["count"]).all() if with_count else (c == -9).all()
        g1 = sp.list_in_regions(regions, max_hits=3, outputs=FIELDS + ("count",))
        g2 = sp.list_in_regions(np.ascontiguousarray(regions[fin]), max_hits=3, outputs=FIELDS + ("count",))
        for k in FIELDS + ("count",):
            _eq(g1[k][fin], g2[k], "finite regions beside non-finite " + k)
        c1 = sp.count_in_regions(regions, outputs=("count", "any"))
        _eq(c1["count"][fin], full[fin].astype(np.int32), "count_in_regions beside non-finite")
    finally:
        sp.close()
        so.close()


def test_call_shapes_streams_and_threads(rt, orc, scenes, blob5k):
    """n = 0, regions without pairs (total 0), a [10, 20, 6, 2, 3] leading shape, output subsets, numpy against torch, torch on a
    torch.cuda.Stream and on its raw handle; two streams with calls in flight at once on one scene; four host threads, each with a
    stream of its own, on one scene.  Every result equals the shim's."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(8)
        regions = _mixed(rt, rng, orc.oracle(), desc, n=70)[0]
        regions = np.ascontiguousarray(regions[rng.choice(len(regions), 200, replace=False)])
        ref, rc = ro.list_in_regions(so, regions), ro.count_in_regions(so, regions)
        g = sp.list_in_regions(regions[:0])
        assert g["offsets"].tolist() == [0] and all(g[k].shape[0] == 0 for k in ("instance", "triangle", "inside", "query_index", "count"))
        g = sp.list_in_regions(regions[:0], max_hits=2, outputs=("normal",))
        assert g["normal"].shape == (0, 2, 3)
        c = sp.count_in_regions(regions[:0], outputs=("count", "inside", "any"))
        assert c["count"].shape == (0,) and c["any"].shape == (0,) and c["inside"].shape == (0,)
        far = np.ascontiguousarray(np.tile(rt.regions_from_boxes(np.array([(50, 50, 50), (51, 51, 51)], F32)), (70, 1, 1, 1)))
        g = sp.list_in_regions(far)
        assert g["offsets"].tolist() == [0] * 71 and g["instance"].shape == (0,) and (g["count"] == 0).all()
        g = sp.list_in_regions(regions.reshape(10, 20, 6, 2, 3), max_hits=3, outputs=("inside", "normal", "count"))
        assert set(g) == {"inside", "normal", "count"} and g["normal"].shape == (10, 20, 3, 3) and g["inside"].shape == (10, 20, 3)
        r3 = ro.list_in_regions(so, regions, max_hits=3)
        _eq(g["normal"], r3["normal"].reshape(10, 20, 3, 3), "[10, 20, 6, 2, 3] normal")
        _eq(g["inside"], r3["inside"].reshape(10, 20, 3), "[10, 20, 6, 2, 3] inside")
        _eq(g["count"], ref["count"].reshape(10, 20), "[10, 20, 6, 2, 3] count")
        g = sp.list_in_regions(regions)
        assert set(g) == {"instance", "triangle", "inside", "offsets", "query_index", "count"}
        bt = torch.from_numpy(regions).cuda()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        r2 = ro.list_in_regions(so, regions, max_hits=2)

        def same(gt, gk, gc, where):
            for k in FIELDS + ("offsets", "query_index", "count"):
                _eq(gt[k].cpu().numpy(), ref[k], "%s CSR %s" % (where, k))
            for k in FIELDS + ("count",):
                _eq(gk[k].cpu().numpy(), r2[k], "%s M=2 %s" % (where, k))
            assert (gk["pops"].cpu().numpy() >= 0).all()
            _eq(gc["count"].cpu().numpy(), ref["count"], where + " count_in_regions")
            _eq(gc["inside"].cpu().numpy(), rc["inside"], where + " count_in_regions inside")
            assert gc["any"].dtype == torch.bool and np.array_equal(gc["any"].cpu().numpy(), ref["count"] > 0)

        def ask(stream):
            return (sp.list_in_regions(bt, outputs=FIELDS, stream=stream),
                    sp.list_in_regions(bt, max_hits=2, outputs=FIELDS + ("count", "pops"), stream=stream),
                    sp.count_in_regions(bt, outputs=("count", "inside", "any", "pops"), stream=stream))
        for stream in (s, s.cuda_stream):
            got = ask(stream)
            s.synchronize()
            assert got[0]["offsets"].dtype == torch.int64 and got[0]["query_index"].dtype == torch.int32
            assert got[0]["inside"].dtype == torch.uint8
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
            t.join(60)                                          # (a deadline, no retry)
        assert not any(t.is_alive() for t in threads) and not errors, errors
        for j in range(4):
            same(*results[j], "thread %d" % j)
    finally:
        sp.close()
        so.close()
