"""Triangle distance queries on the GPU (rt_closest_to_triangles through Scene.closest_to_triangles): every output but `pops` is compared
bit for bit with the brute-force shim over the test oracle's scene (tests/triangle_distance_oracle.c), on the library's scenes, the
adversarial scenes of scene_defs.adversarial_scene, after scene changes and under every call shape.  `pops` is only bounded.  The
coverage the comparison relies on (winners of the three kinds, intersections, misses) is asserted on the shim's answers."""
import ctypes as C
import threading

import numpy as np
import pytest

import query_points as qp
import query_triangles as qt
import scene_defs as sd
import triangle_distance_oracle as tdo
from test_gpu_point_query import SEEDS, _bits, _cam_rays, _library_scene, _product

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
EXACT = tdo.OUTPUTS
ALL = EXACT + ("pops",)
SHARED = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")      # with Scene.closest_points


def _same(got, ref, where="", keys=EXACT):
    """bit for bit; NaN outputs compare equal whatever their bits (the point tests' rule)"""
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and g.dtype == r.dtype, (where, k, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.flatnonzero((_bits(g) != _bits(r)).reshape(g.shape[0] if g.ndim else 1, -1).any(axis=-1))
        assert bad.size == 0, "%s %s: %d triangles differ, first %s: got %s want %s" % (where, k, bad.size, bad[:3], g[bad[:3]], r[bad[:3]])


def _definitions(got, where=""):
    """within == (a distance candidate || intersections > 0); clearance by its definition"""
    cand = got["instance"] >= 0
    assert np.array_equal(got["within"], (cand | (got["intersections"] > 0)).astype(np.int32)), where
    assert np.array_equal(_bits(got["clearance"]), _bits(np.where(got["intersections"] > 0, F32(0), got["distance"]).astype(F32))), where
    assert (got["distance"][~cand] == FLT_MAX).all() and (got["triangle"][~cand] == -1).all(), where
    w = got["query_barycentric"]
    assert ((w >= 0) & (w <= 1)).all(), where


def _check(sp, so, tris, md=None, skip=None, where=""):
    got = sp.closest_to_triangles(tris, md, skip, outputs=ALL)
    ref = tdo.closest_to_triangles(so, tris, md, skip)
    _same(got, ref, where)
    _definitions(got, where)
    assert (got["pops"] >= 0).all(), where
    fast = sp.closest_to_triangles(tris, md, skip, outputs=("within", "pops"))      # the traversal that ends at the first candidate
    assert np.array_equal(fast["within"], ref["within"]), where
    assert (fast["pops"] <= got["pops"]).all(), where
    return got, ref


def _bounds(rng, ref, diag):
    """max_distance per triangle: +inf, 0, the exact distance and its float neighbours, NaN, negative, fractions of the distance, and
    a small bound (misses, and intersected triangles out of the minimum's reach)"""
    md = qp.special_bounds(rng, ref["distance"])
    small = rng.random(len(md)) < 0.25
    md[small] = F32(diag) * F32(1e-4)
    return md


def _edge_parameters(ref):
    """(s, u) of the winners from (c), read back from the weights: candidate 6 + 3 m + k has (q1, q2) = (s, 0), (0, s), (1 - s, s) for
    m = 0, 1, 2 and (b1, b2) likewise in u for k"""
    w, q, b = ref["which"], ref["query_barycentric"], ref["barycentric"]
    m, k = (w - 6) // 3, (w - 6) % 3
    return np.where(m == 0, q[:, 0], q[:, 1]), np.where(k == 0, b[:, 0], b[:, 1])


def _coverage(ref, md_ref, where):
    """what the comparison on this scene is worth: winners of every kind, intersections and misses, on the shim's answers"""
    which = ref["which"]
    s, u = _edge_parameters(ref)
    counts = dict(a=int(((which >= 0) & (which < 3)).sum()), b=int(((which >= 3) & (which < 6)).sum()),
                  c=int(((which >= 6) & (s > 0) & (s < 1) & (u > 0) & (u < 1)).sum()), meet=int((ref["intersections"] > 0).sum()),
                  miss=int(((md_ref["instance"] < 0) & (ref["instance"] >= 0)).sum()))
    print(where, "coverage", counts)
    assert counts["a"] >= 10, (where, "winners from (a)")
    assert counts["b"] >= 10, (where, "winners from (b)")
    assert counts["c"] >= 10, (where, "winners from (c) inside both edges")
    assert counts["meet"] >= 10, (where, "intersections")
    assert counts["miss"] >= 10, (where, "misses under max_distance")


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    """Every triangle family on c1, the multi-instance scene (rotation, non-uniform scale, texture), the demo scene and a 28-level
    tree, with every bound kind: equal to the shim bit for bit; on multi and demo the families reach every kind of winner."""
    desc, (W, H, K, pose) = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        fams, diag = qt.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        tris = qt.flatten(fams)
        got, ref = _check(sp, so, tris, where=name)
        md = _bounds(rng, ref, diag)
        got_md, ref_md = _check(sp, so, tris, md, where=name + " bounded")
        if name in ("multi", "demo"):
            _coverage(ref, ref_md, name)
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
        fams, diag = qt.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        tris = qt.flatten(fams)
        got, ref = _check(sp, so, tris, where=info)
        _check(sp, so, tris, _bounds(rng, ref, diag), where=info + " bounded")
    finally:
        sp.close()
        so.close()


@pytest.fixture(scope="module")
def multi(rt, orc, scenes, blob5k):
    """the multi-instance scene on both sides with its triangles and the shim's answers, computed once and left unchanged"""
    desc, (W, H, K, pose) = _library_scene("multi", scenes, blob5k, None)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    rng = np.random.default_rng(21)
    fams, diag = qt.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
    tris = qt.flatten(fams)
    ref = tdo.closest_to_triangles(so, tris)
    md = _bounds(rng, ref, diag)
    ref_md = tdo.closest_to_triangles(so, tris, md)
    yield dict(desc=desc, so=so, sp=sp, tris=tris, ref=ref, md=md, ref_md=ref_md, diag=diag, fams=fams)
    sp.close()
    so.close()


def test_max_distance_kinds(multi):
    """max_distance None, finite, 0, negative and NaN, and the inclusive boundary: the exact distance is within, its float predecessor
    is not."""
    sp, so, tris, ref = multi["sp"], multi["so"], multi["tris"], multi["ref"]
    n, d = len(tris), ref["distance"]
    for md, hit in ((None, True), (d, True), (np.nextafter(d, F32(0)), None), (np.nextafter(d, F32(np.inf)), True),
                    (np.full(n, np.inf, F32), True), (np.zeros(n, F32), None), (np.full(n, np.nan, F32), False),
                    (np.full(n, -1.0, F32), False), (np.full(n, multi["diag"] * 0.01, F32), None)):
        md = None if md is None else np.ascontiguousarray(md, F32)
        got = sp.closest_to_triangles(tris, md, outputs=ALL)
        _same(got, tdo.closest_to_triangles(so, tris, md), "bound")
        _definitions(got)
        if hit is not None:
            assert ((got["instance"] >= 0) == hit).all()
        assert np.array_equal(got["intersections"], ref["intersections"])       # the intersection half does not depend on the bound
    got = sp.closest_to_triangles(tris, np.ascontiguousarray(np.nextafter(d, F32(0)), F32))
    assert (got["instance"][d > 0] < 0).all() and (got["instance"][d == 0] >= 0).all()


def test_every_output_alone_and_all_together(multi):
    """Each field wanted alone gives the bits it has among all of them (the host chooses the kernels by the fields wanted)."""
    sp, tris, md, ref = multi["sp"], multi["tris"], multi["md"], multi["ref_md"]
    everything = sp.closest_to_triangles(tris, md, outputs=ALL)
    _same(everything, ref, "all together")
    for k in ALL:
        alone = sp.closest_to_triangles(tris, md, outputs=(k,))
        assert set(alone) == {k}
        if k == "pops":
            assert (alone[k] <= everything[k]).all() and (alone[k] >= 0).all()      # (alone: the first-candidate traversal)
        else:
            _same(alone, ref, "alone " + k, keys=(k,))
    pair = sp.closest_to_triangles(tris, md, outputs=("clearance", "within"))        # no intersections buffer, both patched in place
    _same(pair, ref, "clearance and within", keys=("clearance", "within"))


def test_agrees_with_the_point_and_intersection_queries(multi):
    """A triangle whose three vertices are equal is Scene.closest_points on the GPU for the fields they share; intersections is
    Scene.count_intersecting on the same triangles, with and without skip_instance."""
    sp, tris, md = multi["sp"], multi["tris"], multi["md"]
    pts = np.ascontiguousarray(tris[:, 0])
    point = np.ascontiguousarray(np.stack([pts, pts, pts], axis=1))
    for bound in (None, md):
        a = sp.closest_to_triangles(point, bound, outputs=SHARED + ("query_barycentric", "intersections", "query_point"))
        b = sp.closest_points(pts, bound, outputs=SHARED)
        _same(a, b, "point triangle", keys=SHARED)
        assert not a["query_barycentric"].any() and not a["intersections"].any()
    cc = sp.count_intersecting(tris, outputs=("count",))["count"]
    assert np.array_equal(cc, sp.closest_to_triangles(tris, outputs=("intersections",))["intersections"])
    assert np.array_equal(cc, multi["ref"]["intersections"]) and (cc > 0).sum() >= 10
    skip = (np.arange(len(tris)) % 4 - 1).astype(np.int32)
    cs = sp.count_intersecting(tris, skip, outputs=("count",))["count"]
    assert np.array_equal(cs, sp.closest_to_triangles(tris, None, skip, outputs=("intersections",))["intersections"])


def test_skip_instance(rt, orc, multi):
    """skip_instance per query on the multi-instance scene, and an instance's own world triangles with itself skipped: equal to the
    shim, and no result names the skipped instance."""
    sp, so, tris, md, desc = multi["sp"], multi["so"], multi["tris"], multi["md"], multi["desc"]
    ninst = len(desc.instances)
    rng = np.random.default_rng(2)
    skip = rng.integers(-1, ninst, len(tris)).astype(np.int32)
    got, ref = _check(sp, so, tris, md, skip, where="skip")
    assert (got["instance"][skip >= 0] != skip[skip >= 0]).all() and (got["instance"] >= 0).sum() >= 10
    assert (ref["instance"] != multi["ref_md"]["instance"]).sum() >= 10            # (skipping changed winners)
    o = orc.oracle()
    for k, (mesh, _mat, pose, scale) in enumerate(desc.instances):
        t = o.mesh_dump(desc.oracle_meshes[mesh])["tris"][:, :9].reshape(-1, 3, 3)
        t = t[np.isfinite(t).all(axis=(1, 2))][:60]
        own = np.ascontiguousarray(qp._world(o, pose, scale, t.reshape(-1, 3)).reshape(-1, 3, 3), F32)
        sk = np.full(len(own), k, np.int32)
        got, ref = _check(sp, so, own, None, sk, where="own triangles of instance %d" % k)
        assert (got["instance"] != k).all() and (got["instance"] >= 0).all()


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_wave_boundaries_on_the_deep_tree(rt, orc, scenes, n):
    """n around the 64 triangles of a wave, on the 28-level tree (the stack beyond its LDS part)."""
    desc, (W, H, K, pose) = _library_scene("deep", scenes, None, None)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        fams, diag = qt.families(np.random.default_rng(n), orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        tris = np.ascontiguousarray(qt.flatten(fams)[np.random.default_rng(n).permutation(130)[:n]])
        assert len(tris) == n
        _check(sp, so, tris, where="deep n = %d" % n)
    finally:
        sp.close()
        so.close()


def test_non_finite_triangles_and_guard_words(rt, multi):
    """Triangles with NaN / inf components between finite ones: the finite triangles' results equal the shim's, and nothing is written
    outside any output array (guard words before and after each of the thirteen, through the C ABI on buffers of the test's own)."""
    import torch
    sp, tris, md, ref = multi["sp"], multi["tris"], multi["md"], multi["ref_md"]
    rng = np.random.default_rng(6)
    n = len(tris)
    bad = tris.copy()
    sel = np.arange(n) % 3 == 1
    flat = bad.reshape(n, 9)
    flat[sel, rng.integers(0, 9, sel.sum())] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), sel.sum())
    G = 64
    fields = {k: rt._FIELDS[k] for k in ALL}
    bufs = {}
    for k, (shape, dt) in fields.items():
        per = int(np.prod(shape, dtype=np.int64))
        t = torch.full((n * per + 2 * G,), 90, dtype={np.float32: torch.float32, np.int32: torch.int32}[dt], device="cuda")
        bufs[k] = (t, per)
    guard = {k: t.clone() for k, (t, per) in bufs.items()}
    d_tris, d_md = torch.from_numpy(bad).cuda(), torch.from_numpy(md).cuda()
    hits = rt.RtTriangleHits(*[bufs[k][0].data_ptr() + G * 4 for k in rt.Scene.TRIANGLE_HIT_OUTPUTS])
    torch.cuda.synchronize()
    rc = rt.libs()[0].rt_closest_to_triangles(sp.device_handle, d_tris.data_ptr(), d_md.data_ptr(), None, n, C.byref(hits), None, 1)
    assert rc == 0
    got = {}
    for k, (t, per) in bufs.items():
        h, g = t.cpu().numpy(), guard[k].cpu().numpy()
        assert np.array_equal(h[:G].view(np.uint32), g[:G].view(np.uint32)) and np.array_equal(h[-G:].view(np.uint32), g[-G:].view(np.uint32)), k
        got[k] = h[G:-G].reshape((n,) + fields[k][0])
    _same({k: v[~sel] for k, v in got.items()}, {k: v[~sel] for k, v in ref.items()}, "finite beside non-finite")


def test_tree_independence_and_scene_changes(rt, orc, scenes, blob5k):
    """Host-built and device-built trees give the same bits; after refit_mesh, rebuild_mesh and an async update_mesh_instance on a
    stream the results equal the shim of the new state."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp, dev = _product(rt, desc), _product(rt, desc, for_device=True)
    o = orc.oracle()
    try:
        rng = np.random.default_rng(5)
        m = sd.MULTI_CAMERA
        fams, diag = qt.families(rng, o, desc, so, _cam_rays(scenes, 96, 54, scenes.scaled_K(96), m["pose"]), n=300)
        tris_q = qt.flatten(fams)
        got, ref = _check(sp, so, tris_q, where="host tree")
        _same(dev.closest_to_triangles(tris_q, outputs=ALL), ref, "device tree")
        md = _bounds(rng, ref, diag)
        tris = desc.meshes[1][1].copy()
        tris[:, [0, 3, 6]] += 0.05
        tris[:, [2, 5, 8]] -= 0.03
        sp.refit_mesh(1, tris)
        o.mesh_refit(desc.oracle_meshes[1], tris)
        _check(sp, so, tris_q, md, where="refit_mesh")
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        sp.rebuild_mesh(1, new)
        desc2 = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances)
        so2 = desc2.build_oracle(orc)
        so.close()
        so = so2
        _check(sp, so, tris_q, md, where="rebuild_mesh")
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        sp.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        with torch.cuda.stream(s):
            tg = sp.closest_to_triangles(torch.from_numpy(tris_q).cuda(), torch.from_numpy(md).cuda(), outputs=ALL)
        s.synchronize()
        _same({k: v.cpu().numpy() for k, v in tg.items()}, tdo.closest_to_triangles(so, tris_q, md), "update_mesh_instance(stream)")
    finally:
        sp.close()
        dev.close()
        so.close()


def test_call_shapes_streams_and_threads(multi):
    """n = 0, a [.., 3, 3] leading shape, the numpy path, torch on the current stream, on a torch.cuda.Stream and on its raw handle, two
    streams with calls in flight at once, and four host threads on one scene."""
    import torch
    sp, tris, md, ref = multi["sp"], multi["tris"], multi["md"], multi["ref_md"]
    n = len(tris)
    empty = sp.closest_to_triangles(tris[:0], outputs=ALL)
    assert all(v.shape[0] == 0 for v in empty.values())
    m = n // 4 * 4
    lead = sp.closest_to_triangles(tris[:m].reshape(4, m // 4, 3, 3), md[:m].reshape(4, m // 4), outputs=("distance", "query_point", "within"))
    _same(lead, {k: v[:m].reshape((4, m // 4) + v.shape[1:]) for k, v in ref.items()}, "[4, m, 3, 3]", keys=("distance", "query_point", "within"))
    tt, tm = torch.from_numpy(tris).cuda(), torch.from_numpy(md).cuda()
    torch.cuda.synchronize()

    def host(d):
        return {k: v.cpu().numpy() for k, v in d.items()}
    cur = sp.closest_to_triangles(tt, tm, outputs=ALL)
    torch.cuda.synchronize()
    _same(host(cur), ref, "torch, current stream")
    assert cur["within"].dtype == torch.int32 and cur["distance"].dtype == torch.float32
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = sp.closest_to_triangles(tt, tm, outputs=ALL, stream=s1)
    b = sp.closest_to_triangles(tt, None, outputs=ALL, stream=s2.cuda_stream)       # (the raw handle; in flight beside a)
    c = sp.closest_to_triangles(tt, tm, outputs=("within",), stream=s1)
    s1.synchronize()
    s2.synchronize()
    _same(host(a), ref, "torch.cuda.Stream")
    _same(host(b), multi["ref"], "raw stream handle")
    _same(host(c), ref, "second call on the stream", keys=("within",))
    errors = []

    def work(j):
        try:
            for r in range(3):
                if j % 2:
                    _same(sp.closest_to_triangles(tris, md, outputs=ALL), ref, "thread %d numpy" % j)
                else:
                    st = torch.cuda.Stream()
                    g = sp.closest_to_triangles(tt, tm, outputs=ALL, stream=st)
                    st.synchronize()
                    _same(host(g), ref, "thread %d torch" % j)
        except BaseException as e:                      # (an assertion in a thread must fail the test)
            errors.append(e)
    threads = [threading.Thread(target=work, args=(j,)) for j in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]


def test_pruning_is_real(rt, orc, scenes, demo_objs):
    """On the demo scene, mean pops of the small triangles at the surface stays under 1 % of the interior nodes."""
    desc, (W, H, K, pose) = _library_scene("demo", scenes, None, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        fams, diag = qt.families(np.random.default_rng(3), orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=1200)
        tris = dict(fams)["surface_small"]
        assert len(tris) >= 100
        got = sp.closest_to_triangles(tris, outputs=ALL)
        _same(got, tdo.closest_to_triangles(so, tris), "demo surface")
        o = orc.oracle()
        interior = sum(int((o.mesh_dump(desc.oracle_meshes[mesh])["child"][:, 0] > 0).sum()) for mesh, _m, _p, _s in desc.instances)
        print("mean pops %.1f of %d interior nodes" % (got["pops"].mean(), interior))
        assert got["pops"].mean() < 0.01 * interior, (got["pops"].mean(), interior)
    finally:
        sp.close()
        so.close()
