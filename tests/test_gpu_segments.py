"""Segment queries on the GPU (rt_closest_to_segments through Scene.closest_to_segments): every output but `pops` is compared bit for bit
with the brute-force shim over the test oracle's scene (tests/segment_oracle.c), on the library's scenes, the adversarial scenes of
scene_defs.adversarial_scene, after scene changes and under every call shape.  `pops` is only bounded.  The coverage the comparison
relies on (edge and end winners, crossings, misses) is asserted on the shim's answers."""
import ctypes as C
import threading

import numpy as np
import pytest

import query_points as qp
import query_segments as qs
import scene_defs as sd
import segment_oracle
from test_gpu_point_query import SEEDS, _bits, _cam_rays, _library_scene, _product

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
EXACT = segment_oracle.OUTPUTS
ALL = EXACT + ("pops",)
SHARED = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")      # with Scene.closest_points


def _same(got, ref, where="", keys=EXACT):
    """bit for bit; NaN outputs compare equal whatever their bits (the point tests' rule)"""
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and g.dtype == r.dtype, (where, k, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.flatnonzero((_bits(g) != _bits(r)).reshape(g.shape[0] if g.ndim else 1, -1).any(axis=-1))
        assert bad.size == 0, "%s %s: %d segments differ, first %s: got %s want %s" % (where, k, bad.size, bad[:3], g[bad[:3]], r[bad[:3]])


def _definitions(got, where=""):
    """within == (a distance candidate || crossings > 0); clearance by its definition"""
    cand = got["instance"] >= 0
    assert np.array_equal(got["within"], (cand | (got["crossings"] > 0)).astype(np.int32)), where
    assert np.array_equal(_bits(got["clearance"]), _bits(np.where(got["crossings"] > 0, F32(0), got["distance"]).astype(F32))), where
    assert (got["distance"][~cand] == FLT_MAX).all() and (got["triangle"][~cand] == -1).all(), where
    assert ((got["parameter"] >= 0) & (got["parameter"] <= 1)).all(), where


def _check(sp, so, segs, md=None, where=""):
    got = sp.closest_to_segments(segs, md, outputs=ALL)
    ref = segment_oracle.closest_to_segments(so, segs, md)
    _same(got, ref, where)
    _definitions(got, where)
    assert (got["pops"] >= 0).all(), where
    fast = sp.closest_to_segments(segs, md, outputs=("within", "pops"))         # the traversal that ends at the first candidate
    assert np.array_equal(fast["within"], ref["within"]), where
    assert (fast["pops"] <= got["pops"]).all(), where
    return got, ref


def _bounds(rng, ref, diag):
    """max_distance per segment: +inf, 0, the exact distance and its float neighbours, NaN, negative, fractions of the distance, and a
    small radius (misses, and pierced triangles out of the minimum's reach)"""
    md = qp.special_bounds(rng, ref["distance"])
    small = rng.random(len(md)) < 0.25
    md[small] = F32(diag) * F32(1e-4)
    return md


def _coverage(ref, md_ref, where):
    """what the comparison on this scene is worth: winners of every kind, crossings and misses, on the shim's answers"""
    s, which = ref["parameter"], ref["which"]
    assert ((which >= 2) & (s > 0) & (s < 1)).sum() >= 10, (where, "edge winners inside the segment")
    assert ((which == 0) | (which == 1)).sum() >= 10, (where, "end winners")
    assert (ref["crossings"] > 0).sum() >= 10, (where, "crossings")
    assert ((md_ref["instance"] < 0) & (ref["instance"] >= 0)).sum() >= 10, (where, "misses under max_distance")
    assert ((md_ref["instance"] < 0) & (md_ref["crossings"] > 0)).sum() >= 3, (where, "pierced beyond the radius")


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    """Every segment family on c1, the multi-instance scene (rotation, non-uniform scale, texture), the demo scene and a 28-level tree,
    with every radius kind: equal to the shim bit for bit; on multi and demo the families reach every kind of winner."""
    desc, (W, H, K, pose) = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        fams, diag = qs.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        segs = qs.flatten(fams)
        got, ref = _check(sp, so, segs, where=name)
        md = _bounds(rng, ref, diag)
        got_md, ref_md = _check(sp, so, segs, md, where=name + " bounded")
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
        fams, diag = qs.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        segs = qs.flatten(fams)
        got, ref = _check(sp, so, segs, where=info)
        _check(sp, so, segs, _bounds(rng, ref, diag), where=info + " bounded")
    finally:
        sp.close()
        so.close()


@pytest.fixture(scope="module")
def multi(rt, orc, scenes, blob5k):
    """the multi-instance scene on both sides with its segments and the shim's answers, computed once and left unchanged"""
    desc, (W, H, K, pose) = _library_scene("multi", scenes, blob5k, None)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    rng = np.random.default_rng(21)
    fams, diag = qs.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
    segs = qs.flatten(fams)
    ref = segment_oracle.closest_to_segments(so, segs)
    md = _bounds(rng, ref, diag)
    ref_md = segment_oracle.closest_to_segments(so, segs, md)
    yield dict(desc=desc, so=so, sp=sp, segs=segs, ref=ref, md=md, ref_md=ref_md, diag=diag, fams=fams)
    sp.close()
    so.close()


def test_max_distance_kinds(multi):
    """max_distance None, finite, 0, negative and NaN, and the inclusive boundary: the exact distance is within, its float predecessor
    is not."""
    sp, so, segs, ref = multi["sp"], multi["so"], multi["segs"], multi["ref"]
    n, d = len(segs), ref["distance"]
    for md, hit in ((None, True), (d, True), (np.nextafter(d, F32(0)), None), (np.full(n, np.inf, F32), True), (np.zeros(n, F32), None),
                    (np.full(n, np.nan, F32), False), (np.full(n, -1.0, F32), False), (np.full(n, multi["diag"] * 0.01, F32), None)):
        md = None if md is None else np.ascontiguousarray(md, F32)
        got = sp.closest_to_segments(segs, md, outputs=ALL)
        _same(got, segment_oracle.closest_to_segments(so, segs, md), "radius")
        _definitions(got)
        if hit is not None:
            assert ((got["instance"] >= 0) == hit).all()
        assert np.array_equal(got["crossings"], ref["crossings"])       # the crossing half does not depend on the radius
    got = sp.closest_to_segments(segs, np.ascontiguousarray(np.nextafter(d, F32(0)), F32))
    assert (got["instance"][d > 0] < 0).all() and (got["instance"][d == 0] >= 0).all()


def test_every_output_alone_and_all_together(multi):
    """Each field wanted alone gives the bits it has among all of them (the host chooses the kernels by the fields wanted)."""
    sp, segs, md, ref = multi["sp"], multi["segs"], multi["md"], multi["ref_md"]
    everything = sp.closest_to_segments(segs, md, outputs=ALL)
    _same(everything, ref, "all together")
    for k in ALL:
        alone = sp.closest_to_segments(segs, md, outputs=(k,))
        assert set(alone) == {k}
        if k == "pops":
            assert (alone[k] <= everything[k]).all() and (alone[k] >= 0).all()      # (alone: the first-candidate traversal)
        else:
            _same(alone, ref, "alone " + k, keys=(k,))
    pair = sp.closest_to_segments(segs, md, outputs=("clearance", "within"))         # no crossings buffer, both patched in place
    _same(pair, ref, "clearance and within", keys=("clearance", "within"))


def test_agrees_with_the_point_and_crossing_queries(multi):
    """A zero-length segment is Scene.closest_points on the GPU for the fields they share; crossings is Scene.count_crossings for
    origins P0, directions P1 - P0 and tmax 1."""
    sp, segs, md = multi["sp"], multi["segs"], multi["md"]
    pts = np.ascontiguousarray(segs[:, 0])
    zero = np.ascontiguousarray(np.stack([pts, pts], axis=1))
    for bound in (None, md):
        a = sp.closest_to_segments(zero, bound, outputs=SHARED + ("parameter", "crossings", "segment_point"))
        b = sp.closest_points(pts, bound, outputs=SHARED)
        _same(a, b, "zero length", keys=SHARED)
        assert not a["parameter"].any() and not a["crossings"].any()
    d = np.ascontiguousarray(segs[:, 1] - segs[:, 0], F32)
    cc = sp.count_crossings(pts, d, np.ones(len(segs), F32), outputs=("count",))["count"]
    assert np.array_equal(cc, sp.closest_to_segments(segs, outputs=("crossings",))["crossings"])
    assert np.array_equal(cc, multi["ref"]["crossings"]) and (cc > 0).sum() >= 10


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_wave_boundaries_on_the_deep_tree(rt, orc, scenes, n):
    """n around the 64 segments of a wave, on the 28-level tree (the stack beyond its LDS part)."""
    desc, (W, H, K, pose) = _library_scene("deep", scenes, None, None)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        fams, diag = qs.families(np.random.default_rng(n), orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        segs = np.ascontiguousarray(qs.flatten(fams)[np.random.default_rng(n).permutation(130)[:n]])
        assert len(segs) == n
        _check(sp, so, segs, where="deep n = %d" % n)
    finally:
        sp.close()
        so.close()


def test_non_finite_segments_and_guard_words(rt, multi):
    """Segments with NaN / inf components between finite ones: the finite segments' results equal the shim's, and nothing is written
    outside any output array (guard words before and after each, through the C ABI on buffers of the test's own)."""
    import torch
    sp, segs, md, ref = multi["sp"], multi["segs"], multi["md"], multi["ref_md"]
    rng = np.random.default_rng(6)
    n = len(segs)
    bad = segs.copy()
    sel = np.arange(n) % 3 == 1
    flat = bad.reshape(n, 6)
    flat[sel, rng.integers(0, 6, sel.sum())] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), sel.sum())
    G = 64
    fields = {k: rt._FIELDS[k] for k in ALL}
    bufs = {}
    for k, (shape, dt) in fields.items():
        per = int(np.prod(shape, dtype=np.int64))
        t = torch.full((n * per + 2 * G,), 90, dtype={np.float32: torch.float32, np.int32: torch.int32}[dt], device="cuda")
        bufs[k] = (t, per)
    guard = {k: t.clone() for k, (t, per) in bufs.items()}
    d_segs, d_md = torch.from_numpy(bad).cuda(), torch.from_numpy(md).cuda()
    hits = rt.RtSegmentHits(*[bufs[k][0].data_ptr() + G * 4 for k in rt.Scene.SEGMENT_OUTPUTS])
    torch.cuda.synchronize()
    rc = rt.libs()[0].rt_closest_to_segments(sp.device_handle, d_segs.data_ptr(), d_md.data_ptr(), n, C.byref(hits), None, 1)
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
        fams, diag = qs.families(rng, o, desc, so, _cam_rays(scenes, 96, 54, scenes.scaled_K(96), m["pose"]), n=300)
        segs = qs.flatten(fams)
        got, ref = _check(sp, so, segs, where="host tree")
        _same(dev.closest_to_segments(segs, outputs=ALL), ref, "device tree")
        md = _bounds(rng, ref, diag)
        tris = desc.meshes[1][1].copy()
        tris[:, [0, 3, 6]] += 0.05
        tris[:, [2, 5, 8]] -= 0.03
        sp.refit_mesh(1, tris)
        o.mesh_refit(desc.oracle_meshes[1], tris)
        _check(sp, so, segs, md, where="refit_mesh")
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        sp.rebuild_mesh(1, new)
        desc2 = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances)
        so2 = desc2.build_oracle(orc)
        so.close()
        so = so2
        _check(sp, so, segs, md, where="rebuild_mesh")
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        sp.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        with torch.cuda.stream(s):
            tg = sp.closest_to_segments(torch.from_numpy(segs).cuda(), torch.from_numpy(md).cuda(), outputs=ALL)
        s.synchronize()
        _same({k: v.cpu().numpy() for k, v in tg.items()}, segment_oracle.closest_to_segments(so, segs, md), "update_mesh_instance(stream)")
    finally:
        sp.close()
        dev.close()
        so.close()


def test_call_shapes_streams_and_threads(multi):
    """n = 0, a [.., 2, 3] leading shape, the numpy path, torch on the current stream, on a torch.cuda.Stream and on its raw handle, two
    streams with calls in flight at once, and four host threads on one scene."""
    import torch
    sp, segs, md, ref = multi["sp"], multi["segs"], multi["md"], multi["ref_md"]
    n = len(segs)
    empty = sp.closest_to_segments(segs[:0], outputs=ALL)
    assert all(v.shape[0] == 0 for v in empty.values())
    m = n // 4 * 4
    lead = sp.closest_to_segments(segs[:m].reshape(4, m // 4, 2, 3), md[:m].reshape(4, m // 4), outputs=("distance", "segment_point", "within"))
    _same(lead, {k: v[:m].reshape((4, m // 4) + v.shape[1:]) for k, v in ref.items()}, "[4, m, 2, 3]", keys=("distance", "segment_point", "within"))
    ts, tm = torch.from_numpy(segs).cuda(), torch.from_numpy(md).cuda()
    torch.cuda.synchronize()

    def host(d):
        return {k: v.cpu().numpy() for k, v in d.items()}
    cur = sp.closest_to_segments(ts, tm, outputs=ALL)
    torch.cuda.synchronize()
    _same(host(cur), ref, "torch, current stream")
    assert cur["within"].dtype == torch.int32 and cur["distance"].dtype == torch.float32
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = sp.closest_to_segments(ts, tm, outputs=ALL, stream=s1)
    b = sp.closest_to_segments(ts, None, outputs=ALL, stream=s2.cuda_stream)        # (the raw handle; in flight beside a)
    c = sp.closest_to_segments(ts, tm, outputs=("within",), stream=s1)
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
                    _same(sp.closest_to_segments(segs, md, outputs=ALL), ref, "thread %d numpy" % j)
                else:
                    st = torch.cuda.Stream()
                    g = sp.closest_to_segments(ts, tm, outputs=ALL, stream=st)
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
    """On the demo scene, mean pops of the segments of 1e-3 of the diagonal at the surface stays under 1 % of the interior nodes."""
    desc, (W, H, K, pose) = _library_scene("demo", scenes, None, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        fams, diag = qs.families(np.random.default_rng(3), orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=1200)
        segs = dict(fams)["surface_short"]
        assert len(segs) >= 100
        got = sp.closest_to_segments(segs, outputs=ALL)
        _same(got, segment_oracle.closest_to_segments(so, segs), "demo surface")
        o = orc.oracle()
        interior = sum(int((o.mesh_dump(desc.oracle_meshes[mesh])["child"][:, 0] > 0).sum()) for mesh, _m, _p, _s in desc.instances)
        print("mean pops %.1f of %d interior nodes" % (got["pops"].mean(), interior))
        assert got["pops"].mean() < 0.01 * interior, (got["pops"].mean(), interior)
    finally:
        sp.close()
        so.close()
