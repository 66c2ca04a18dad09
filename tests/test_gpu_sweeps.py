"""Sphere sweeps on the GPU (rt_sweep_spheres through Scene.sweep_spheres): every output but `pops` is compared bit for bit with the
brute-force shim over the test oracle's scene (tests/sweep_oracle.c), on the library's scenes, the adversarial scenes of
scene_defs.adversarial_scene, after scene changes and under every call shape.  `pops` is only bounded.  The coverage the comparison
relies on (winners from the face, an edge, a vertex and the start, and misses) is asserted on the shim's answers."""
import ctypes as C
import threading

import numpy as np
import pytest

import query_sweeps as qw
import scene_defs as sd
import sweep_oracle
from test_gpu_point_query import SEEDS, _bits, _cam_rays, _library_scene, _product

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
EXACT = sweep_oracle.OUTPUTS
ALL = EXACT + ("pops",)
SHARED = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")      # with Scene.closest_points


def _same(got, ref, where="", keys=EXACT):
    """bit for bit; NaN outputs compare equal whatever their bits (the point tests' rule)"""
    for k in keys:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and g.dtype == r.dtype, (where, k, g.shape, r.shape, g.dtype, r.dtype)
        bad = np.flatnonzero((_bits(g) != _bits(r)).reshape(g.shape[0] if g.ndim else 1, -1).any(axis=-1))
        assert bad.size == 0, "%s %s: %d sweeps differ, first %s: got %s want %s" % (where, k, bad.size, bad[:3], g[bad[:3]], r[bad[:3]])


def _definitions(got, where=""):
    """hit == (there is a winner); the miss values; time in [0, 1] on a hit"""
    hit = got["instance"] >= 0
    assert np.array_equal(got["hit"], hit.astype(np.int32)), where
    assert (got["time"][~hit] == FLT_MAX).all() and (got["distance"][~hit] == FLT_MAX).all() and (got["triangle"][~hit] == -1).all(), where
    assert ((got["time"][hit] >= 0) & (got["time"][hit] <= 1)).all(), where
    for k in ("centre", "point", "normal", "contact_normal", "barycentric", "uv"):
        assert not got[k][~hit].any(), (where, k)


def _check(sp, so, segs, rad, where=""):
    got = sp.sweep_spheres(segs, rad, outputs=ALL)
    ref = sweep_oracle.sweep_spheres(so, segs, rad)
    _same(got, ref, where)
    _definitions(got, where)
    assert (got["pops"] >= 0).all(), where
    fast = sp.sweep_spheres(segs, rad, outputs=("hit", "pops"))                 # the traversal that ends at the first valid candidate
    assert np.array_equal(fast["hit"], ref["hit"]), where
    assert (fast["pops"] <= got["pops"]).all(), where
    return got, ref


def coverage(ref, where):
    """what the comparison on this scene is worth: winners of every kind and misses, on the shim's answers"""
    which = ref["which"]
    assert (which == 1).sum() >= 10, (where, "face winners", np.bincount(which + 1, minlength=9))
    assert ((which >= 2) & (which <= 4)).sum() >= 10, (where, "edge winners", np.bincount(which + 1, minlength=9))
    assert (which >= 5).sum() >= 10, (where, "vertex winners", np.bincount(which + 1, minlength=9))
    assert (which == 0).sum() >= 10, (where, "start winners", np.bincount(which + 1, minlength=9))
    assert (which < 0).sum() >= 10, (where, "misses", np.bincount(which + 1, minlength=9))


@pytest.mark.parametrize("name", ["c1", "multi", "demo", "deep"])
def test_library_scenes_equal_oracle(rt, orc, scenes, blob5k, demo_objs, name):
    """Every sweep family on c1, the multi-instance scene (rotation, non-uniform scale, texture), the demo scene and a 28-level tree:
    equal to the shim bit for bit; on multi and demo the families reach every kind of winner."""
    desc, (W, H, K, pose) = _library_scene(name, scenes, blob5k, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(7)
        fams, diag = qw.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        segs, rad = qw.flatten(fams)
        got, ref = _check(sp, so, segs, rad, where=name)
        if name in ("multi", "demo"):
            coverage(ref, name)
    finally:
        sp.close()
        so.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_adversarial_scenes_equal_oracle(rt, orc, scenes, seed):
    """The render fuzz's adversarial scenes (lattices, degenerate and needle triangles, piles above 30 per leaf, 1e18 and 1e-20
    coordinates, non-finite vertices; mirrored, tiny and huge scales): every family equal to the shim."""
    desc, W, H, K, pose, info = sd.adversarial_scene(scenes, np.random.default_rng(91000 + seed))
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        rng = np.random.default_rng(seed)
        fams, diag = qw.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        segs, rad = qw.flatten(fams)
        _check(sp, so, segs, rad, where=info)
    finally:
        sp.close()
        so.close()


@pytest.fixture(scope="module")
def multi(rt, orc, scenes, blob5k):
    """the multi-instance scene on both sides with its sweeps and the shim's answers, computed once and left unchanged"""
    desc, (W, H, K, pose) = _library_scene("multi", scenes, blob5k, None)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    rng = np.random.default_rng(21)
    fams, diag = qw.families(rng, orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
    segs, rad = qw.flatten(fams)
    ref = sweep_oracle.sweep_spheres(so, segs, rad)
    yield dict(desc=desc, so=so, sp=sp, segs=segs, rad=rad, ref=ref, diag=diag, fams=fams)
    sp.close()
    so.close()


def test_every_output_alone_and_all_together(multi):
    """Each field wanted alone gives the bits it has among all of them (the host chooses the kernel by the fields wanted)."""
    sp, segs, rad, ref = multi["sp"], multi["segs"], multi["rad"], multi["ref"]
    everything = sp.sweep_spheres(segs, rad, outputs=ALL)
    _same(everything, ref, "all together")
    for k in ALL:
        alone = sp.sweep_spheres(segs, rad, outputs=(k,))
        assert set(alone) == {k}
        if k == "pops":
            assert (alone[k] <= everything[k]).all() and (alone[k] >= 0).all()      # (alone: the first-candidate traversal)
        else:
            _same(alone, ref, "alone " + k, keys=(k,))
    assert set(sp.sweep_spheres(segs, rad)) == {"time", "instance", "triangle"}


def test_time_zero_is_the_point_query(multi):
    """Where the sphere starts in contact the sweep is Scene.closest_points(P0, max_distance=r) on the GPU for the fields they share,
    bit for bit; and wherever that query has a winner, the sweep's time is 0."""
    sp, segs, rad = multi["sp"], multi["segs"], multi["rad"]
    pts = np.ascontiguousarray(segs[:, 0])
    a = sp.sweep_spheres(segs, rad, outputs=SHARED + ("time",))
    b = sp.closest_points(pts, rad, outputs=SHARED)
    at = b["instance"] >= 0
    assert at.sum() >= 10
    assert (a["time"][at] == 0).all()
    _same({k: v[at] for k, v in a.items()}, {k: v[at] for k, v in b.items()}, "time 0", keys=SHARED)
    zero = np.ascontiguousarray(np.stack([pts, pts], axis=1))
    z = sp.sweep_spheres(zero, rad, outputs=SHARED + ("time",))
    _same({k: v[at] for k, v in z.items()}, {k: v[at] for k, v in b.items()}, "zero length", keys=SHARED)
    assert (z["time"][z["instance"] >= 0] == 0).all()


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_wave_boundaries_on_the_deep_tree(rt, orc, scenes, n):
    """n around the 64 sweeps of a wave, on the 28-level tree (the stack beyond its LDS part)."""
    desc, (W, H, K, pose) = _library_scene("deep", scenes, None, None)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        fams, diag = qw.families(np.random.default_rng(n), orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=300)
        segs, rad = qw.flatten(fams)
        sel = np.random.default_rng(n).permutation(130)[:n]
        segs, rad = np.ascontiguousarray(segs[sel]), np.ascontiguousarray(rad[sel])
        assert len(segs) == n
        _check(sp, so, segs, rad, where="deep n = %d" % n)
    finally:
        sp.close()
        so.close()


def test_non_finite_sweeps_and_guard_words(rt, multi):
    """Sweeps with NaN / inf components between finite ones: the finite sweeps' results equal the shim's, and nothing is written
    outside any of the twelve output arrays (guard words before and after each, through the C ABI on buffers of the test's own)."""
    import torch
    sp, segs, rad, ref = multi["sp"], multi["segs"], multi["rad"], multi["ref"]
    rng = np.random.default_rng(6)
    n = len(segs)
    bad = segs.copy()
    sel = np.arange(n) % 3 == 1
    flat = bad.reshape(n, 6)
    flat[sel, rng.integers(0, 6, sel.sum())] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), sel.sum())
    G = 64
    fields = {k: rt._FIELDS[k] for k in ALL}
    assert len(fields) == 12
    bufs = {}
    for k, (shape, dt) in fields.items():
        per = int(np.prod(shape, dtype=np.int64))
        t = torch.full((n * per + 2 * G,), 90, dtype={np.float32: torch.float32, np.int32: torch.int32}[dt], device="cuda")
        bufs[k] = (t, per)
    guard = {k: t.clone() for k, (t, per) in bufs.items()}
    d_segs, d_rad = torch.from_numpy(bad).cuda(), torch.from_numpy(rad).cuda()
    hits = rt.RtSweepHits(*[bufs[k][0].data_ptr() + G * 4 for k in rt.Scene.SWEEP_OUTPUTS])
    torch.cuda.synchronize()
    rc = rt.libs()[0].rt_sweep_spheres(sp.device_handle, d_segs.data_ptr(), d_rad.data_ptr(), n, C.byref(hits), None, 1)
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
        fams, diag = qw.families(rng, o, desc, so, _cam_rays(scenes, 96, 54, scenes.scaled_K(96), m["pose"]), n=300)
        segs, rad = qw.flatten(fams)
        got, ref = _check(sp, so, segs, rad, where="host tree")
        _same(dev.sweep_spheres(segs, rad, outputs=ALL), ref, "device tree")
        tris = desc.meshes[1][1].copy()
        tris[:, [0, 3, 6]] += 0.05
        tris[:, [2, 5, 8]] -= 0.03
        sp.refit_mesh(1, tris)
        o.mesh_refit(desc.oracle_meshes[1], tris)
        _check(sp, so, segs, rad, where="refit_mesh")
        new = sd.random_triangles(200, seed=12, spread=0.8, size=0.3)
        sp.rebuild_mesh(1, new)
        desc2 = sd.SceneDesc(desc.materials, [desc.meshes[0], ("tris", new)] + desc.meshes[2:], desc.instances)
        so2 = desc2.build_oracle(orc)
        so.close()
        so = so2
        _check(sp, so, segs, rad, where="rebuild_mesh")
        s = torch.cuda.Stream()
        pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, -0.8, 1.2)
        sp.update_mesh_instance(0, 0, 2, pose, scale, stream=s.cuda_stream)
        so.update_instance(0, 0, 2, pose, scale)
        with torch.cuda.stream(s):
            tg = sp.sweep_spheres(torch.from_numpy(segs).cuda(), torch.from_numpy(rad).cuda(), outputs=ALL)
        s.synchronize()
        _same({k: v.cpu().numpy() for k, v in tg.items()}, sweep_oracle.sweep_spheres(so, segs, rad), "update_mesh_instance(stream)")
    finally:
        sp.close()
        dev.close()
        so.close()


def test_call_shapes_streams_and_threads(multi):
    """n = 0, a [.., 2, 3] leading shape, the numpy path, torch on the current stream, on a torch.cuda.Stream and on its raw handle, two
    streams with calls in flight at once, and four host threads on one scene."""
    import torch
    sp, segs, rad, ref = multi["sp"], multi["segs"], multi["rad"], multi["ref"]
    n = len(segs)
    empty = sp.sweep_spheres(segs[:0], rad[:0], outputs=ALL)
    assert all(v.shape[0] == 0 for v in empty.values())
    m = n // 4 * 4
    lead = sp.sweep_spheres(segs[:m].reshape(4, m // 4, 2, 3), rad[:m].reshape(4, m // 4), outputs=("time", "centre", "hit"))
    _same(lead, {k: v[:m].reshape((4, m // 4) + v.shape[1:]) for k, v in ref.items()}, "[4, m, 2, 3]", keys=("time", "centre", "hit"))
    ts, tr = torch.from_numpy(segs).cuda(), torch.from_numpy(rad).cuda()
    torch.cuda.synchronize()

    def host(d):
        return {k: v.cpu().numpy() for k, v in d.items()}
    cur = sp.sweep_spheres(ts, tr, outputs=ALL)
    torch.cuda.synchronize()
    _same(host(cur), ref, "torch, current stream")
    assert cur["hit"].dtype == torch.int32 and cur["time"].dtype == torch.float32
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = sp.sweep_spheres(ts, tr, outputs=ALL, stream=s1)
    b = sp.sweep_spheres(ts, tr, outputs=ALL, stream=s2.cuda_stream)             # (the raw handle; in flight beside a)
    c = sp.sweep_spheres(ts, tr, outputs=("hit",), stream=s1)
    s1.synchronize()
    s2.synchronize()
    _same(host(a), ref, "torch.cuda.Stream")
    _same(host(b), ref, "raw stream handle")
    _same(host(c), ref, "second call on the stream", keys=("hit",))
    errors = []

    def work(j):
        try:
            for r in range(3):
                if j % 2:
                    _same(sp.sweep_spheres(segs, rad, outputs=ALL), ref, "thread %d numpy" % j)
                else:
                    st = torch.cuda.Stream()
                    g = sp.sweep_spheres(ts, tr, outputs=ALL, stream=st)
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
    """On the demo scene, mean pops of the short sweeps at the surface (length and radius 1e-3 of the diagonal) stays under 1 % of
    the interior nodes."""
    desc, (W, H, K, pose) = _library_scene("demo", scenes, None, demo_objs)
    so = desc.build_oracle(orc)
    sp = _product(rt, desc)
    try:
        fams, diag = qw.families(np.random.default_rng(3), orc.oracle(), desc, so, _cam_rays(scenes, W, H, K, pose), n=2400)
        segs, rad = next((s, r) for name, s, r in fams if name == "surface_short")
        assert len(segs) >= 100
        got = sp.sweep_spheres(segs, rad, outputs=ALL)
        _same(got, sweep_oracle.sweep_spheres(so, segs, rad), "demo surface")
        o = orc.oracle()
        interior = sum(int((o.mesh_dump(desc.oracle_meshes[mesh])["child"][:, 0] > 0).sum()) for mesh, _m, _p, _s in desc.instances)
        print("mean pops %.1f of %d interior nodes" % (got["pops"].mean(), interior))
        assert got["pops"].mean() < 0.01 * interior, (got["pops"].mean(), interior)
    finally:
        sp.close()
        so.close()
