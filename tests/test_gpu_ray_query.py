"""Ray queries on the GPU (rt_trace_rays / rt_occluded / rt_camera_rays through Scene.trace_rays / Scene.occluded / Camera.rays):
every comparison is bit for bit -- against the test oracle's cast_ray_lp / camera_ray on the same rays (tests/ray_oracle.c) and
against the production render kernel's hit ids (rt_render_ids)."""
import numpy as np
import pytest

import ray_oracle
import scene_defs as sd

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max
ALL = ("t", "instance", "triangle", "location", "normal", "uv", "pops")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_rays(a, b):
    """bit for bit, except that a NaN equals a NaN whatever its payload and sign (the reference's ray through the principal point is
    0 / 0: the GPU and the CPU spell that NaN differently)"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(_bits(np.where(na, 0, a).astype(np.float32)), _bits(np.where(nb, 0, b).astype(np.float32)))


def _same(got, ref, keys=ALL, where=""):
    for k in keys:
        g, r = got[k], ref[k]
        assert g.shape == r.shape, (k, g.shape, r.shape, where)
        bad = np.flatnonzero((_bits(g) != _bits(r)).reshape(g.shape[0] if g.ndim else 1, -1).any(axis=-1))
        assert bad.size == 0, "%s %s: %d rays differ, first %s: got %s want %s" % (where, k, bad.size, bad[:3], g[bad[:3]], r[bad[:3]])


def _camera(rt, W, H, K, D, pose):
    cam = rt.Camera(W, H, K, D)
    cam.set_pose(pose)
    return cam


def _flat(o, d):
    return np.ascontiguousarray(o.reshape(-1, 3)), np.ascontiguousarray(d.reshape(-1, 3))


def _random_rays(rng, n, lo, hi, hits=None):
    """uniform origins in the box [lo, hi] (some inside the meshes), uniform directions on the sphere; one ray in eight axis-aligned
    with +-0 components; with `hits` (world locations of earlier hits), one ray in four starts exactly there (no epsilon)."""
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ax = rng.integers(0, 3, n)
    sel = np.arange(n) % 8 == 3
    z = np.where(rng.random((n, 3)) < 0.5, np.float32(0.0), np.float32(-0.0))
    d[sel] = z[sel]
    d[sel, ax[sel]] = np.where(rng.random(sel.sum()) < 0.5, 1.0, -1.0)
    if hits is not None and len(hits):
        sec = np.arange(n) % 4 == 1
        o[sec] = hits[rng.integers(0, len(hits), sec.sum())]
    return o, d.astype(np.float32)


def test_camera_rays_equal_oracle(rt, scenes):
    """Camera.rays() is the oracle's camera_ray for every pixel (numpy and torch paths)."""
    c1 = scenes.C1
    for W, H, K, pose in ((c1["width"], c1["height"], c1["K"], c1["cam_pose"]), (320, 180, scenes.scaled_K(320), scenes.C2_CAMERAS["mid"])):
        cam = _camera(rt, W, H, K, scenes.D_REF if W == 320 else c1["D"], pose)
        o, d = cam.rays(as_numpy=True)
        ro, rd = ray_oracle.camera_rays(W, H, K, scenes.D_REF if W == 320 else c1["D"], pose)
        assert o.shape == (H, W, 3) and _same_rays(o, ro) and _same_rays(d, rd)
        assert np.isnan(d).sum() == (3 if W == 256 else 0)      # (C1's K puts the principal point on pixel (128, 128))
        import torch
        to, td = cam.rays()
        torch.cuda.synchronize()
        assert _same_rays(to.cpu().numpy(), ro) and _same_rays(td.cpu().numpy(), rd)


def test_camera_queries_equal_render_ids_full_size(rt, orc, scenes, blob70k, demo_objs):
    """trace_rays(Camera.rays()) finds the hits the production render kernel finds: C2 at 1920x1080 from its three cameras (the mid
    one also against the oracle), and the demo scene at 1080p."""
    import torch
    W, H = 1920, 1080
    cases = [(sd.blob_scene(scenes, blob70k), pose, name) for name, pose in scenes.C2_CAMERAS.items()]
    cases.append((sd.demo_scene(scenes, demo_objs), scenes.DEMO["cam_pose"], "demo"))
    products = {}
    for desc, pose, name in cases:
        key = id(desc) if name == "demo" else "c2"
        if key not in products:
            sp = desc.build_product(rt)
            sp.upload_to_device()
            products[key] = sp
        sp = products[key]
        cam = _camera(rt, W, H, scenes.scaled_K(W), scenes.D_REF, pose)
        ids = rt.render_ids(sp, cam)
        o, d = cam.rays()
        got = sp.trace_rays(o, d)
        torch.cuda.synchronize()
        assert np.array_equal(got["instance"].cpu().numpy(), ids["hit_inst"]), name
        assert np.array_equal(got["triangle"].cpu().numpy(), ids["hit_tri"]), name
        assert (ids["hit_inst"] >= 0).any(), name
        if name == "mid":
            so = desc.build_oracle(orc)
            ref = ray_oracle.cast_rays(so, o.cpu().numpy(), d.cpu().numpy(), threads=16)
            so.close()
            assert np.array_equal(got["instance"].cpu().numpy(), ref["instance"])
            assert np.array_equal(got["triangle"].cpu().numpy(), ref["triangle"])
            assert np.array_equal(_bits(got["t"].cpu().numpy()), _bits(ref["t"]))


def _exact_uv_scene():
    tris = sd.random_triangles(50, seed=5, spread=0.6, size=0.5)
    tris[::3, 12] = 3.0e38
    tris[1::7, 14] = np.float32(np.finfo(np.float32).max)
    return sd.SceneDesc([((0.8, 0.8, 0.1), None)], [("tris", tris)], [(0, 0, (0,) * 6, (1, 1, 1))])


def _kinds(scenes, blob5k, demo_objs):
    """(name, scene, camera W, H, pose, random-ray box): every scene kind of the parity suite"""
    m = sd.MULTI_CAMERA
    c1 = scenes.C1
    return [("c1", sd.c1_scene(scenes), 256, 256, c1["cam_pose"], (-1.5, 1.5)),
            ("blob5k", sd.blob_scene(scenes, blob5k), 320, 180, scenes.C2_CAMERAS["mid"], (-1.2, 1.2)),
            ("multi", sd.multi_instance_scene(scenes, blob5k), m["width"], m["height"], m["pose"], (-2.0, 2.0)),
            ("demo", sd.demo_scene(scenes, demo_objs), 320, 180, scenes.DEMO["cam_pose"], (-3.0, 3.0)),
            ("exact_uv", _exact_uv_scene(), 160, 120, (0.0, -2.5, 0.0, 0, 0, 0), (-1.0, 1.0)),
            ("deep", sd.deep_stack_scene(28), 96, 64, (0.0, -1.0, 0.0, 0, 0, 0), (-1.0, 1.0))]


def test_all_outputs_equal_oracle(rt, orc, scenes, blob5k, demo_objs):
    """All seven outputs against the oracle's cast_ray on camera rays and on 100 003 random rays per scene kind (origins inside the
    meshes, axis-aligned directions with +-0 components, secondary rays from earlier hit locations); binning on and off."""
    rng = np.random.default_rng(20261015)
    for name, desc, W, H, pose, box in _kinds(scenes, blob5k, demo_objs):
        so = desc.build_oracle(orc)
        sp = desc.build_product(rt)
        sp.upload_to_device()
        K = scenes.C1["K"] if name == "c1" else scenes.scaled_K(W)
        D = scenes.C1["D"] if name == "c1" else scenes.D_REF
        o, d = _flat(*_camera(rt, W, H, K, D, pose).rays(as_numpy=True))
        ref = ray_oracle.cast_rays(so, o, d, threads=16)
        assert (ref["instance"] >= 0).any(), name
        if name == "deep":
            assert ref["pops"].max() > 28                       # rays that walk the whole chain (the LDS part of the stack holds 16)
        if name in ("demo", "multi"):
            assert (ref["uv"] != 0).any()
        for binning in (False, True):
            _same(sp.trace_rays(o, d, outputs=ALL, binning=binning), ref, where="%s camera binning=%s" % (name, binning))
        perm = rng.permutation(len(o))
        _same(sp.trace_rays(o[perm], d[perm], outputs=ALL, binning=True), {k: v[perm] for k, v in ref.items()}, where=name + " shuffled")
        hits = ref["location"][ref["instance"] >= 0]
        ro, rd = _random_rays(rng, 100003, box[0], box[1], hits)
        rref = ray_oracle.cast_rays(so, ro, rd, threads=16)
        for binning in (False, True):
            _same(sp.trace_rays(ro, rd, outputs=ALL, binning=binning), rref, where="%s random binning=%s" % (name, binning))
        # occlusion with per-ray bounds: random, 0, FLT_MAX and +inf mixed
        tmax = rng.uniform(0.0, 3.0, len(ro)).astype(np.float32)
        tmax[::5] = 0.0
        tmax[1::5] = FLT_MAX
        tmax[2::5] = np.inf
        oref = ray_oracle.cast_rays(so, ro, rd, lighting_pass=1, tmax=tmax, threads=16)["occluded"]
        for binning in (False, True):
            got = sp.occluded(ro, rd, tmax, binning=binning)
            assert got.dtype == np.uint8 and np.array_equal(got, oref), (name, binning, np.flatnonzero(got != oref)[:5])
        assert np.array_equal(sp.occluded(ro, rd), ray_oracle.cast_rays(so, ro, rd, lighting_pass=1, threads=16)["occluded"]), name
        so.close()
        sp.close()


def test_edge_sizes(rt, orc, scenes, blob5k):
    """n = 0 launches nothing and returns OK, n = 1 works, 16 M rays in one call (t only, spot-checked)."""
    import ctypes as C
    import torch
    desc = sd.blob_scene(scenes, blob5k)
    sp = desc.build_product(rt)
    sp.upload_to_device()
    h = rt.libs()[0]
    hits = rt.RtRayHits()
    assert h.rt_trace_rays(sp.device_handle, None, None, 0, C.byref(hits), None, 0, None, 1) == 0
    assert h.rt_occluded(sp.device_handle, None, None, None, 0, None, None, 0, None, 1) == 0
    assert h.rt_trace_rays(sp.device_handle, None, None, -1, C.byref(hits), None, 0, None, 1) == -1
    e = np.zeros((0, 3), np.float32)
    assert sp.trace_rays(e, e)["t"].shape == (0,)
    so = desc.build_oracle(orc)
    o = np.array([[0.0, -1.6, 0.2]], np.float32)
    d = np.array([[0.0, 1.0, 0.0]], np.float32)
    _same(sp.trace_rays(o, d, outputs=ALL), ray_oracle.cast_rays(so, o, d), where="n=1")
    n = 1 << 24
    g = torch.Generator(device="cuda").manual_seed(5)
    to = (torch.rand((n, 3), device="cuda", generator=g) * 2.4 - 1.2).contiguous()
    td = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=g), dim=1).contiguous()
    t = sp.trace_rays(to, td, outputs=("t",))["t"]
    torch.cuda.synchronize()
    idx = np.random.default_rng(1).choice(n, 20000, replace=False)
    ref = ray_oracle.cast_rays(so, to[idx].cpu().numpy(), td[idx].cpu().numpy(), threads=16)
    assert np.array_equal(_bits(t[idx].cpu().numpy()), _bits(ref["t"]))
    assert (ref["t"] < FLT_MAX).any()
    so.close()
    sp.close()


def test_queries_follow_scene_updates(rt, scenes, blob5k):
    """After update_mesh_instance, refit_mesh and rebuild_mesh, trace_rays(Camera.rays()) still finds the render kernel's hits."""
    import torch
    desc = sd.multi_instance_scene(scenes, blob5k)
    sp = desc.build_product(rt)
    sp.upload_to_device()
    m = sd.MULTI_CAMERA
    cam = _camera(rt, m["width"], m["height"], scenes.scaled_K(m["width"]), scenes.D_REF, m["pose"])

    def check(what):
        ids = rt.render_ids(sp, cam)
        o, d = cam.rays()
        got = sp.trace_rays(o, d)
        torch.cuda.synchronize()
        assert np.array_equal(got["instance"].cpu().numpy(), ids["hit_inst"]), what
        assert np.array_equal(got["triangle"].cpu().numpy(), ids["hit_tri"]), what

    check("upload")
    sp.update_mesh_instance(0, 0, 2, (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, 0.8, 1.2))
    check("update_mesh_instance")
    tris = desc.meshes[1][1].copy()
    tris[:, [0, 3, 6]] += 0.05
    tris[:, [2, 5, 8]] -= 0.03
    sp.refit_mesh(1, tris)
    check("refit_mesh")
    sp.rebuild_mesh(1, sd.random_triangles(200, seed=12, spread=0.8, size=0.3))
    check("rebuild_mesh")
    sp.close()


def test_torch_queries_on_streams_overlap_a_render(rt, scenes, blob5k):
    """The torch path enqueues without a synchronise: two queries on two torch streams run beside a render on a third, and every result
    equals the sequential one."""
    import torch
    desc = sd.blob_scene(scenes, blob5k)
    sp = desc.build_product(rt)
    sp.upload_to_device()
    cam = _camera(rt, 640, 360, scenes.scaled_K(640), scenes.D_REF, scenes.C2_CAMERAS["mid"])
    o, d = cam.rays()
    g = torch.Generator(device="cuda").manual_seed(9)
    ro = (torch.rand((300007, 3), device="cuda", generator=g) * 2.4 - 1.2).contiguous()
    rd = torch.nn.functional.normalize(torch.randn((300007, 3), device="cuda", generator=g), dim=1).contiguous()
    torch.cuda.synchronize()
    seq_a = {k: v.cpu() for k, v in sp.trace_rays(o, d, outputs=ALL).items()}
    seq_b = sp.occluded(ro, rd).cpu()
    ids = rt.render_ids(sp, cam)
    img = rt.DeviceBuffer(width_bytes=640 * 3, height=360)
    sa, sb, sc = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(sa):
        a = sp.trace_rays(o, d, outputs=ALL)
    b = sp.occluded(ro, rd, stream=sb)
    h = rt.libs()[0]
    assert h.rt_render(sp.device_handle, cam.params(), img.ptr, img.pitch, sc.cuda_stream, 0) == 0
    torch.cuda.synchronize()
    for k in ALL:
        assert torch.equal(a[k].cpu(), seq_a[k]), k
    assert torch.equal(b.cpu(), seq_b)
    assert np.array_equal(img.to_host().reshape(360, 640, 3), ids["img"])
    img.free()
    sp.close()
