"""G-buffer frames on the GPU (rt_render_gbuffer through Camera.render_gbuffer and through the C ABI): every plane bit for bit against
the CPU oracle -- ray_oracle's camera_ray + cast_ray_lp per pixel, `depth` through tests/gbuffer_oracle.c -- and, on one scene, against
Scene.trace_rays(Camera.rays()) and rt_render_ids on the GPU.  Frames are a few 8x8 tiles large: what can go wrong is tile and frame
indexing, the launch form (direction table, view records, plain records; both stack forms and the retrace) and the plane selection, not
the frame's size.  A test that names a launch form asserts, through view_stats() / dir_table_stats() / loop_stats(), that it was taken.
(tests/conftest.py sets RT_VIEW_MIN_RAYS=0: launches of four frames and more take view records however small the frame.)"""
import ctypes as C
import threading

import numpy as np
import pytest

import gbuffer_oracle
import scene_defs as sd
from test_gpu_dir_table import TURNED, _path
from test_gpu_ray_query import _exact_uv_scene

pytestmark = pytest.mark.gpu
FLT_MAX = np.finfo(np.float32).max
ALL = gbuffer_oracle.PLANES
WIDTH = dict(t=1, depth=1, instance=1, triangle=1, location=3, normal=3, uv=2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, ref, keys=ALL, where=""):
    for k in keys:
        g, r = got[k], ref[k]
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert g.shape == r.shape and g.dtype == r.dtype, (k, g.shape, r.shape, g.dtype, where)
        bad = np.argwhere(_bits(g) != _bits(r))
        assert bad.size == 0, "%s %s: %d values differ, first at %s: got %s want %s" % (where, k, len(bad), bad[0], g[tuple(bad[0])], r[tuple(bad[0])])


def _nine_scene():
    """nine instances of one small mesh (more than kMaxViewInstances = 8: no view records), spread over the view, each posed"""
    tris = sd.random_triangles(60, seed=21, spread=0.5, size=0.35)
    inst = [(0, 0, (-2.0 + 0.5 * k, 0.3 * (k % 3), -0.6 + 0.15 * k, 0.2 * k, -0.1 * k, 0.05 * k), (1.0 + 0.05 * k, 0.9, 1.1)) for k in range(9)]
    return sd.SceneDesc([((0.7, 0.6, 0.2), sd.checker_texture(16, 16, seed=2))], [("tris", tris)], inst)


class World:
    """the scenes of this module, each built once on the oracle and on the product, and the oracle frames computed so far"""

    def __init__(self, rt, orc, scenes, demo_objs, blob5k):
        self.rt, self.orc, self.scenes = rt, orc, scenes
        self.make = dict(demo=lambda: sd.demo_scene(scenes, demo_objs), turned=lambda: self._turned(demo_objs),
                         multi=lambda: sd.multi_instance_scene(scenes, blob5k), c1=lambda: sd.c1_scene(scenes), exact_uv=_exact_uv_scene,
                         deep=lambda: sd.deep_stack_scene(28), nine=_nine_scene)
        self.built, self.refs = {}, {}

    def _turned(self, demo_objs):
        d = sd.demo_scene(self.scenes, demo_objs)
        d.instances[1] = (1, 1) + TURNED
        return d

    def get(self, name):
        """(oracle scene, uploaded product scene)"""
        if name not in self.built:
            desc = self.make[name]()
            sp = desc.build_product(self.rt)
            sp.upload_to_device()
            self.built[name] = (desc.build_oracle(self.orc), sp)
        return self.built[name]

    def ref(self, name, w, h, K, D, poses):
        """the oracle's planes [len(poses), h, w](, k); frames are computed once per (scene, camera, pose)"""
        so = self.get(name)[0]
        per = []
        for p in poses:
            key = (name, w, h, tuple(K), tuple(D), tuple(np.float32(p).tolist()))
            if key not in self.refs:
                self.refs[key] = gbuffer_oracle.frame(so, w, h, K, D, p)
            per.append(self.refs[key])
        return {k: np.stack([f[k] for f in per]) for k in ALL}

    def close(self):
        for so, sp in self.built.values():
            so.close()
            sp.close()


@pytest.fixture(scope="module")
def world(rt, orc, scenes, demo_objs, blob5k):
    w = World(rt, orc, scenes, demo_objs, blob5k)
    yield w
    w.close()


def _views(world, name, n):
    """(w, h, K, D, n poses) of scene `name`'s parity camera"""
    sc = world.scenes
    if name in ("demo", "turned"):
        return 40, 24, sc.scaled_K(40), sc.D_REF, _path(32)[:n] if n <= 32 else _path(n)
    if name == "multi":
        m = sd.MULTI_CAMERA["pose"]
        return 40, 24, sc.scaled_K(40), sc.D_REF, [(m[0] + 0.02 * i, m[1] + 0.03 * i, m[2] - 0.01 * i, m[3] - 0.01 * i, m[4], m[5] + 0.005 * i) for i in range(n)]
    if name == "c1":                                                    # (C1's camera at 32 x 32: the principal point stays on a pixel centre)
        c = sc.C1["cam_pose"]
        return 32, 32, (30.0, 0, 16.0, 0, 30.0, 16.0, 0, 0, 1.0), sc.C1["D"], [(c[0] + 0.05 * i, c[1] + 0.1 * i, c[2], 0.02 * i, 0.0, 0.0) for i in range(n)]
    if name == "exact_uv":
        return 40, 30, sc.scaled_K(40), sc.D_REF, [(0.02 * i, -2.5, 0.01 * i, 0.0, 0.0, 0.0) for i in range(n)]
    if name == "deep":                                                  # central pixels: the rays that walk the whole chain
        return 32, 24, sc.scaled_K(32), sc.D_REF, [(0.0005 * i, -1.0, 0.0, 0.0, 0.0, 0.0) for i in range(n)]
    if name == "nine":
        return 40, 24, sc.scaled_K(40), sc.D_REF, [(0.03 * i, -3.5, 0.1, 0.01 * i, 0.0, 0.0) for i in range(n)]
    raise KeyError(name)


def _camera(rt, w, h, K, D, pose=None):
    cam = rt.Camera(w, h, K, D)
    if pose is not None:
        cam.set_pose(pose)
    return cam


def _render(world, name, w, h, K, D, poses, outputs=ALL, image=False, stream=None):
    cam = _camera(world.rt, w, h, K, D)
    try:
        return cam.render_gbuffer(world.get(name)[1], poses, outputs=outputs, image=image, stream=stream)
    finally:
        cam.close()


def _stats(sp):
    v, d = sp.view_stats(), sp.dir_table_stats()
    return dict(view=v["launches"] - v["fallbacks"], asked=v["launches"], table=d["launches"], no_table=d["skipped"])


def _delta(sp, before):
    now = _stats(sp)
    return {k: now[k] - before[k] for k in now}


def _cams(rt, w, h, K, D, poses):
    cam = rt.Camera(w, h, K, D)
    out = (rt.RtCameraParams * len(poses))()
    for i, ps in enumerate(poses):
        cam.set_pose(ps)
        out[i] = cam.params()
    cam.close()
    return out


def _handle(sp):
    h = sp.device_handle
    return h if isinstance(h, C.c_void_p) else C.c_void_p(h)


GUARD = 64                                                              # guard words before and after every plane


class Planes:
    """device planes for a direct rt_render_gbuffer call, each between two runs of GUARD sentinel words"""

    def __init__(self, rt, n, h, w, names, image=False, stream=None):
        import torch
        self.torch, self.n, self.h, self.w, self.names = torch, n, h, w, tuple(names)
        with torch.cuda.stream(stream):
            self.buf = {k: torch.full((n * h * w * WIDTH[k] + 2 * GUARD,), -559038737, dtype=torch.int32, device="cuda") for k in self.names}
            self.img = torch.full((n * h * w * 3 + 2 * GUARD,), 0xCD, dtype=torch.uint8, device="cuda") if image else None
        self.struct = rt.RtGBuffer(**{k: self.buf[k].data_ptr() + 4 * GUARD for k in self.names})
        self.ptrs = (C.c_void_p * n)(*[self.img.data_ptr() + GUARD + i * h * w * 3 for i in range(n)]) if image else None

    def results(self):
        """dict of numpy planes (and "image"); asserts every guard word is intact"""
        out = {}
        for k in self.names:
            a = self.buf[k].cpu().numpy()
            assert (a[:GUARD] == -559038737).all() and (a[-GUARD:] == -559038737).all(), "guard words of %s" % k
            body = a[GUARD:-GUARD]
            shape = (self.n, self.h, self.w) + ((WIDTH[k],) if WIDTH[k] > 1 else ())
            out[k] = (body if k in ("instance", "triangle") else body.view(np.float32)).reshape(shape).copy()
        if self.img is not None:
            a = self.img.cpu().numpy()
            assert (a[:GUARD] == 0xCD).all() and (a[-GUARD:] == 0xCD).all(), "guard bytes of the images"
            out["image"] = a[GUARD:-GUARD].reshape(self.n, self.h, self.w, 3).copy()
        return out


def _call(rt, sp, cams, planes, stream=None, synchronize=1):
    n, w = len(cams), cams[0].width
    rt.check(rt.libs()[0].rt_render_gbuffer(_handle(sp), cams, n, planes.ptrs, w * 3, C.byref(planes.struct), stream, synchronize), "rt_render_gbuffer")


def _rt_render(rt, sp, cp):
    """the frame of one camera through rt_render"""
    import torch
    img = torch.empty((cp.height, cp.width, 3), dtype=torch.uint8, device="cuda")
    rt.check(rt.libs()[0].rt_render(_handle(sp), C.byref(cp), C.c_void_p(img.data_ptr()), C.c_size_t(cp.width * 3), None, 1), "rt_render")
    return img.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- oracle parity

@pytest.mark.parametrize("name", ["demo", "turned", "multi", "c1"])
def test_every_plane_equals_the_oracle(world, name):
    """Four frames (the table form) and the first of them alone (plain records), every plane.  The coverage condition is the ORACLE's:
    each frame of demo / turned / multi has at least 10 % hit pixels and 10 % misses, turned and multi hit two instances per frame."""
    w, h, K, D, poses = _views(world, name, 4)
    ref = world.ref(name, w, h, K, D, poses)
    hit = ref["instance"] >= 0
    if name != "c1":
        frac = hit.reshape(4, -1).mean(axis=1)
        assert (frac >= 0.1).all() and (frac <= 0.9).all(), frac
        assert (ref["uv"] != 0).any() and (ref["depth"][hit] != ref["t"][hit]).any()
    else:
        assert hit.any() and not hit.all()
    if name in ("turned", "multi"):
        assert all(len(np.unique(ref["instance"][i][hit[i]])) >= 2 for i in range(4))
    assert (ref["depth"][~hit] == FLT_MAX).all() and (ref["location"][~hit] == 0).all()
    sp = world.get(name)[1]
    before = _stats(sp)
    _same(_render(world, name, w, h, K, D, poses), ref, where=name + " x4")
    # (c1's tree is one leaf: a scene without interior records has no view records to write, and renders four frames as it renders one)
    assert _delta(sp, before) == (dict(view=1, asked=1, table=1, no_table=0) if name != "c1" else dict(view=0, asked=0, table=0, no_table=0))
    before = _stats(sp)
    _same(_render(world, name, w, h, K, D, poses[:1]), {k: v[:1] for k, v in ref.items()}, where=name + " x1")
    assert _delta(sp, before) == dict(view=0, asked=0, table=0, no_table=0)


def test_planes_equal_trace_rays_and_render_ids_on_the_gpu(world):
    """the detour this call replaces, on the GPU: Scene.trace_rays(Camera.rays()) for every plane it has, rt_render_ids for the ids"""
    import torch
    rt = world.rt
    w, h, K, D, poses = _views(world, "turned", 4)
    sp = world.get("turned")[1]
    got = _render(world, "turned", w, h, K, D, poses)
    for i in (0, 3):
        cam = _camera(rt, w, h, K, D, poses[i])
        o, d = cam.rays()
        q = sp.trace_rays(o, d, outputs=("t", "instance", "triangle", "location", "normal", "uv"))
        torch.cuda.synchronize()
        for k, v in q.items():
            assert torch.equal(got[k][i].view(torch.int32), v.view(torch.int32)), (k, i)
        ids = rt.render_ids(sp, cam)
        assert np.array_equal(got["instance"][i].cpu().numpy(), ids["hit_inst"]) and np.array_equal(got["triangle"][i].cpu().numpy(), ids["hit_tri"])
        cam.close()


# ---------------------------------------------------------------------------------------------------------------- launch forms

def test_frames_with_two_intrinsics_take_view_records_without_a_table(world):
    """frames 0, 2 with one K and frames 1, 3 with another (zoomed, principal point moved): view records, no direction table"""
    rt, sc = world.rt, world.scenes
    w, h, K, D, poses = _views(world, "turned", 4)
    K2 = list(K)
    K2[0] *= 1.3; K2[4] *= 1.3; K2[2] += 1.25; K2[5] -= 0.5
    K2 = tuple(K2)
    a, b = _cams(rt, w, h, K, D, poses), _cams(rt, w, h, K2, D, poses)
    cams = (rt.RtCameraParams * 4)(a[0], b[1], a[2], b[3])
    ra, rb = world.ref("turned", w, h, K, D, poses), world.ref("turned", w, h, K2, D, poses)
    ref = {k: np.stack([ra[k][0], rb[k][1], ra[k][2], rb[k][3]]) for k in ALL}
    assert not np.array_equal(ra["instance"][1], rb["instance"][1])
    sp = world.get("turned")[1]
    planes = Planes(rt, 4, h, w, ALL)
    before = _stats(sp)
    _call(rt, sp, cams, planes)
    assert _delta(sp, before) == dict(view=1, asked=1, table=0, no_table=1)
    _same(planes.results(), ref, where="two intrinsics")


def test_nine_instances_render_without_view_records(world):
    w, h, K, D, poses = _views(world, "nine", 4)
    ref = world.ref("nine", w, h, K, D, poses)
    assert len(np.unique(ref["instance"])) >= 5 and (ref["instance"] < 0).any()
    sp = world.get("nine")[1]
    before = _stats(sp)
    _same(_render(world, "nine", w, h, K, D, poses), ref, where="nine instances")
    assert _delta(sp, before) == dict(view=0, asked=0, table=0, no_table=0)


@pytest.mark.parametrize("count", [1, 4])
def test_deep_tree_takes_the_optimistic_stack_and_the_retrace(world, count):
    """deep_stack_scene at central pixels: a tree deeper than the LDS part of the stack (the SPILL instantiations: optimistic stack,
    then the general stack for the lanes that outgrew it), as plain records (one frame) and through view records and the table (four).
    That these very frames retrace lanes is what rt_scene_loop_stats says of them; the oracle's pop counts say why."""
    import torch
    rt = world.rt
    w, h, K, D, poses = _views(world, "deep", count)
    so, sp = world.get("deep")
    import ray_oracle
    pops = ray_oracle.cast_rays(so, *ray_oracle.camera_rays(w, h, K, D, poses[0]))["pops"]
    assert pops.max() > 28
    img = torch.empty((count, h, w, 3), dtype=torch.uint8, device="cuda")
    cam = _camera(rt, w, h, K, D)
    st = rt.Scene.loop_stats(sp, cam, poses, [img[i].data_ptr() for i in range(count)], w * 3)
    cam.close()
    assert st["retraced_lanes"] > 0 and st["deep"] > 0, st
    ref = world.ref("deep", w, h, K, D, poses)
    assert (ref["instance"] >= 0).any() and (ref["instance"] < 0).any()
    before = _stats(sp)
    got = _render(world, "deep", w, h, K, D, poses, image=True)
    assert _delta(sp, before) == (dict(view=1, asked=1, table=1, no_table=0) if count == 4 else dict(view=0, asked=0, table=0, no_table=0))
    _same(got, ref, where="deep x%d" % count)
    assert torch.equal(got["image"], img)


# ---------------------------------------------------------------------------------------------------------------- shapes

@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (9, 7), (64, 1), (1, 64), (17, 23)])
def test_frame_sizes(world, w, h):
    """one pixel, one tile, ragged tiles, one row and one column of eight tiles, 3 x 3 ragged tiles: four frames each, every plane"""
    sc = world.scenes
    K = list(sc.scaled_K(max(w, h, 16)))
    K[2], K[5] = w / 2.0 + 0.25, h / 2.0 - 0.25
    poses = _path(32)[10:14]
    ref = world.ref("turned", w, h, K, sc.D_REF, poses)
    assert (ref["instance"] >= 0).any()
    if min(w, h) >= 7:
        assert (ref["instance"] < 0).any()
    _same(_render(world, "turned", w, h, K, sc.D_REF, poses), ref, where="%d x %d" % (w, h))


@pytest.mark.parametrize("count", [1, 2, 3, 32])
def test_frame_counts(world, count):
    sc = world.scenes
    w, h, K = 17, 23, sc.scaled_K(17)
    poses = _path(32)[:count]
    ref = world.ref("demo", w, h, K, sc.D_REF, poses)
    sp = world.get("demo")[1]
    before = _stats(sp)
    _same(_render(world, "demo", w, h, K, sc.D_REF, poses), ref, where="%d frames" % count)
    assert _delta(sp, before)["table"] == (1 if count == 32 else 0)


def test_thirty_three_poses_are_two_launches(world):
    sc = world.scenes
    w, h, K = 17, 23, sc.scaled_K(17)
    poses = _path(33)
    ref = world.ref("demo", w, h, K, sc.D_REF, poses)
    assert len({ref["t"][i].tobytes() for i in range(33)}) == 33
    sp = world.get("demo")[1]
    before = _stats(sp)
    got = _render(world, "demo", w, h, K, sc.D_REF, poses, image=True)
    assert _delta(sp, before) == dict(view=1, asked=1, table=1, no_table=0)     # (32 frames with a table, then one frame alone)
    _same(got, ref, where="33 poses")
    assert tuple(got["image"].shape) == (33, h, w, 3)
    cams = _cams(world.rt, w, h, K, sc.D_REF, [poses[0], poses[32]])
    img = got["image"].cpu().numpy()
    assert np.array_equal(img[0], _rt_render(world.rt, sp, cams[0])) and np.array_equal(img[32], _rt_render(world.rt, sp, cams[1]))


# ---------------------------------------------------------------------------------------------------------------- plane selection

@pytest.fixture(scope="module")
def selection(world):
    """the turned scene's four parity frames: cameras, oracle planes, rt_render's bytes per pose"""
    w, h, K, D, poses = _views(world, "turned", 4)
    sp = world.get("turned")[1]
    cams = _cams(world.rt, w, h, K, D, poses)
    return dict(w=w, h=h, cams=cams, ref=world.ref("turned", w, h, K, D, poses), sp=sp, frames=np.stack([_rt_render(world.rt, sp, cams[i]) for i in range(4)]))


@pytest.mark.parametrize("names,image", [((k,), False) for k in ALL] + [(ALL, False), (ALL, True), ((), True), (("depth", "uv"), True)])
def test_plane_selection_and_guard_words(world, selection, names, image):
    """every plane alone, all together, images with and without planes: what is asked for is the oracle's (the images rt_render's),
    and nothing is written outside it"""
    s = selection
    planes = Planes(world.rt, 4, s["h"], s["w"], names, image)
    _call(world.rt, s["sp"], s["cams"], planes)
    got = planes.results()
    _same(got, s["ref"], keys=names, where=str(names))
    if image:
        assert np.array_equal(got["image"], s["frames"])
        assert len(np.unique(got["image"].reshape(-1, 3), axis=0)) > 8                # textures on screen


def test_a_frame_of_a_batch_equals_the_frame_alone(world, selection):
    s = selection
    rt = world.rt
    batch = Planes(rt, 4, s["h"], s["w"], ALL, True)
    _call(rt, s["sp"], s["cams"], batch)
    got = batch.results()
    for i in range(4):
        one = Planes(rt, 1, s["h"], s["w"], ALL, True)
        _call(rt, s["sp"], (rt.RtCameraParams * 1)(s["cams"][i]), one)
        alone = one.results()
        for k in ALL + ("image",):
            assert np.array_equal(_bits(got[k][i]), _bits(alone[k][0])), (k, i)


def test_exact_uv_mesh(world):
    """a mesh in the exact-uv mode (uv data that could reach FLT_MAX: the hit carries the interpolated uv itself)"""
    w, h, K, D, poses = _views(world, "exact_uv", 4)
    ref = world.ref("exact_uv", w, h, K, D, poses)
    hit = ref["instance"] >= 0
    assert hit.any() and (~hit).any() and (np.abs(ref["uv"][hit]) > 1e30).any()
    _same(_render(world, "exact_uv", w, h, K, D, poses), ref, where="exact uv x4")
    _same(_render(world, "exact_uv", w, h, K, D, poses[:1]), {k: v[:1] for k, v in ref.items()}, where="exact uv x1")


# ---------------------------------------------------------------------------------------------------------------- streams and updates

@pytest.mark.parametrize("raw", [False, True])
def test_a_non_finite_pose_between_finite_frames(world, raw):
    """frame 1 of four has a NaN and an infinity in its pose: no fault, frames 0, 2 and 3 are what they are without it -- on a torch
    stream and on its raw handle"""
    import torch
    w, h, K, D, poses = _views(world, "turned", 4)
    ref = world.ref("turned", w, h, K, D, poses)
    bad = list(poses)
    bad[1] = (float("nan"), poses[1][1], float("inf"), poses[1][3], float("nan"), 0.0)
    stream = torch.cuda.Stream()
    got = _render(world, "turned", w, h, K, D, bad, image=True, stream=stream.cuda_stream if raw else stream)
    stream.synchronize()
    keep = [0, 2, 3]
    _same({k: got[k][keep] for k in ALL}, {k: v[keep] for k, v in ref.items()}, where="beside a non-finite pose")
    sp = world.get("turned")[1]
    cams = _cams(world.rt, w, h, K, D, poses)
    img = got["image"].cpu().numpy()
    for i in keep:
        assert np.array_equal(img[i], _rt_render(world.rt, sp, cams[i])), i


def test_two_streams_in_flight_on_one_scene(world):
    """two threads, a stream each, six launches each of four and of one frame with no wait in between: every result equals the serial one"""
    import torch
    w, h, K, D, poses = _views(world, "turned", 8)
    ref = world.ref("turned", w, h, K, D, poses)
    jobs = [(torch.cuda.Stream(), [0, 1, 2, 3]), (torch.cuda.Stream(), [4, 5, 6, 7])]
    torch.cuda.synchronize()
    go, out, errors = threading.Barrier(2), [None, None], []

    def worker(k):
        try:
            stream, idx = jobs[k]
            go.wait(60)
            res = []
            for r in range(6):
                sel = idx if r % 2 == 0 else idx[r % 4:r % 4 + 1]
                res.append((sel, _render(world, "turned", w, h, K, D, [poses[i] for i in sel], stream=stream)))
            stream.synchronize()
            out[k] = res
        except Exception as e:                                          # noqa: BLE001 (reported below, on the main thread)
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for k in range(2):
        for sel, got in out[k]:
            _same(got, {key: v[sel] for key, v in ref.items()}, where="stream %d frames %s" % (k, sel))


def test_frames_follow_scene_updates(rt, orc, scenes, blob5k):
    """after update_mesh_instance and after refit_mesh a frame equals the oracle of the scene as it is now"""
    desc = sd.multi_instance_scene(scenes, blob5k)
    sp = desc.build_product(rt)
    sp.upload_to_device()
    m = sd.MULTI_CAMERA["pose"]
    w, h, K, D = 40, 24, scenes.scaled_K(40), scenes.D_REF
    poses = [(m[0] + 0.02 * i,) + tuple(m[1:]) for i in range(4)]
    cam = _camera(rt, w, h, K, D)

    def check(what, n):
        so = desc.build_oracle(orc)
        ref = gbuffer_oracle.frames(so, w, h, K, D, poses[:n])
        so.close()
        assert (ref["instance"] >= 0).any()
        _same(cam.render_gbuffer(sp, poses[:n], outputs=ALL), ref, where=what)
        return ref

    first = check("upload", 4)
    pose, scale = (0.4, 0.2, 0.0, -0.3, 0.2, 0.5), (0.9, 0.8, 1.2)
    sp.update_mesh_instance(0, 0, 2, pose, scale)
    desc.instances[0] = (0, 2, pose, scale)
    second = check("update_mesh_instance", 4)
    assert not np.array_equal(first["t"], second["t"])
    tris = desc.meshes[1][1].copy()
    tris[:, [0, 3, 6]] += 0.05
    tris[:, [2, 5, 8]] -= 0.03
    sp.refit_mesh(1, tris)
    desc.meshes[1] = ("tris", tris)
    third = check("refit_mesh", 1)
    assert not np.array_equal(second["t"][:1], third["t"])
    check("refit_mesh x4", 4)
    cam.close()
    sp.close()
