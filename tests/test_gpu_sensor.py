"""Sensor frames on the GPU (rt_render_gbuffer_table through Sensor.render_gbuffer and through the C ABI).
1. The pinhole anchor: Sensor(Camera.directions()) against Camera on the GPU, bit for bit -- rays, all seven planes, the image -- in
   every launch form: plain records + table (1, 3 frames: the new kernel forms), view records + table (4, 32), two launches (33), a
   scene that never gets a view slot (nine instances) and the spill stack form with its retrace (deep).
2. Tables that are no pinhole -- a panorama, a spinning lidar, entries of other lengths, exact axis directions -- from a sensor
   INSIDE the scene, every plane bit for bit against the CPU oracle (tests/sensor_oracle.py) and against
   Scene.trace_rays(Sensor.rays()) on the GPU.
3. Plane selection, images alone, the sky colour; 4. non-finite and all-zero entries beside finite ones; 5. one table on two
   threads, two streams and two scenes; 6. the C ABI with ctypes alone.
Frames are a few 8x8 tiles large: what can go wrong is tile and lane indexing, ragged edges, the launch form and frame indexing.  A test
that names a launch form asserts through view_stats() that it was taken, and through dir_table_stats() that the library's own
direction tables were neither written nor counted.  (tests/conftest.py sets RT_VIEW_MIN_RAYS=0: four frames take view records.)"""
import ctypes as C
import importlib
import math
import threading

import numpy as np
import pytest

import sensor_oracle
from test_gpu_gbuffer import ALL, Planes, World, _bits, _handle, _same, _stats, _delta, _views

pytestmark = pytest.mark.gpu
SKY = (255, 204, 153)                                                   # raycast.cu:208-216, as the kernels store it
INSIDE = (-0.4, 0.8, 0.8)                                               # a sensor position between the demo scene's two meshes


@pytest.fixture(scope="module")
def world(rt, orc, scenes, demo_objs, blob5k):
    w = World(rt, orc, scenes, demo_objs, blob5k)
    yield w
    w.close()


@pytest.fixture(scope="module")
def sensors():
    return importlib.import_module("cuda-raytracing_amd.sensors")


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _equal(got, ref, keys, where):
    got, ref = _np(got), _np(ref)
    for k in keys:
        assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, (k, where)
        bad = np.argwhere(_bits(got[k]) != _bits(ref[k]))
        assert bad.size == 0, "%s %s: %d values differ, first at %s" % (where, k, len(bad), bad[0])


# ---------------------------------------------------------------------------------------------------------------- 1. the pinhole anchor

def _anchor_camera(world, name, ragged):
    """(w, h, K, D, pose maker) of the scene's parity camera; ragged: 37 x 21 of the same intrinsics (ragged in both axes)"""
    w, h, K, D, _p = _views(world, name, 1)
    if ragged:
        w, h = 37 if w >= 37 else 29, 21 if h >= 21 else 19
    return w, h, K, D


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("name", ["demo", "turned", "nine", "deep"])
def test_pinhole_table_equals_the_camera(world, name, ragged):
    import torch
    rt = world.rt
    w, h, K, D = _anchor_camera(world, name, ragged)
    sp = world.get(name)[1]
    cam = rt.Camera(w, h, K, D)
    sensor = rt.Sensor(cam.directions())
    assert (sensor.width, sensor.height) == (w, h)
    poses33 = _views(world, name, 33)[4]
    try:
        cam.set_pose(poses33[2])
        co, cd = cam.rays()
        so, sd_ = sensor.rays(poses33[2])
        assert torch.equal(co.view(torch.int32), so.view(torch.int32)) and torch.equal(cd.view(torch.int32), sd_.view(torch.int32))
        views = name != "nine"                                          # (nine instances: more than kMaxViewInstances, never a view slot)
        for count in (1, 3, 4, 32, 33):
            poses = poses33[:count]
            want = cam.render_gbuffer(sp, poses, outputs=ALL, image=True)
            before = _stats(sp)
            got = sensor.render_gbuffer(sp, poses, outputs=ALL, image=True)
            form = _delta(sp, before)
            taken = 1 if (views and count >= 4) else 0                  # (33 = 32 through view records, then one frame of plain records)
            assert form == dict(view=taken, asked=taken, table=0, no_table=0), (name, count, form)
            _equal(got, want, ALL + ("image",), "%s %dx%d x%d" % (name, w, h, count))
            if count == 4:
                hit = got["instance"].cpu().numpy() >= 0
                assert hit.any() and (name == "nine" or (~hit).any())
    finally:
        sensor.close()
        cam.close()


def test_deep_tree_retraces_lanes_under_a_table(world):
    """the frames of the anchor above on the deep scene do take the optimistic stack and retrace lanes: rt_scene_loop_stats of the
    same camera and poses says so (the table changes no ray)"""
    import torch
    rt = world.rt
    w, h, K, D, poses = _views(world, "deep", 1)
    sp = world.get("deep")[1]
    cam = rt.Camera(w, h, K, D)
    img = torch.empty((1, h, w, 3), dtype=torch.uint8, device="cuda")
    st = rt.Scene.loop_stats(sp, cam, poses, [img[0].data_ptr()], w * 3)
    cam.close()
    assert st["retraced_lanes"] > 0 and st["deep"] > 0, st


# ---------------------------------------------------------------------------------------------------------------- 2. other tables

def _axes_table():
    """16 x 8: the six exact axis directions, vectors with two zero components of other lengths, every vector with one zero component
    and equal other two, and a fan of general directions"""
    rng = np.random.default_rng(11)
    d = rng.normal(size=(8, 16, 3)).astype(np.float32)
    special = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (2.5, 0, 0), (0, -0.001, 0), (0, 0, 7.0)]
    special += [(a, b, 0) for a in (1, -1) for b in (1, -1)] + [(a, 0, b) for a in (1, -1) for b in (1, -1)] + [(0, a, b) for a in (1, -1) for b in (1, -1)]
    flat = d.reshape(-1, 3)
    flat[np.arange(len(special)) * 5 % 128] = np.array(special, np.float32)     # spread over the tiles and lanes
    return d


def _table(sensors, kind):
    if kind in ("equirectangular", "turned"):
        return sensors.equirectangular(64, 24)
    if kind == "lidar":
        return sensors.spinning_lidar(np.radians(np.linspace(-25.0, 15.0, 16)), 128)
    if kind == "scaled":
        rng = np.random.default_rng(12)
        return sensors.equirectangular(64, 24) * rng.choice(np.array([1e-3, 1.0, 3.0], np.float32), size=(24, 64, 1))
    if kind == "axes":
        return _axes_table()
    raise KeyError(kind)


def _inside_poses(n, level):
    """n poses inside the demo scene; level: no rotation in frame 0 (axis entries stay axis directions)"""
    x, y, z = INSIDE
    return [(x + 0.05 * i, y - 0.04 * i, z + 0.02 * i, 0.0 if (level and i == 0) else 0.4 + 0.3 * i, 0.0 if (level and i == 0) else -0.15 + 0.05 * i,
             0.0 if (level and i == 0) else 0.1 * i) for i in range(n)]


@pytest.mark.parametrize("kind", ["equirectangular", "lidar", "scaled", "axes", "turned"])
def test_tables_against_the_oracle_and_trace_rays(world, sensors, kind):
    import torch
    rt = world.rt
    name = "turned" if kind == "turned" else "demo"
    so, sp = world.get(name)
    dirs = _table(sensors, kind)
    h, w = dirs.shape[:2]
    poses = _inside_poses(5, kind == "axes")
    ref = sensor_oracle.frames(so, dirs, poses)
    hit = ref["instance"] >= 0
    # the coverage is the ORACLE's: hits in every frame, two instances seen, rays leaving in all eight octants
    assert (hit.reshape(5, -1).mean(axis=1) >= 0.1).all() and len(np.unique(ref["instance"][hit])) >= 2
    o0, d0 = sensor_oracle.rays(dirs, poses[1])
    assert len({tuple(v) for v in (d0.reshape(-1, 3) > 0)}) == 8
    if kind == "axes":
        _o, dl = sensor_oracle.rays(dirs, poses[0])
        zeros = (dl.reshape(-1, 3) == 0).sum(axis=1)
        assert (zeros == 2).sum() >= 9 and (zeros == 1).sum() >= 12
    sensor = rt.Sensor(dirs)
    try:
        for count in (1, 5):
            before = _stats(sp)
            got = sensor.render_gbuffer(sp, poses[:count], outputs=ALL)
            taken = 1 if count >= 4 else 0
            assert _delta(sp, before) == dict(view=taken, asked=taken, table=0, no_table=0)
            _same(got, {k: v[:count] for k, v in ref.items()}, where="%s x%d" % (kind, count))
            for i in {0, count - 1}:
                ro, rd = sensor.rays(poses[i])
                assert np.array_equal(_bits(rd.cpu().numpy()), _bits(sensor_oracle.rays(dirs, poses[i])[1])), (kind, i)
                q = sp.trace_rays(ro, rd, outputs=("t", "instance", "triangle", "location", "normal", "uv"))
                torch.cuda.synchronize()
                for k, v in q.items():
                    assert torch.equal(got[k][i].view(torch.int32), v.view(torch.int32)), (kind, k, i)
    finally:
        sensor.close()


# ---------------------------------------------------------------------------------------------------------------- 3. selection, images

@pytest.fixture(scope="module")
def panorama(world, sensors):
    """a panorama from outside the turned scene, so that some rays miss: the sensor, five poses, the full render of five and of one"""
    rt = world.rt
    sp = world.get("turned")[1]
    sensor = rt.Sensor(sensors.equirectangular(37, 21, azimuth=(-1.2, 1.2), elevation=(-0.7, 0.7)))
    poses = _views(world, "turned", 5)[4]
    full = {n: _np(sensor.render_gbuffer(sp, poses[:n], outputs=ALL, image=True)) for n in (1, 5)}
    yield dict(sensor=sensor, sp=sp, poses=poses, full=full)
    sensor.close()


@pytest.mark.parametrize("count", [1, 5])
@pytest.mark.parametrize("names,image", [((k,), False) for k in ALL] + [((), True), (("depth", "uv"), True), (ALL, False)])
def test_plane_selection_and_images_alone(panorama, names, image, count):
    p = panorama
    got = _np(p["sensor"].render_gbuffer(p["sp"], p["poses"][:count], outputs=names, image=image))
    assert set(got) == set(names) | ({"image"} if image else set())
    _equal(got, p["full"][count], tuple(got), "%s image=%s x%d" % (names, image, count))


def test_the_image_of_a_miss_is_the_sky(panorama):
    for n in (1, 5):
        full = panorama["full"][n]
        miss = full["instance"] < 0
        assert miss.any() and (~miss).any()
        assert (full["image"][miss] == np.array(SKY, np.uint8)).all()
        assert (full["image"][~miss] != np.array(SKY, np.uint8)).any(axis=-1).any()
        assert (full["t"][miss] == np.finfo(np.float32).max).all() and (full["location"][miss] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- 4. bad entries

def test_bad_entries_leave_the_other_pixels_alone(world, sensors):
    """one NaN, one +inf and one all-zero entry among finite ones: RT_OK, every other pixel is what it is with finite entries there, and
    the scene renders correctly afterwards.  (trace_instance keeps such lanes out of the loops by construction; this pins it for tables.)"""
    rt = world.rt
    sp = world.get("demo")[1]
    clean = sensors.equirectangular(64, 24)
    bad = clean.copy()
    spots = [(3, 5), (10, 20), (17, 40)]
    bad[3, 5, 0] = np.nan
    bad[10, 20, 2] = np.inf
    bad[17, 40] = 0.0
    keep = np.ones((24, 64), bool)
    for y, x in spots:
        keep[y, x] = False
    poses = _inside_poses(5, False)
    a, b = rt.Sensor(clean), rt.Sensor(bad)
    try:
        for count in (1, 5):
            want = _np(a.render_gbuffer(sp, poses[:count], outputs=ALL, image=True))
            got = _np(b.render_gbuffer(sp, poses[:count], outputs=ALL, image=True))          # (check() raises unless RT_OK)
            for k in ALL + ("image",):
                assert np.array_equal(_bits(got[k][:, keep]), _bits(want[k][:, keep])), (k, count)
            again = _np(a.render_gbuffer(sp, poses[:count], outputs=ALL, image=True))
            _equal(again, want, ALL + ("image",), "after the bad table x%d" % count)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------- 5. sharing

def test_one_table_on_two_threads_two_streams_and_two_scenes(world, sensors):
    import torch
    rt = world.rt
    scenes_ = [world.get("demo")[1], world.get("turned")[1]]
    maker = torch.cuda.Stream()
    dirs = sensors.equirectangular(37, 21)
    sensor = rt.Sensor(dirs)                                            # (made with synchronize = 1: usable on any stream from here)
    poses = _inside_poses(8, False)
    serial = [[_np(sensor.render_gbuffer(sc, poses[4 * k:4 * k + 4], outputs=ALL, image=True)) for k in range(2)] for sc in scenes_]
    one = [_np(sensor.render_gbuffer(sc, poses[1:2], outputs=ALL, image=True)) for sc in scenes_]
    assert not np.array_equal(serial[0][0]["t"], serial[1][0]["t"])     # (the two scenes differ)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    go, out, errors = threading.Barrier(2), [None, None], []

    def worker(k):
        try:
            go.wait(60)
            res = []
            for r in range(6):
                sc = r % 2                                              # both threads on both scenes, thread k on its own stream
                if r < 4:
                    res.append((sc, k, sensor.render_gbuffer(scenes_[sc], poses[4 * k:4 * k + 4], outputs=ALL, image=True, stream=streams[k])))
                else:
                    res.append((sc, None, sensor.render_gbuffer(scenes_[sc], poses[1:2], outputs=ALL, image=True, stream=streams[k])))
            streams[k].synchronize()
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
        for sc, part, got in out[k]:
            _equal(got, serial[sc][part] if part is not None else one[sc], ALL + ("image",), "thread %d scene %d" % (k, sc))
    # a table made on one stream (with synchronize = 1) and read on another
    h = rt.libs()[0]
    with torch.cuda.stream(maker):
        d = torch.from_numpy(dirs).to("cuda")
    table = C.c_void_p()
    rt.check(h.rt_ray_table_create(C.c_void_p(d.data_ptr()), 37, 21, C.c_void_p(maker.cuda_stream), 1, C.byref(table)), "rt_ray_table_create")
    del d
    cams = _pose_params(rt, 37, 21, poses[:4])
    planes = Planes(rt, 4, 21, 37, ALL, True, stream=streams[0])
    rt.check(h.rt_render_gbuffer_table(_handle(scenes_[0]), table, cams, 4, planes.ptrs, 37 * 3, C.byref(planes.struct), C.c_void_p(streams[0].cuda_stream), 1),
             "rt_render_gbuffer_table")
    _equal(planes.results(), serial[0][0], ALL + ("image",), "another stream")
    assert h.rt_ray_table_destroy(table) == 0
    sensor.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the C ABI alone

def _pose_params(rt, w, h, poses):
    """RtCameraParams of poses for the table calls: the size and the two poses, K_inv and D left zero (they are not read)"""
    inv = rt.libs()[1].rth_invert_lre
    out = (rt.RtCameraParams * len(poses))()
    for i, ps in enumerate(poses):
        out[i].width, out[i].height = w, h
        p = np.asarray(ps, np.float32)
        q = np.zeros(6, np.float32)
        inv(p.ctypes.data_as(C.POINTER(C.c_float)), q.ctypes.data_as(C.POINTER(C.c_float)))
        for j in range(6):
            out[i].camera_pose[j] = float(p[j])
            out[i].inv_camera_pose[j] = float(q[j])
    return out


def test_c_abi_directly(world, sensors):
    import torch
    rt = world.rt
    h = rt.libs()[0]
    so, sp = world.get("demo")
    w_, h_ = 37, 21
    dirs = sensors.equirectangular(w_, h_)
    d = torch.from_numpy(dirs).to("cuda")
    torch.cuda.synchronize()
    table = C.c_void_p()
    rt.check(h.rt_ray_table_create(C.c_void_p(d.data_ptr()), w_, h_, None, 1, C.byref(table)), "rt_ray_table_create")
    wi, hi, nb = C.c_int32(), C.c_int32(), C.c_size_t()
    assert h.rt_ray_table_info(table, C.byref(wi), C.byref(hi), C.byref(nb)) == 0
    assert (wi.value, hi.value, nb.value) == (w_, h_, 5 * 3 * 768)      # 5 x 3 tiles of 768 bytes
    assert h.rt_ray_table_info(table, None, None, None) == 0
    poses = _inside_poses(3, False)
    cams = _pose_params(rt, w_, h_, poses)
    ro = torch.full((h_, w_, 3), -7.0, device="cuda")
    rd = torch.full((h_, w_, 3), -7.0, device="cuda")
    assert h.rt_ray_table_rays(table, C.byref(cams[1]), C.c_void_p(ro.data_ptr()), C.c_void_p(rd.data_ptr()), None, 1) == 0
    oo, od = sensor_oracle.rays(dirs, poses[1])
    assert np.array_equal(_bits(ro.cpu().numpy()), _bits(oo)) and np.array_equal(_bits(rd.cpu().numpy()), _bits(od))
    planes = Planes(rt, 3, h_, w_, ALL, True)
    assert h.rt_render_gbuffer_table(_handle(sp), table, cams, 3, planes.ptrs, w_ * 3, C.byref(planes.struct), None, 1) == 0
    got = planes.results()                                              # (asserts the guard words)
    _same(got, sensor_oracle.frames(so, dirs, poses), where="C ABI")
    # a pose of another size is refused by both calls, and nothing is written
    for bw, bh in ((w_ + 1, h_), (w_, h_ - 1), (40, 24)):
        wrong = _pose_params(rt, bw, bh, poses)
        assert h.rt_render_gbuffer_table(_handle(sp), table, wrong, 3, planes.ptrs, 40 * 3, C.byref(planes.struct), None, 1) == -1
        assert h.rt_ray_table_rays(table, C.byref(wrong[0]), C.c_void_p(ro.data_ptr()), C.c_void_p(rd.data_ptr()), None, 1) == -1
    mixed = _pose_params(rt, w_, h_, poses)
    mixed[2].width = w_ + 1
    assert h.rt_render_gbuffer_table(_handle(sp), table, mixed, 3, planes.ptrs, w_ * 3, C.byref(planes.struct), None, 1) == -1
    _same(planes.results(), got, where="after refused calls")
    # rt_camera_directions packs to the table the view pre-pass would have written: the rays are rt_camera_rays'
    K, D = world.scenes.scaled_K(40), world.scenes.D_REF
    cam = rt.Camera(w_, h_, K, D)
    cam.set_pose(poses[1])
    cp = cam.params()
    cdir = torch.empty((h_, w_, 3), device="cuda")
    assert h.rt_camera_directions(C.byref(cp), C.c_void_p(cdir.data_ptr()), None, 1) == 0
    t2 = C.c_void_p()
    assert h.rt_ray_table_create(C.c_void_p(cdir.data_ptr()), w_, h_, None, 1, C.byref(t2)) == 0
    assert h.rt_ray_table_rays(t2, C.byref(cp), C.c_void_p(ro.data_ptr()), C.c_void_p(rd.data_ptr()), None, 1) == 0
    co, cd = cam.rays()
    torch.cuda.synchronize()
    assert torch.equal(co.view(torch.int32), ro.view(torch.int32)) and torch.equal(cd.view(torch.int32), rd.view(torch.int32))
    cam.close()
    assert h.rt_ray_table_destroy(t2) == 0 and h.rt_ray_table_destroy(table) == 0
