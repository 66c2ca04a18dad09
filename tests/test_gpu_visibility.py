"""Visibility masks on the GPU (rt_visibility through Scene.visibility, Camera.render_visibility, Sensor.render_visibility and the
C ABI): every mask equal to the CPU oracle (tests/visibility_oracle.py) as integers.
1. Four scenes with the points the masks are interesting for -- the oracle's occluded share of the hit pixels is asserted per (frame,
   point), and on `multi` that visible and facing disagree both ways.  2. The bias: 0 (the surface shadows itself, the accepted
   distance within a few ulp of the bound), 2^-10, 0.25.  3. Sizes with ragged tiles, K = 1, 5, 32 (the sign bit), 1, 3 and 33
   frames, points that differ per frame.  4. The general stack on a chain deeper than the LDS part.  5. Against Scene.occluded on
   rays made by the rule in numpy, with and without binning.  6. The wrappers, rolling planes, plane selection between guard words
   through ctypes, the sky, a NaN point, a non-finite pose, two threads on two streams, the RT_E_INVALID cases that need a scene.
Frames are a few 8x8 tiles large: what can go wrong is tile, frame and point indexing, the bound's bits and the stack forms.  The
input planes of the oracle comparisons are the ORACLE's G-buffer planes, so these tests do not lean on the G-buffer kernel."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest

import ray_oracle
import visibility_oracle as vo
from test_gpu_dir_table import _path
from test_gpu_gbuffer import GUARD, World, _handle, _same, _views

pytestmark = pytest.mark.gpu
BOTH = ("visible", "facing")
SENTINEL = -559038737
BIAS = 2.0 ** -10
#        scene    points, as the masks are interesting from them
POINTS = dict(demo=((-0.6, 1.0, 0.7), (-0.6, 1.2, 0.3), (-0.2, 1.0, 0.4), (-1.4, 0.8, 1.0)),
              inside=((-0.6, 1.0, 0.7), (-1.4, 0.8, 1.0)),
              multi=((3.0, 0.0, 2.0), (-3.0, 2.0, 0.0), (0.0, 1.0, 3.0), (0.1 + 0.8, -3.0, 0.4)),      # (the last: MULTI_CAMERA + 0.8 in x)
              nine=((3.0, -1.0, 1.0), (-3.0, 0.0, 0.5)),
              deep=((0.3, -1.0, 0.2), (2.0, -1.0, 0.0)))
INSIDE_POSE = (-0.4, 0.8, 0.8, 0.4, -0.15, 0.0)


@pytest.fixture(scope="module")
def world(rt, orc, scenes, demo_objs, blob5k):
    w = World(rt, orc, scenes, demo_objs, blob5k)
    w.masks = {}
    yield w
    w.close()


@pytest.fixture(scope="module")
def sensors():
    return importlib.import_module("cuda-raytracing_amd.sensors")


def _frames(world, name):
    """(scene name, w, h, K, D, poses) of the frames the issue names for `name`"""
    if name == "demo":
        w, h, K, D, _p = _views(world, "demo", 1)
        return "demo", w, h, K, D, [_path(32)[0], _path(32)[31]]
    if name == "inside":
        w, h, K, D, _p = _views(world, "demo", 1)
        return "demo", w, h, K, D, [INSIDE_POSE]
    w, h, K, D, poses = _views(world, name, 1)
    return name, w, h, K, D, poses


def _oracle(world, key, scene, planes, points, bias=BIAS):
    """the oracle's masks of `planes` (computed once per key)"""
    key = (key, float(bias))
    if key not in world.masks:
        world.masks[key] = vo.masks(world.get(scene)[0], planes["instance"], planes["location"], planes["normal"], points, bias)
    return world.masks[key]


def _np(d):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}


def _visibility(sp, planes, points, outputs=BOTH, tensors=False, **kw):
    """Scene.visibility on numpy planes (the host staging) or on the same planes as CUDA tensors -> numpy masks"""
    inst, loc, nrm = planes["instance"], planes["location"], planes["normal"] if "facing" in outputs else None
    if tensors:
        import torch
        inst, loc = torch.from_numpy(np.ascontiguousarray(inst)).cuda(), torch.from_numpy(np.ascontiguousarray(loc)).cuda()
        nrm = None if nrm is None else torch.from_numpy(np.ascontiguousarray(nrm)).cuda()
    else:
        inst, loc, nrm = (None if a is None else np.ascontiguousarray(a) for a in (inst, loc, nrm))
    got = _np(sp.visibility(inst, loc, points, normal=nrm, outputs=outputs, **kw))
    assert set(got) == set(outputs)
    return got


def _shares(so, planes, points, bias=BIAS):
    """[n, K]: the share of each frame's hit pixels the oracle calls occluded from each point"""
    occ = vo.occluded(so, planes["location"], vo.points_of(points, len(planes["instance"])), bias)
    hit = planes["instance"] >= 0
    return np.stack([occ[i][hit[i]].mean(axis=0) for i in range(len(hit))])


# ---------------------------------------------------------------------------------------------------------------- 1. the oracle

@pytest.mark.parametrize("name", ["demo", "inside", "multi", "nine"])
def test_masks_equal_the_oracle(world, name):
    scene, w, h, K, D, poses = _frames(world, name)
    so, sp = world.get(scene)
    planes = world.ref(scene, w, h, K, D, poses)
    pts = POINTS[name]
    hit = planes["instance"] >= 0
    # the coverage is the ORACLE's: from every point named for the frame, between 5 % and 95 % of the hit pixels are occluded
    share = _shares(so, planes, pts)
    named = share if name != "demo" else np.concatenate([share[0], share[1][:3]])       # (demo's fourth point is named for pose 0)
    assert hit.any() and (named >= 0.05).all() and (named <= 0.95).all(), (name, share)
    if name == "inside":
        assert hit.sum() >= 0.9 * hit.size and not hit.all()
    ref = _oracle(world, name, scene, planes, pts)
    assert (ref["visible"][~hit] == 0).all() and (ref["facing"][~hit] == 0).all() and (ref["visible"] >> len(pts) == 0).all()
    if name == "multi":                                                 # visible and facing are two questions
        for a, b in (("visible", "facing"), ("facing", "visible")):
            assert ((ref[a] & ~ref[b]) != 0).sum() >= 10, (a, "without", b)
    _same(_visibility(sp, planes, pts), ref, BOTH, name + " numpy")
    _same(_visibility(sp, planes, np.float32(pts), tensors=True), ref, BOTH, name + " tensors")


# ---------------------------------------------------------------------------------------------------------------- 2. the bias

def test_the_bias_pins_the_bits_of_the_bound(world):
    scene, w, h, K, D, poses = _frames(world, "demo")
    so, sp = world.get(scene)
    planes = {k: v[:1] for k, v in world.ref(scene, w, h, K, D, poses).items()}
    pts = POINTS["demo"]
    hit = planes["instance"][0] >= 0
    zero, small = _oracle(world, "bias0", scene, planes, pts, 0.0), _oracle(world, "bias", scene, planes, pts, BIAS)
    # without a bias the surface shadows itself: the oracle answers differently, and most of the flipped rays were decided by a
    # distance within 4 ulp of the bound -- the bits of v, d and tmax are what this case compares
    flipped = (small["visible"] & ~zero["visible"])[0]
    assert all(((flipped >> k) & 1).sum() >= 50 for k in range(len(pts))), [int(((flipped >> k) & 1).sum()) for k in range(len(pts))]
    L, v, tmax = vo.rays(planes["location"], vo.points_of(pts, 1), 0.0)
    t = ray_oracle.cast_rays(so, L, v, lighting_pass=1, tmax=tmax)["t"]
    ulps = np.abs(t.view(np.int32).astype(np.int64) - tmax.view(np.int32).astype(np.int64))[0]
    close = (ulps <= 4) & hit[..., None] & (((flipped[..., None] >> np.arange(len(pts))) & 1) != 0)
    assert (close.sum(axis=(0, 1)) >= 25).all(), close.sum(axis=(0, 1))
    for key, bias in (("bias0", 0.0), ("bias", BIAS), ("bias25", 0.25)):
        ref = _oracle(world, key, scene, planes, pts, bias)
        _same(_visibility(sp, planes, pts, bias=bias), ref, BOTH, "bias %g" % bias)
    assert np.array_equal(zero["facing"], small["facing"])              # (the bias is the cast's alone)


# ---------------------------------------------------------------------------------------------------------------- 3. shapes

SIZES = ((40, 24), (13, 5), (8, 8))


def _shape_case(world, size):
    """(planes of four frames, points [4, 32, 3] that differ per frame, the oracle's masks) of a camera of `size` on the demo path"""
    key = ("shape",) + size
    if key not in world.masks:
        w, h = size
        sc = world.scenes
        poses = [_path(32)[i] for i in (0, 10, 21, 31)]
        planes = world.ref("demo", w, h, sc.scaled_K(w), sc.D_REF, poses)
        rng = np.random.default_rng(5)
        base = np.concatenate([np.float32(POINTS["demo"]), rng.uniform((-1.6, 0.4, 0.1), (0.4, 1.6, 1.3), (28, 3)).astype(np.float32)])
        pts = np.stack([base + np.float32((0.25 * i, -0.2 * i, 0.15 * i)) for i in range(4)])
        so = world.get("demo")[0]
        ref = vo.masks(so, planes["instance"], planes["location"], planes["normal"], pts)
        # an implementation that ignores the frame index cannot pass: with frame 0's points, at least a tenth of every later frame's
        # hit pixels get another answer (the first five points, the K every case has in common with K = 5 and 32)
        first = vo.masks(so, planes["instance"], planes["location"], planes["normal"], pts[0, :5])
        hit = planes["instance"] >= 0
        assert hit[0].any()
        for i in range(1, 4):
            if hit[i].sum() >= 10:
                differ = ((ref["visible"][i] & 31) != first["visible"][i]) | ((ref["facing"][i] & 31) != first["facing"][i])
                assert differ[hit[i]].mean() >= 0.1, (size, i, differ[hit[i]].mean())
        world.masks[key] = (planes, pts, ref)
    return world.masks[key]


@pytest.mark.parametrize("frames", [1, 3, 33])
@pytest.mark.parametrize("K", [1, 5, 32])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_sizes_points_and_frames(world, size, K, frames):
    planes, pts, ref = _shape_case(world, size)
    idx = np.arange(frames) % 4
    keep = np.uint32((1 << K) - 1).view(np.int32) if K == 32 else np.int32((1 << K) - 1)
    want = {k: (v[idx] & keep).astype(np.int32) for k, v in ref.items()}
    if K == 32 and size == (40, 24):
        assert (want["visible"] < 0).any() and (want["facing"] < 0).any()      # the sign bit is in use
    got = _visibility(world.get("demo")[1], {k: v[idx] for k, v in planes.items()}, pts[idx][:, :K], tensors=frames == 3)
    _same(got, want, BOTH, "%s K=%d x%d" % (size, K, frames))


def test_shared_points_are_every_frames_points(world):
    planes, pts, _ref = _shape_case(world, (40, 24))
    sp = world.get("demo")[1]
    shared = _visibility(sp, planes, pts[1, :5])
    tiled = _visibility(sp, planes, np.stack([pts[1, :5]] * 4))
    _same(shared, tiled, BOTH, "[K, 3] against [n, K, 3]")
    _same(shared, _oracle(world, "shared", "demo", planes, pts[1, :5]), BOTH, "[K, 3]")


# ---------------------------------------------------------------------------------------------------------------- 4. the stack

def test_a_chain_deeper_than_the_lds_stack(world):
    scene, w, h, K, D, poses = _frames(world, "deep")
    so, sp = world.get(scene)
    assert sp.info()["max_stack"] > 16                                   # more than the LDS part holds
    planes = world.ref(scene, w, h, K, D, poses)
    ref = _oracle(world, "deep", scene, planes, POINTS["deep"])
    hit = planes["instance"] >= 0
    assert hit.sum() > 100 and (ref["visible"][hit] == 3).all()
    _same(_visibility(sp, planes, POINTS["deep"]), ref, BOTH, "deep")


# ---------------------------------------------------------------------------------------------------------------- 5. the library itself

@pytest.mark.parametrize("name", ["demo", "multi"])
def test_visible_is_what_scene_occluded_answers(world, name):
    scene, w, h, K, D, poses = _frames(world, name)
    sp = world.get(scene)[1]
    planes = world.ref(scene, w, h, K, D, poses)
    pts = vo.points_of(POINTS[name], len(poses))
    L, v, tmax = vo.rays(planes["location"], pts, BIAS)
    hit = (planes["instance"] >= 0)[..., None]
    got = _visibility(sp, planes, pts, outputs=("visible",))["visible"]
    for binning in (False, True):
        occ = sp.occluded(L, v, tmax, binning=binning)
        assert np.array_equal(vo.pack((occ == 0) & hit), got), binning


# ---------------------------------------------------------------------------------------------------------------- 6. plumbing

def _gbuffer_then_visibility(owner, sp, pts, poses, gbuffer, bias=BIAS):
    planes = owner.render_gbuffer(sp, poses, outputs=tuple(set(gbuffer) | {"instance", "location", "normal"}))
    masks = sp.visibility(planes["instance"], planes["location"], pts, normal=planes["normal"], bias=bias, outputs=BOTH)
    return _np(dict({k: planes[k] for k in gbuffer}, **masks))


def test_camera_render_visibility_is_gbuffer_then_visibility(world):
    scene, w, h, K, D, poses = _frames(world, "demo")
    sp = world.get(scene)[1]
    poses = [_path(32)[i % 32] for i in range(35)]                      # (two launches of the G-buffer, one of the masks)
    pts = np.float32(POINTS["demo"])
    cam = world.rt.Camera(w, h, K, D)
    try:
        want = _gbuffer_then_visibility(cam, sp, pts, poses, ("t", "location", "uv"))
        got = cam.render_visibility(sp, pts, poses, outputs=BOTH, gbuffer=("t", "location", "uv"), image=True)
        assert set(got) == {"visible", "facing", "t", "location", "uv", "image"}
        _same(_np(got), want, ("visible", "facing", "t", "location", "uv"), "camera")
        assert np.array_equal(_np(got)["image"], _np(cam.render_gbuffer(sp, poses, outputs=(), image=True))["image"])
        ref = _oracle(world, "demo", scene, world.ref(scene, w, h, K, D, [poses[0], poses[31]]), POINTS["demo"])
        assert np.array_equal(want["visible"][[0, 31]], ref["visible"]) and np.array_equal(want["facing"][[0, 31]], ref["facing"])
        # the defaults: the current pose, visible alone, numpy on request; per-frame points
        cam.set_pose(poses[3])
        one = cam.render_visibility(sp, pts, as_numpy=True)
        assert set(one) == {"visible"} and isinstance(one["visible"], np.ndarray) and np.array_equal(one["visible"], want["visible"][3:4])
        per = np.stack([pts + np.float32(0.1 * i) for i in range(3)])
        got = _np(cam.render_visibility(sp, per, poses[:3], outputs=("facing",)))
        for i in range(3):
            assert np.array_equal(got["facing"][i], _gbuffer_then_visibility(cam, sp, per[i], poses[i:i + 1], ())["facing"][0]), i
    finally:
        cam.close()


def test_sensor_render_visibility_is_gbuffer_then_visibility(world, sensors):
    sp = world.get("demo")[1]
    lidar = world.rt.Sensor(sensors.spinning_lidar(np.radians(np.linspace(-25.0, 15.0, 16)), 128))
    pts = np.float32(POINTS["inside"])
    poses = [INSIDE_POSE, (-0.35, 0.76, 0.82, 0.7, -0.1, 0.1)]
    try:
        want = _gbuffer_then_visibility(lidar, sp, pts, poses, ("t", "instance"))
        assert ((want["visible"] & 1) != 0).mean() > 0.2 and (want["visible"] != want["facing"]).any()
        got = lidar.render_visibility(sp, pts, poses, outputs=BOTH, gbuffer=("t", "instance"))
        assert set(got) == {"visible", "facing", "t", "instance"}
        _same(_np(got), want, ("visible", "facing", "t", "instance"), "lidar")
    finally:
        lidar.close()


def test_rolling_planes_serve(world, sensors):
    """Sensor.render_rolling's planes through Scene.visibility equal the oracle on those planes: 64 x 24, four slices of 16 columns"""
    so, sp = world.get("demo")
    pano = world.rt.Sensor(sensors.equirectangular(64, 24))
    try:
        poses = np.stack([sensors.rolling_poses(INSIDE_POSE, (-0.3, 0.7, 0.85, 0.9, -0.1, 0.1), 4)] * 2)
        poses[1, :, 0] += np.float32(0.05)
        planes = _np(pano.render_rolling(sp, poses, axis="x", slice_pixels=16, outputs=("instance", "location", "normal")))
        assert 0.3 < (planes["instance"] >= 0).mean() < 1.0
        ref = vo.masks(so, planes["instance"], planes["location"], planes["normal"], POINTS["inside"])
        assert (ref["visible"] != 0).any() and (ref["visible"] != 3)[planes["instance"] >= 0].any()
        _same(_visibility(sp, planes, POINTS["inside"]), ref, BOTH, "rolling")
    finally:
        pano.close()


@pytest.mark.parametrize("which", BOTH)
def test_one_plane_between_guard_words_through_ctypes(world, which):
    import torch
    scene, w, h, K, D, poses = _frames(world, "demo")
    sp = world.get(scene)[1]
    planes = world.ref(scene, w, h, K, D, poses)
    ref = _oracle(world, "demo", scene, planes, POINTS["demo"])
    n = len(poses)
    dev = {k: torch.from_numpy(np.ascontiguousarray(planes[k])).cuda() for k in ("instance", "location", "normal")}
    pts = torch.from_numpy(vo.points_of(POINTS["demo"], n)).cuda()
    buf = torch.full((n * h * w + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    out = world.rt.RtVisibility(**{which: buf.data_ptr() + 4 * GUARD})
    nrm = dev["normal"].data_ptr() if which == "facing" else None
    rc = world.rt.libs()[0].rt_visibility(_handle(sp), dev["instance"].data_ptr(), dev["location"].data_ptr(), nrm, w, h, n, pts.data_ptr(), 4,
                                          BIAS, C.byref(out), None, 1)
    assert rc == 0
    a = buf.cpu().numpy()
    assert (a[:GUARD] == SENTINEL).all() and (a[-GUARD:] == SENTINEL).all()
    assert np.array_equal(a[GUARD:-GUARD].reshape(n, h, w), ref[which])


def test_the_sky_is_all_zero(world):
    scene, w, h, K, D, poses = _frames(world, "demo")
    sp = world.get(scene)[1]
    away = [(p[0], p[1], p[2], p[3] + np.pi, p[4], p[5]) for p in poses]
    cam = world.rt.Camera(w, h, K, D)
    try:
        got = _np(cam.render_visibility(sp, POINTS["demo"], away, outputs=BOTH, gbuffer=("instance",)))
    finally:
        cam.close()
    assert (got["instance"] == -1).all() and not got["visible"].any() and not got["facing"].any()


def test_a_nan_point_changes_no_other_bit(world):
    scene, w, h, K, D, poses = _frames(world, "demo")
    sp = world.get(scene)[1]
    planes = world.ref(scene, w, h, K, D, poses)
    ref = _oracle(world, "demo", scene, planes, POINTS["demo"])
    for bad in ((np.nan, 1.0, 0.7), (np.inf, 1.0, 0.7), (-0.6, -np.inf, np.nan)):
        pts = np.float32(POINTS["demo"])
        pts[1] = bad
        got = _visibility(sp, planes, pts)
        for k in BOTH:
            assert np.array_equal(got[k] & 0b1101, ref[k] & 0b1101) and (got[k] >> 4 == 0).all(), (k, bad)
    # a point ON a seen surface point (v == 0 for that pixel): no fault, the other points' bits are what they were
    hit = np.argwhere(planes["instance"][0] >= 0)[7]
    pts = np.float32(POINTS["demo"])
    pts[2] = planes["location"][0, hit[0], hit[1]]
    got = _visibility(sp, planes, pts)
    for k in BOTH:
        assert np.array_equal(got[k] & 0b1011, ref[k] & 0b1011), k


def test_a_non_finite_pose_changes_no_other_frame(world):
    scene, w, h, K, D, _poses = _frames(world, "demo")
    sp = world.get(scene)[1]
    poses = [_path(32)[i] for i in (0, 10, 21, 31)]
    bad = list(poses)
    bad[1] = (float("nan"), poses[1][1], float("inf"), poses[1][3], float("nan"), 0.0)
    cam = world.rt.Camera(w, h, K, D)
    try:
        want = _np(cam.render_visibility(sp, POINTS["demo"], poses, outputs=BOTH))
        got = _np(cam.render_visibility(sp, POINTS["demo"], bad, outputs=BOTH))
    finally:
        cam.close()
    keep = [0, 2, 3]
    assert want["visible"][keep].any()
    for k in BOTH:
        assert np.array_equal(got[k][keep], want[k][keep]), k


def test_two_threads_on_two_streams(world):
    """two threads, a stream each, six calls each with no wait in between, one scene: every result equals the oracle"""
    import torch
    planes, pts, ref = _shape_case(world, (40, 24))
    sp = world.get("demo")[1]
    dev = {k: torch.from_numpy(np.ascontiguousarray(planes[k])).cuda() for k in ("instance", "location", "normal")}
    jobs = [(torch.cuda.Stream(), [0, 1]), (torch.cuda.Stream(), [2, 3])]
    # (the inputs of every call are made before the threads start: nothing of a call runs on another stream than its own)
    cut = {tuple(sel): {k: v[sel].contiguous() for k, v in dev.items()} for _s, idx in jobs for sel in (idx, idx[1:])}
    points = {sel: torch.from_numpy(np.ascontiguousarray(pts[list(sel)])).cuda() for sel in cut}
    torch.cuda.synchronize()
    go, out, errors = threading.Barrier(2), [None, None], []

    def worker(j):
        try:
            stream, idx = jobs[j]
            go.wait(60)
            res = []
            for r in range(6):
                sel = idx if r % 2 == 0 else idx[1:]
                a = cut[tuple(sel)]
                res.append((sel, sp.visibility(a["instance"], a["location"], points[tuple(sel)], normal=a["normal"], outputs=BOTH, stream=stream)))
            stream.synchronize()
            out[j] = res
        except Exception as e:                                          # noqa: BLE001 (reported below, on the main thread)
            errors.append((j, repr(e)))

    threads = [threading.Thread(target=worker, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors and not any(t.is_alive() for t in threads), errors
    for j in range(2):
        for sel, got in out[j]:
            _same(_np(got), {k: v[sel] for k, v in ref.items()}, BOTH, "stream %d frames %s" % (j, sel))


def test_invalid_arguments_with_a_real_scene(world):
    import torch
    scene, w, h, K, D, poses = _frames(world, "demo")
    sp = world.get(scene)[1]
    planes = world.ref(scene, w, h, K, D, poses)
    ref = _oracle(world, "demo", scene, planes, POINTS["demo"])
    n = len(poses)
    dev = {k: torch.from_numpy(np.ascontiguousarray(planes[k])).cuda() for k in ("instance", "location", "normal")}
    pts = torch.from_numpy(vo.points_of(POINTS["demo"], n)).cuda()
    vis, fac = (torch.full((n, h, w), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))
    both, none, only_f = world.rt.RtVisibility(vis.data_ptr(), fac.data_ptr()), world.rt.RtVisibility(), world.rt.RtVisibility(facing=fac.data_ptr())
    f = world.rt.libs()[0].rt_visibility

    def call(inst=dev["instance"].data_ptr(), loc=dev["location"].data_ptr(), nrm=dev["normal"].data_ptr(), ww=w, hh=h, nn=n, p=pts.data_ptr(), kk=4,
             bias=BIAS, out=both):
        return f(_handle(sp), inst, loc, nrm, ww, hh, nn, p, kk, bias, C.byref(out) if out is not None else None, None, 1)

    bad = [dict(inst=None), dict(loc=None), dict(p=None), dict(out=None), dict(out=none), dict(nrm=None), dict(nrm=None, out=only_f), dict(ww=0), dict(hh=-1),
           dict(nn=0), dict(ww=2 ** 16, hh=2 ** 15, nn=1), dict(kk=0), dict(kk=33), dict(bias=1.0), dict(bias=-BIAS), dict(bias=float("nan")),
           dict(bias=float("inf"))]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert (vis == SENTINEL).all() and (fac == SENTINEL).all()          # nothing was launched
    assert call() == 0
    assert np.array_equal(vis.cpu().numpy(), ref["visible"]) and np.array_equal(fac.cpu().numpy(), ref["facing"])
    host = world.rt.libs()[1].rth_scene_visibility                      # the facade gives the same answers
    assert host(sp.h, dev["instance"].data_ptr(), dev["location"].data_ptr(), None, w, h, n, pts.data_ptr(), 4, BIAS, C.byref(both), None, 1) == -1
    vis.fill_(SENTINEL)
    assert host(sp.h, dev["instance"].data_ptr(), dev["location"].data_ptr(), dev["normal"].data_ptr(), w, h, n, pts.data_ptr(), 4, 0.0,
                C.byref(both), None, 1) == 0
    assert np.array_equal(vis.cpu().numpy(), _oracle(world, "bias0x2", scene, planes, POINTS["demo"], 0.0)["visible"])
