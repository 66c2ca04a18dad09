"""Ray headers (RayHeader, rt_device_types.h): a launch that renders through view records also gets, per frame and instance, one
64-byte block with everything of the instance a wave needs before its loop -- the origin in mesh space and whether it is finite, the
mesh's flags, the root, the view delta, the direction's transform -- written by the view pre-pass and read by render_kernel<.., VIEW>
through the scalar cache.  Single-frame launches, the instrumented kernel and the oracle know nothing of it: every frame of a batch
must equal, bit for bit, the frame they give for the same scene state and pose (RGB of the batch; RGB and hit ids of the production
kernel's single-frame launch, rt_render_ids, against the oracle; every plane of the instrumented kernel against the oracle), and
every batch must really have rendered through views (rt_scene_view_stats).

(Hit-id planes are never written by a launch that reads headers: rt_render_ids is a single-frame launch, and launch() takes no
view slot for it; the header path's hits are held to the oracle through the batch's RGB -- textured, so a colour depends on the
triangle and on where it was hit -- and through the instrumented copy of the kernel.)

Shapes: 256 x 160 is what four frames of the 5k blob need to bring eight rays per interior record (4 598 of them) -- the launch
code's condition, which tests/conftest.py lifts for the suite anyway; smaller frames only where the frame's shape is the point."""
import ctypes as C

import numpy as np
import pytest

import caller_trees as ct
import scene_defs as sd

pytestmark = pytest.mark.gpu
PLANES = ("hit_inst", "hit_tri", "pops", "aabb", "tris", "inside")
W, H = 256, 160
# four cameras in front of the scenes below, each with its own position and orientation
POSES = [(0.1, -4.2, 0.4, 0.15, -0.05, 0.1), (-0.6, -3.6, 0.1, -0.1, 0.05, 0.0), (0.7, -4.8, 0.9, 0.2, -0.15, -0.2), (0.0, -3.9, -0.3, 0.0, 0.1, 0.3)]
MORE_POSES = POSES + [(0.3 - 0.2 * i, -4.0 - 0.1 * i, 0.2 + 0.1 * i, 0.05 * i, -0.03 * i, 0.04 * i) for i in range(4)]
IDENTITY = ((0.0,) * 6, (1.0, 1.0, 1.0))
TRANSLATED = ((1.8, 0.5, 0.2, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
POSED = ((-1.6, 0.8, 0.3, 0.7, 0.3, -0.4), (0.6, 1.1, 0.8))


def _posed_scene(blob5k):
    """one mesh, three instances: the identity, a pure translation, one rotated and non-uniformly scaled; a texture, so that a
    pixel's colour depends on where its triangle was hit"""
    return sd.SceneDesc([((1.0, 1.0, 1.0), sd.checker_texture()), ((0.9, 0.5, 0.2), None)], [("obj", blob5k)],
                        [(0, 0) + IDENTITY, (0, 1) + TRANSLATED, (0, 0) + POSED])


def _handle(sp):
    h = sp.device_handle
    return h if isinstance(h, C.c_void_p) else C.c_void_p(h)


def _batch(rt, sp, cam, poses, stream=None, bufs=None, synchronize=True):
    """rt_render_batch itself (the production kernels; a scene with or without a host scene behind it): poses[i] -> frame i, after
    asserting that the launch took a view slot.  With synchronize=False the caller reads `bufs` after its own synchronise."""
    n = len(poses)
    cams = (rt.RtCameraParams * n)()
    for i, ps in enumerate(poses):
        cam.set_pose(ps)
        rt.libs()[1].rth_camera_params(cam.h, C.addressof(cams[i]))
    own = bufs is None
    bufs = bufs or [rt.DeviceBuffer(width_bytes=cam.width * 3, height=cam.height) for _ in range(n)]
    ptrs = (C.c_void_p * n)(*[int(b.ptr) if not isinstance(b.ptr, C.c_void_p) else b.ptr.value for b in bufs])
    before = sp.view_stats()
    rt.check(rt.libs()[0].rt_render_batch(_handle(sp), cams, ptrs, C.c_size_t(bufs[0].pitch), C.c_int32(n), C.c_void_p(stream),
                                          C.c_int(1 if synchronize else 0)), "rt_render_batch")
    after = sp.view_stats()
    assert after["launches"] == before["launches"] + 1 and after["fallbacks"] == before["fallbacks"], (before, after)
    if not synchronize:
        return bufs
    frames = [b.to_host().reshape(cam.height, cam.width, 3) for b in bufs]
    if own:
        for b in bufs:
            b.free()
    return frames


def _reference(rt, scenes, so, sp, cam, K, pose, planes=True, threads=8):
    """The frame of `pose` three ways that read no header -- the oracle, the instrumented kernel, the production kernel in a
    single-frame launch with its hit ids -- which must agree as tests/test_gpu_parity.py::_compare asks; returns the frame.
    planes=False: a caller's own tree visits other nodes than the oracle's; RGB and hit ids do not depend on the tree."""
    ref = so.render(cam.width, cam.height, K, scenes.D_REF, pose, threads=threads)
    cam.set_pose(pose)
    launches = sp.view_stats()["launches"]
    dbg = rt.render_debug(sp, cam)
    ids = rt.render_ids(sp, cam)
    assert sp.view_stats()["launches"] == launches              # (single frames take no views)
    for n in ("img", "hit_inst", "hit_tri"):
        assert np.array_equal(ids[n], ref[n]), "production kernel %s: %d pixels differ from the oracle" % (n, int((ids[n] != ref[n]).sum()))
    for n in ("img",) + (PLANES if planes else PLANES[:2]):
        assert np.array_equal(dbg[n], ref[n]), "instrumented kernel %s: %d pixels differ from the oracle" % (n, int((dbg[n] != ref[n]).sum()))
    return ref["img"]


def _camera(rt, scenes, w, h, K):
    return rt.Camera(w, h, K, scenes.D_REF)


def _same(frames, want, what):
    for k, (f, w_) in enumerate(zip(frames, want)):
        assert np.array_equal(f, w_), "%s: frame %d differs in %d pixels" % (what, k, int((f != w_).any(axis=2).sum()))


def _check(rt, orc, scenes, desc, w=W, h=H, K=None, poses=POSES):
    K = K or scenes.scaled_K(w)
    so, sp = desc.build_oracle(orc), desc.build_product(rt)
    sp.upload_to_device()
    cam = _camera(rt, scenes, w, h, K)
    want = [_reference(rt, scenes, so, sp, cam, K, ps) for ps in poses]
    so.close()
    frames = _batch(rt, sp, cam, poses)
    _same(frames, want, "%d x %d" % (w, h))
    return sp, cam, want


def test_posed_instances(rt, orc, scenes, blob5k):
    """The identity, a translation, a rotation with a non-uniform scale: four frames, each from its own camera."""
    sp, cam, want = _check(rt, orc, scenes, _posed_scene(blob5k))
    assert all(len(np.unique(f.reshape(-1, 3), axis=0)) > 20 for f in want)         # the textured instances are on screen
    assert len({f.tobytes() for f in want}) == 4
    st, _ = _loop_stats(rt, sp, cam, POSES)
    assert st["asm_posed"] > 0 and st["asm"] > 2 * st["asm_posed"] and st["asm_loop_frac"] > 0.8, st   # one of the three goes back through the transform


def _loop_stats(rt, sp, cam, poses):
    bufs = [rt.DeviceBuffer(width_bytes=cam.width * 3, height=cam.height) for _ in poses]
    before = sp.view_stats()
    st = rt.Scene.loop_stats(sp, cam, poses, [b.ptr for b in bufs], bufs[0].pitch)
    after = sp.view_stats()
    assert after["launches"] == before["launches"] + 1 and after["fallbacks"] == before["fallbacks"], (before, after)
    frames = [b.to_host().reshape(cam.height, cam.width, 3) for b in bufs]
    for b in bufs:
        b.free()
    waves = len(poses) * ((cam.width + 7) // 8) * ((cam.height + 7) // 8)
    assert st["waves"] == waves and st["retraced_lanes"] == 0 and st["deep"] == 0, st
    return st, frames


def test_eight_instances_then_nine(rt, orc, scenes):
    """kMaxViewInstances = 8 headers per frame; a ninth instance (behind every camera: no ray meets it) takes the whole scene off
    the view path -- no pre-pass, no header, the code of before -- and leaves the frames as they were."""
    tris = sd.random_triangles(400, seed=17, spread=0.5, size=0.2)
    rng = np.random.default_rng(5)
    inst = []
    for k in range(8):
        pose = (1.4 * (k % 4) - 2.1, 0.8 * (k // 4), 1.2 * (k // 4) - 0.6) + tuple(float(a) for a in rng.uniform(-0.8, 0.8, 3) * (k > 0))
        scale = tuple(float(s) for s in rng.uniform(0.6, 1.3, 3)) if k > 1 else (1.0, 1.0, 1.0)
        inst.append((0, k % 2, pose, scale))
    mats = [((1.0, 1.0, 1.0), sd.checker_texture(32, 24, seed=3)), ((0.2, 0.7, 0.4), None)]
    K = scenes.scaled_K(W)
    eight = sd.SceneDesc(mats, [("tris", tris)], inst)
    sp, cam, want = _check(rt, orc, scenes, eight)
    assert sp.view_stats()["launches"] == 1
    nine = sd.SceneDesc(mats, [("tris", tris)], inst + [(0, 1, (0.0, -40.0, 0.0, 0.3, 0.2, 0.1), (1.0, 1.0, 1.0))])
    so, sp9 = nine.build_oracle(orc), nine.build_product(rt)
    sp9.upload_to_device()
    for k in (0, 3):
        assert np.array_equal(_reference(rt, scenes, so, sp9, cam, K, POSES[k]), want[k])
    so.close()
    bufs = [rt.DeviceBuffer(width_bytes=W * 3, height=H) for _ in POSES]
    cam.render_scene_batch(sp9, POSES, [b.ptr for b in bufs], bufs[0].pitch, synchronize=True)
    st = sp9.view_stats()
    assert st["launches"] == 0 and st["slot_frames"] == 0, st
    _same([b.to_host().reshape(H, W, 3) for b in bufs], want, "nine instances")
    for b in bufs:
        b.free()


def test_origin_that_is_not_finite_in_mesh_space(rt, orc, scenes, blob5k):
    """An instance scaled by 2e-38: inv_scale = 5e37 takes a camera seven units away to infinity in its mesh space.  The header's
    finiteness bit keeps every wave's cast on that instance off the octant loops (the hand-written one among them), as the per-lane
    compares did; the other instance stays on the hand-written loop."""
    tiny = (2.0e-38,) * 3
    desc = sd.SceneDesc([((0.9, 0.5, 0.2), None)], [("obj", blob5k)], [(0, 0) + IDENTITY, (0, 0, (0.4, 6.0, 0.1, 0.3, -0.2, 0.1), tiny)])
    poses = [(ps[0], ps[1] - 4.0) + ps[2:] for ps in POSES]       # every camera more than seven units in front of the tiny instance
    o = orc.oracle()
    q = o.euler2quat(np.array([0.3, -0.2, 0.1], np.float32))
    for ps in poses:
        with np.errstate(over="ignore"):
            ro = o.apply_quat(q, np.array(ps[:3], np.float32) - np.array([0.4, 6.0, 0.1], np.float32)) * np.float32(5e37)
        assert not np.isfinite(ro).all(), (ps, ro)
    sp, cam, want = _check(rt, orc, scenes, desc, poses=poses)
    st, frames = _loop_stats(rt, sp, cam, poses)
    _same(frames, want, "instrumented copy of the production kernel")
    waves = st["waves"]
    assert st["asm"] + st["cpp_octant"] + st["cpp_generic"] == 2 * waves, st
    assert st["cpp_generic"] >= waves and st["cpp_octant"] == 0 and 0.9 * waves < st["asm"] <= waves, st


def test_mesh_with_an_unordered_box_beside_a_clean_one(rt, orc, scenes, blob5k):
    """mesh_flags bit 0 travels in the header: a caller's tree with empty leaves (inverted boxes) as the first instance's mesh,
    the library's own tree over other triangles as the second's."""
    tris = [ct.mesh_a(), sd.random_triangles(300, seed=11, spread=0.8, size=0.3)]
    mats = [((1.0, 1.0, 1.0), sd.checker_texture()), ((0.9, 0.5, 0.2), None)]
    inst = [(0, 0) + POSED, (1, 1) + TRANSLATED]
    so = sd.SceneDesc(mats, [("tris", t) for t in tris], inst).build_oracle(orc)
    trees = [ct.variant(rt, "median_empty", tris[0], 0), ct.library_tree(rt.Mesh.from_triangles(tris[1]).dump())]
    sp = ct.RawScene(rt, list(zip(tris, trees)), mats, inst)
    try:
        assert [sp.mesh_flags(k) & 1 for k in range(2)] == [1, 0]
        K = scenes.scaled_K(W)
        cam = _camera(rt, scenes, W, H, K)
        want = [_reference(rt, scenes, so, sp, cam, K, ps, planes=False) for ps in POSES]
        _same(_batch(rt, sp, cam, POSES), want, "caller's tree")
        st, frames = _loop_stats(rt, sp, cam, POSES)
        _same(frames, want, "instrumented copy of the production kernel")
        assert st["cpp_generic"] >= st["waves"] and st["cpp_octant"] == 0 and 0.8 * st["waves"] < st["asm"] <= st["waves"], st
    finally:
        so.close()
        sp.close()


def test_exact_uv_mesh_as_second_instance(rt, orc, scenes, blob5k):
    """uv values beyond 1e37 put a mesh in the mode that tests uv per candidate: the compiler's loops, and the header says so."""
    tris = sd.random_triangles(200, seed=5, spread=0.8, size=0.3)
    tris[7, 12] = np.float32(3e38)
    tris[1::7, 14] = np.float32(np.finfo(np.float32).max)
    desc = sd.SceneDesc([((1.0, 1.0, 1.0), sd.checker_texture()), ((0.8, 0.8, 0.1), None)], [("obj", blob5k), ("tris", tris)],
                        [(0, 0) + IDENTITY, (1, 1) + TRANSLATED])
    sp, cam, want = _check(rt, orc, scenes, desc)
    st, frames = _loop_stats(rt, sp, cam, POSES)
    _same(frames, want, "instrumented copy of the production kernel")
    waves = st["waves"]
    assert st["asm"] + st["cpp_octant"] + st["cpp_generic"] == 2 * waves, st
    assert st["cpp_octant"] + st["cpp_generic"] >= waves and 0.9 * waves < st["asm"] <= waves and st["asm_posed"] == 0, st


@pytest.mark.parametrize("w,h", [(250, 130), (8, 2048)])
def test_frame_sizes(rt, orc, scenes, blob5k, w, h):
    """Widths and heights that are no multiples of the 8 x 8 tile, and a frame one tile wide and 256 tiles high: the edges of
    the grid of (tiles_x, tiles_y, frames) workgroups."""
    K = scenes.scaled_K(w) if w > 8 else (600.0, 0.0, 4.0, 0.0, 600.0, 1024.0, 0.0, 0.0, 1.0)
    _, _, want = _check(rt, orc, scenes, _posed_scene(blob5k), w, h, K)
    assert all((f != np.array([255, 204, 153], np.uint8)).any(axis=2).sum() > (50 if w == 8 else 1000) for f in want)


def test_header_lifetime(rt, orc, scenes, blob5k):
    """A header is rewritten by the pre-pass of every launch that uses its slot: an instance updated between two batches queued on
    one stream, two streams with poses of their own sharing the pool's three slots, a slot that grows from 4 to 32 frames between
    two launches -- every frame is the oracle's for the state the launch was queued in."""
    import torch
    desc = _posed_scene(blob5k)
    K = scenes.scaled_K(W)
    so, sp = desc.build_oracle(orc), desc.build_product(rt)
    sp.upload_to_device()
    cam = _camera(rt, scenes, W, H, K)
    first = {ps: _reference(rt, scenes, so, sp, cam, K, ps) for ps in MORE_POSES}
    # two streams, each with a camera and poses of its own; three rounds without a host wait in between
    streams = [torch.cuda.Stream() for _ in range(2)]
    cams = [_camera(rt, scenes, W, H, K) for _ in streams]
    sets = [[[rt.DeviceBuffer(width_bytes=W * 3, height=H) for _ in range(4)] for _ in range(3)] for _ in streams]
    mine = [[MORE_POSES[(2 * rep + 4 * k + i) % 8] for i in range(4)] for k in range(2) for rep in range(3)]
    for rep in range(3):
        for k, st_ in enumerate(streams):
            _batch(rt, sp, cams[k], mine[3 * k + rep], stream=st_.cuda_stream, bufs=sets[k][rep], synchronize=False)
    torch.cuda.synchronize()
    for k in range(2):
        for rep in range(3):
            _same([b.to_host().reshape(H, W, 3) for b in sets[k][rep]], [first[ps] for ps in mine[3 * k + rep]], "stream %d round %d" % (k, rep))
    assert sp.view_stats()["slot_frames"] == 4
    # an update between two batches on one stream (the default one), queued back to back
    bufs = [[rt.DeviceBuffer(width_bytes=W * 3, height=H) for _ in range(4)] for _ in range(2)]
    moved_pose, moved_scale = (0.9, 0.4, -0.2, -0.3, 0.2, 0.5), (0.9, 0.8, 1.2)
    _batch(rt, sp, cam, POSES, bufs=bufs[0], synchronize=False)
    sp.update_mesh_instance(1, 0, 1, moved_pose, moved_scale, stream=None)
    _batch(rt, sp, cam, POSES, bufs=bufs[1], synchronize=False)
    torch.cuda.synchronize()
    so.update_instance(1, 0, 1, moved_pose, moved_scale)
    second = {ps: _reference(rt, scenes, so, sp, cam, K, ps) for ps in MORE_POSES}
    _same([b.to_host().reshape(H, W, 3) for b in bufs[0]], [first[ps] for ps in POSES], "before the update")
    _same([b.to_host().reshape(H, W, 3) for b in bufs[1]], [second[ps] for ps in POSES], "after the update")
    assert not any(np.array_equal(first[ps], second[ps]) for ps in POSES)
    # the slot grows from 4 to 32 frames: the record array moves, the headers with it
    grows = sp.view_stats()["grows"]
    many = [MORE_POSES[(3 * i) % 8] for i in range(32)]
    _same(_batch(rt, sp, cam, many), [second[ps] for ps in many], "32 frames")
    st = sp.view_stats()
    assert st["slot_frames"] == 32 and st["grows"] == grows + 1 and st["fallbacks"] == 0, st
    _same(_batch(rt, sp, cam, POSES), [second[ps] for ps in POSES], "four frames in the grown slot")
    so.close()
    for b in [b for s_ in sets for r in s_ for b in r] + bufs[0] + bufs[1]:
        b.free()


@pytest.mark.parametrize("prof", [False, True])
def test_trace_rows_follow_the_grid(rt, scenes, blob5k, monkeypatch, tmp_path, prof):
    """RT_TRACE_FILE: one row of sixteen words per wave, at the workgroup's linear index in the (tiles_x, tiles_y, frames) grid --
    frame-major -- from both writers: render_kernel's stamps (words 0..3: start, end, hardware id, tile) and, with RT_TRACE_PROF,
    trace_loop's phase sums (words 4..13; word 8 = the longest lane's iterations).  Three frames: no frame's rows stay empty and
    none collects another's sums."""
    w, h, n = 64, 48, 3
    tiles = (w // 8) * (h // 8)
    sp = sd.blob_scene(scenes, blob5k).build_product(rt)
    sp.upload_to_device()
    cam = _camera(rt, scenes, w, h, scenes.scaled_K(w))
    path = tmp_path / "trace.bin"
    monkeypatch.setenv("RT_TRACE_FILE", str(path))
    if prof:
        monkeypatch.setenv("RT_TRACE_PROF", "1")
    bufs = [rt.DeviceBuffer(width_bytes=w * 3, height=h) for _ in range(n)]
    cam.render_scene_batch(sp, [scenes.C2_CAMERAS["near"]] * n, [b.ptr for b in bufs], bufs[0].pitch, synchronize=True)
    monkeypatch.delenv("RT_TRACE_FILE")
    for b in bufs:
        b.free()
    t = np.fromfile(path, dtype=np.uint64).reshape(-1, 16)
    assert t.shape[0] == n * tiles
    assert (t[:, 0] > 0).all() and (t[:, 1] >= t[:, 0]).all()
    assert np.array_equal(t[:, 3].astype(np.int64), np.tile(np.arange(tiles), n))
    if prof:
        its = t[:, 8].astype(np.int64).reshape(n, tiles)
        assert (its > 0).all() and np.array_equal(its[0], its[1]) and np.array_equal(its[0], its[2]), its     # (the same pose three times)
    else:
        assert not t[:, 4:14].any()
