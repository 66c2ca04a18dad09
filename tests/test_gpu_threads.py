"""One scene driven from several host threads and streams at once ("Threads"): calls on one scene are
serialised by the scene's call_mu only while they prepare and queue their launches, so everything a scene owns on the device
and shares between calls must be ordered between streams by the library itself.  Every check is bit for bit against the oracle
(tests/orc.py, tests/ray_oracle.py) of a known scene state, never against another GPU run alone.

The threads call the C-ABI on the scene's device handle (ctypes releases the GIL inside a call, so the calls really overlap), each
on its own torch stream (non-blocking: not ordered against the NULL stream) with its own camera and image buffers.  A thread that
raises fails the test with its traceback; a thread still alive after its deadline fails it with its name.  Nothing retries."""
import ctypes as C
import threading
import time
import traceback

import numpy as np
import pytest

import ray_oracle
import scene_defs as sd

pytestmark = pytest.mark.gpu
PLANES = ("hit_inst", "hit_tri", "pops", "aabb", "tris", "inside")
RAY_OUTPUTS = ("t", "instance", "triangle", "location", "normal", "uv", "pops")
DEADLINE = 120.0
_f = C.POINTER(C.c_float)


class _Threads:
    """Worker threads whose exceptions are re-raised in the main thread; a failing worker breaks the barriers the others wait on."""

    def __init__(self):
        self.threads, self.errors, self.barriers = [], [], []

    def barrier(self, parties):
        b = threading.Barrier(parties, timeout=DEADLINE)
        self.barriers.append(b)
        return b

    def start(self, name, fn, *args):
        def run():
            try:
                fn(*args)
            except BaseException as e:                         # noqa: B902 (re-raised in the main thread by join)
                self.errors.append((name, e, traceback.format_exc()))
                for b in self.barriers:
                    b.abort()
        t = threading.Thread(target=run, name=name, daemon=True)
        self.threads.append(t)
        t.start()

    def join(self):
        end = time.monotonic() + DEADLINE
        for t in self.threads:
            t.join(timeout=max(0.0, end - time.monotonic()))
        # the first error that is not a consequence of another thread's failure (a barrier it broke)
        real = [e for e in self.errors if not isinstance(e[1], threading.BrokenBarrierError)] or self.errors
        if real:
            name, e, tb = real[0]
            raise AssertionError("thread %s raised:\n%s" % (name, tb)) from e
        alive = [t.name for t in self.threads if t.is_alive()]
        assert not alive, "threads still running after %.0f s: %s" % (DEADLINE, alive)


def _render_batch_fn(rt):
    """rt_render_batch (a prototype of its own: the package's bindings do not declare it)"""
    proto = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(rt.RtCameraParams), C.POINTER(C.c_void_p), C.c_size_t, C.c_int32, C.c_void_p, C.c_int)
    return proto(("rt_render_batch", rt.libs()[0]))


def _params(rt, cam, pose):
    cam.set_pose(pose)
    return cam.params()


def _debug_frame(rt, handle, params, stream, W, H):
    """rt_render_debug of one frame on `stream` (torch): dict(img, *PLANES) as numpy, after the stream has passed it"""
    import torch
    with torch.cuda.stream(stream):
        img = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
        planes = {n: torch.empty((H, W), dtype=torch.int32, device="cuda") for n in PLANES}
        dp = rt.RtDebugPlanes(*[planes[n].data_ptr() for n in PLANES])
        rt.check(rt.libs()[0].rt_render_debug(handle, C.byref(params), img.data_ptr(), W * 3, C.byref(dp), stream.cuda_stream, 1),
                 "rt_render_debug")
        out = dict(img=img.cpu().numpy())
        out.update({n: planes[n].cpu().numpy() for n in PLANES})
    return out


def _same_frame(got, ref, what, planes=PLANES):
    for n in ("img",) + tuple(planes):
        bad = int((np.asarray(got[n]) != ref[n]).reshape(ref[n].shape[0], ref[n].shape[1], -1).any(axis=-1).sum())
        assert bad == 0, "%s: %s differs from the oracle in %d pixels" % (what, n, bad)


def _normals(v):
    n = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    ln[ln == 0] = 1.0
    return (n / ln).astype(np.float32)


def _deformed(rest, step, amp):
    """the mesh `rest` [n, 18] bent by a travelling wave and stretched (same triangles, same order); unit normals of the new
    vertices (both sides take the normals they are given)"""
    m = rest.copy()
    v = m[:, :9].reshape(-1, 3, 3)
    v[..., 2] += np.float32(amp * step) * np.sin(3.0 * v[..., 0] + step).astype(np.float32)
    v[..., 1] *= np.float32(1.0 + 0.05 * step)
    m[:, 9:12] = _normals(v)
    return m


def _host_arrays(tris):
    return np.ascontiguousarray(tris[:, :9]), np.ascontiguousarray(tris[:, 9:12])


def _records(sp):
    return [sp.debug_read(k, np.uint8) for k in range(5)]


# ---------------------------------------------------------------------------------------------------------------------------
def test_host_array_refits_on_two_streams(rt, orc, scenes, atrium, blob5k, blob70k):
    """rt_scene_refit_mesh stages the caller's vertices in one per-scene buffer.  Two host-array refits of two meshes of ONE scene
    on two streams -- from one thread (the C-ABI form) or from two -- must not fold one mesh's vertices into the other's boxes:
    after every round the scene's arrays equal those of the same refits done one after the other, and the frame equals the
    oracle's after both refits.  The large mesh (the 260 k-triangle atrium: many level launches) is stretched by a render batch
    of another scene that keeps the CUs busy; the staging buffer is at its full size before the first round, so no synchronising
    re-allocation hides a race."""
    import torch
    import orc as orc_mod
    o = orc_mod.oracle()
    h = rt.libs()[0]
    W, H = 320, 180
    K, D, pose = scenes.scaled_K(W), scenes.D_REF, scenes.C4["cam_pose"]
    tex = sd.checker_texture(64, 48, seed=21)
    meshes = [rt.Mesh.load_obj(atrium), rt.Mesh.load_obj(blob5k), rt.Mesh.from_triangles(sd.random_triangles(300, seed=11, spread=0.8, size=0.3))]
    rest = [m.dump()["tris"].copy() for m in meshes]
    inst = [(0, 0, (0,) * 6, (1, 1, 1)), (1, 1, (0.3, -5.2, 1.5, 0.3, 0.2, 0.1), (0.7, 0.7, 0.7)),
            (2, 2, (-0.6, -5.6, 1.9, -0.2, 0.4, 0.0), (0.5, 0.6, 0.5))]
    mats = [((0.8, 0.8, 0.7), tex), ((0.9, 0.5, 0.2), None), ((0.2, 0.7, 0.4), None)]
    sp = rt.Scene()
    so = orc_mod.OracleScene(o)
    om = [o.mesh_from_triangles(r) for r in rest]
    for albedo, t in mats:
        sp.add_material(albedo, texture_bgr=t)
        so.add_material(albedo, t)
    for m, q in zip(meshes, om):
        sp.add_mesh(m)
        so.add_mesh(q)
    for mi, mat, p, s in inst:
        sp.add_mesh_instance(mi, mat, p, s)
        so.add_instance(mi, mat, p, s)
    sp.upload_to_device()
    handle = sp.device_handle
    cam = rt.Camera(W, H, K, D)
    cam.set_pose(pose)
    # shapes: 0 = rest, 1 and 2 = deformed (the small soup is refitted from DEVICE arrays, rt_scene_refit_mesh_device)
    shapes = [[r] + [_deformed(r, k, amp) for k in (1, 2)] for r, amp in zip(rest, (0.08, 0.15, 0.2))]
    host = [[_host_arrays(t) for t in per] for per in shapes]
    dev = [tuple(torch.from_numpy(a).cuda() for a in host[2][k]) for k in range(3)]
    torch.cuda.synchronize()

    def refit_host(mesh, k, stream):
        v, n = host[mesh][k]
        rt.check(h.rt_scene_refit_mesh(handle, mesh, v.ctypes.data_as(_f), n.ctypes.data_as(_f), len(v), stream), "rt_scene_refit_mesh")

    def refit_dev(k, stream):
        v, n = dev[k]
        rt.check(h.rt_scene_refit_mesh_device(handle, 2, v.data_ptr(), n.data_ptr(), v.shape[0], stream), "rt_scene_refit_mesh_device")

    # (atrium, blob, soup) shape of every round
    states = [(1, 1, 0), (2, 2, 0), (0, 0, 1), (1, 2, 1), (2, 1, 1)]
    want = []
    for a, b, c in states:                                      # the same refits one after the other (this also sizes the staging buffer)
        refit_host(0, a, None)
        rt.check(h.rt_device_synchronize())
        refit_host(1, b, None)
        rt.check(h.rt_device_synchronize())
        refit_dev(c, None)
        rt.check(h.rt_device_synchronize())
        want.append(_records(sp))
    refit_host(0, 0, None)
    refit_host(1, 0, None)
    refit_dev(0, None)
    rt.check(h.rt_device_synchronize())

    # the busy work: a batch of another scene on a third stream
    busy_scene = sd.blob_scene(scenes, blob70k).build_product(rt)
    busy_scene.upload_to_device()
    BW, BH, NB = 1920, 1080, 16
    busy_scene.reserve_views(NB)                                # (no pool growth, which drains the device, inside a round)
    busy_cam = rt.Camera(BW, BH, scenes.scaled_K(BW), D)
    base = scenes.C2_CAMERAS["mid"]
    busy_cams = (rt.RtCameraParams * NB)(*[_params(rt, busy_cam, (base[0] + 0.002 * i,) + tuple(base[1:])) for i in range(NB)])
    busy_img = torch.empty((NB, BH, BW * 3), dtype=torch.uint8, device="cuda")
    busy_ptrs = (C.c_void_p * NB)(*[busy_img[i].data_ptr() for i in range(NB)])
    render_batch = _render_batch_fn(rt)
    s1, s2, s3 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()

    for r, (a, b, c) in enumerate(states):
        rt.check(render_batch(busy_scene.device_handle, busy_cams, busy_ptrs, BW * 3, NB, s3.cuda_stream, 0), "rt_render_batch")
        if r == 1:                                              # the small mesh first
            refit_host(1, b, s2.cuda_stream)
            refit_host(0, a, s1.cuda_stream)
        elif r == 2:                                            # a device-array refit of a third mesh on the third stream in between
            refit_host(0, a, s1.cuda_stream)
            refit_dev(c, s3.cuda_stream)
            refit_host(1, b, s2.cuda_stream)
        elif r >= 3:                                            # two threads, one refit each (Scene::refit_mesh's shape)
            th = _Threads()
            go = th.barrier(2)

            def one(mesh, k, stream):
                go.wait()
                refit_host(mesh, k, stream)
            th.start("refit-atrium", one, 0, a, s1.cuda_stream)
            th.start("refit-blob", one, 1, b, s2.cuda_stream)
            th.join()
        else:
            refit_host(0, a, s1.cuda_stream)
            refit_host(1, b, s2.cuda_stream)
        rt.check(h.rt_device_synchronize())                     # (the host arrays live in `host` until here and beyond)
        got = _records(sp)
        for kind in range(5):
            if not np.array_equal(got[kind], want[r][kind]):
                diff = np.flatnonzero(got[kind] != want[r][kind])
                raise AssertionError("round %d: rt_scene_debug_read(%d) differs from the serial refits in %d bytes, first at %d"
                                     % (r, kind, diff.size, diff[0]))
        for mesh, k in enumerate((a, b, c)):
            o.mesh_refit(om[mesh], shapes[mesh][k])
        ref = so.render(W, H, K, D, pose, threads=16)
        _same_frame(rt.render_debug(sp, cam), ref, "round %d" % r)
        if r == 0:
            seen = set(np.unique(ref["hit_inst"]).tolist())
            assert {0, 1, 2} <= seen, seen                      # every mesh is in the frame
    so.close()


# ---------------------------------------------------------------------------------------------------------------------------
def test_four_threads_on_one_scene(rt, orc, scenes, blob5k):
    """Four threads on one multi-instance, textured scene whose view pool is NOT reserved (it grows under contention), through four
    phases that alternate two known states (S0: as uploaded; S1: an instance moved with rt_scene_update_instance_async and a mesh
    refitted from host arrays, both on a mutator stream).  T1 / T2: rt_render_batch of 4 / 8 frames (T2's first batch grows the pool
    while T1's frames are in flight); T3: pairs of rt_render_overlapped frames, each pair followed by rt_device_synchronize (a
    device-wide wait from one thread while others hold the scene's lock); T4: Scene.trace_rays (all outputs, binned) and
    Scene.occluded with per-ray bounds.  Between phases the application orders the state change after every worker's last call
    (events), and every worker's next call after the change.  Every frame and query result equals the oracle of its phase's state;
    the view and overlap statistics account for every launch exactly."""
    import torch
    import orc as orc_mod
    desc = sd.multi_instance_scene(scenes, blob5k)
    m = sd.MULTI_CAMERA
    W, H, K, D = m["width"], m["height"], scenes.scaled_K(m["width"]), scenes.D_REF
    so = desc.build_oracle(orc)
    sp = desc.build_product(rt)
    sp.upload_to_device()
    h = rt.libs()[0]
    handle = sp.device_handle
    o = orc_mod.oracle()
    render_batch = _render_batch_fn(rt)
    base = m["pose"]
    poses = [(base[0] + 0.02 * (k % 5) - 0.04, base[1] + 0.05 * (k // 5), base[2] + 0.01 * k, base[3], base[4] + 0.004 * k, base[5])
             for k in range(14)]
    T1, T2, T3 = list(range(0, 4)), list(range(4, 12)), [12, 13]
    # S1: instance 2 moved and turned, mesh 1 (the soup) deformed
    rest1 = desc.product_meshes[1].dump()["tris"].copy()
    moved1 = _deformed(rest1, 2, 0.15)
    arrays = {0: _host_arrays(rest1), 1: _host_arrays(moved1)}
    inst2 = {0: desc.instances[2][2:], 1: ((0.7, 0.9, 0.9, 0.3, -0.2, 0.5), (0.6, 0.5, 0.7))}
    # the ray set of T4: random origins and directions around the scene, per-ray bounds for the occlusion query
    rng = np.random.default_rng(77)
    nr = 40000
    ro = rng.uniform(-2.5, 2.5, (nr, 3)).astype(np.float32)
    rd = rng.normal(size=(nr, 3)).astype(np.float32)
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    tmax = rng.uniform(0.0, 4.0, nr).astype(np.float32)
    # the oracle of both states
    frames, rays = {}, {}
    for state in (0, 1):
        if state == 1:
            so.update_instance(2, 0, 2, *inst2[1])
            o.mesh_refit(desc.oracle_meshes[1], moved1)
        frames[state] = [so.render(W, H, K, D, p, threads=16, planes=False)["img"] for p in poses]
        ref = ray_oracle.cast_rays(so, ro, rd, threads=16)
        ref["occluded"] = ray_oracle.cast_rays(so, ro, rd, lighting_pass=1, tmax=tmax, threads=16)["occluded"]
        rays[state] = ref
    so.close()
    assert any(not np.array_equal(frames[0][k], frames[1][k]) for k in range(len(poses)))
    assert not np.array_equal(rays[0]["t"], rays[1]["t"])

    phases = [0, 1, 0, 1]
    streams = {w: torch.cuda.Stream() for w in ("T1", "T2", "T4")}
    mut = torch.cuda.Stream()
    img = {w: torch.full((len(phases), len(ks), H, W * 3), 0xCD, dtype=torch.uint8, device="cuda") for w, ks in (("T1", T1), ("T2", T2))}
    img["T3"] = torch.full((len(phases), 2, 2, H, W * 3), 0xCD, dtype=torch.uint8, device="cuda")
    d_ro, d_rd, d_tm = (torch.from_numpy(a).cuda() for a in (ro, rd, tmax))
    torch.cuda.synchronize()
    view0, over0 = sp.view_stats(), sp.overlap_stats()
    assert view0["launches"] == 0 and view0["grows"] == 0 and view0["slot_frames"] == 0

    th = _Threads()
    end_phase, next_phase = th.barrier(5), th.barrier(5)
    done = {w: [torch.cuda.Event() for _ in phases] for w in streams}
    ready = [torch.cuda.Event() for _ in phases]
    t1_issued = threading.Event()
    results = {}

    def batch_worker(name, ks):
        s = streams[name]
        cam = rt.Camera(W, H, K, D)
        cams = (rt.RtCameraParams * len(ks))(*[_params(rt, cam, poses[k]) for k in ks])
        for ph in range(len(phases)):
            if ph == 0 and name == "T2":
                assert t1_issued.wait(DEADLINE), "T1 never issued its first batch"
            ptrs = (C.c_void_p * len(ks))(*[img[name][ph, i].data_ptr() for i in range(len(ks))])
            rt.check(render_batch(handle, cams, ptrs, W * 3, len(ks), s.cuda_stream, 0), "rt_render_batch (%s)" % name)
            if name == "T1":
                t1_issued.set()
            done[name][ph].record(s)
            end_phase.wait()
            next_phase.wait()
            s.wait_event(ready[ph])

    def overlapped_worker():
        cam = rt.Camera(W, H, K, D)
        cams = [_params(rt, cam, poses[k]) for k in T3]
        for ph in range(len(phases)):
            for pair in range(2):
                for i in range(2):
                    rt.check(h.rt_render_overlapped(handle, C.byref(cams[i]), img["T3"][ph, pair, i].data_ptr(), W * 3), "rt_render_overlapped")
                rt.check(h.rt_device_synchronize(), "rt_device_synchronize")
            end_phase.wait()
            next_phase.wait()
            ready[ph].synchronize()                             # (its frames go to the scene's own streams, which no torch event orders)

    def query_worker():
        s = streams["T4"]
        with torch.cuda.stream(s):
            for ph in range(len(phases)):
                hits = sp.trace_rays(d_ro, d_rd, outputs=RAY_OUTPUTS, stream=s, binning=True)
                occ = sp.occluded(d_ro, d_rd, d_tm, stream=s, binning=True)
                results[ph] = (hits, occ)
                done["T4"][ph].record(s)
                end_phase.wait()
                next_phase.wait()
                s.wait_event(ready[ph])

    th.start("T1", batch_worker, "T1", T1)
    th.start("T2", batch_worker, "T2", T2)
    th.start("T3", overlapped_worker)
    th.start("T4", query_worker)
    try:
        for ph in range(len(phases)):
            end_phase.wait()
            for w in streams:
                mut.wait_event(done[w][ph])
            if ph + 1 < len(phases) and phases[ph + 1] != phases[ph]:
                to = phases[ph + 1]
                sp.update_mesh_instance(2, 0, 2, *inst2[to], stream=mut.cuda_stream)
                v, n = arrays[to]
                rt.check(h.rt_scene_refit_mesh(handle, 1, v.ctypes.data_as(_f), n.ctypes.data_as(_f), len(v), mut.cuda_stream), "rt_scene_refit_mesh")
            ready[ph].record(mut)
            next_phase.wait()
    except threading.BrokenBarrierError:
        pass                                                    # (a worker failed: join says which and why)
    th.join()
    torch.cuda.synchronize()

    for ph, state in enumerate(phases):
        for name, ks in (("T1", T1), ("T2", T2)):
            for i, k in enumerate(ks):
                got = img[name][ph, i].cpu().numpy().reshape(H, W, 3)
                _same_frame(dict(img=got), dict(img=frames[state][k]), "phase %d %s frame %d" % (ph, name, i), planes=())
        for pair in range(2):
            for i, k in enumerate(T3):
                got = img["T3"][ph, pair, i].cpu().numpy().reshape(H, W, 3)
                _same_frame(dict(img=got), dict(img=frames[state][k]), "phase %d T3 pair %d frame %d" % (ph, pair, i), planes=())
        hits, occ = results[ph]
        for k in RAY_OUTPUTS:
            g, r = hits[k].cpu().numpy(), rays[state][k]
            bad = int((g.view(np.uint32) != r.view(np.uint32)).reshape(nr, -1).any(axis=1).sum()) if g.dtype == np.float32 else int((g != r).reshape(nr, -1).any(axis=1).sum())
            assert bad == 0, "phase %d trace_rays %s: %d rays differ from the oracle" % (ph, k, bad)
        assert np.array_equal(occ.cpu().numpy(), rays[state]["occluded"]), "phase %d occluded" % ph
    view, over = sp.view_stats(), sp.overlap_stats()
    issued = 2 * len(phases)                                    # T1's and T2's batches; single overlapped frames never take views
    assert view["launches"] - view0["launches"] == issued, view
    assert view["grows"] == 2 and view["slot_frames"] == 8, view      # 4 frames per slot (T1's first batch), then 8 (T2's)
    assert view["fallbacks"] <= view["launches"], view
    assert over[0] - over0[0] == 4 * len(phases), over


# ---------------------------------------------------------------------------------------------------------------------------
def test_more_streams_than_tile_order_slots(rt, orc, scenes, blob5k):
    """Single frames of half a million pixels and more are dispatched heavy tiles first (launch_ordered, tile_sort_kernel): one order
    state per frame size, which tracks the last launch of four streams.  Six threads on six streams render single frames of the SAME
    size (some launches run unordered, sorts run beside them), two of them also frames of a second size (two order states at once).
    Concurrent cost updates and sorts may change the order of work only: every frame equals the oracle's (a lost tile would keep
    the buffer's fill pattern, a tile rendered from a torn order would show too)."""
    import torch
    desc = sd.blob_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    sp = desc.build_product(rt)
    sp.upload_to_device()
    h = rt.libs()[0]
    handle = sp.device_handle
    D = scenes.D_REF
    base = scenes.C2_CAMERAS["mid"]
    sizes = [(1024, 512), (1280, 720)]                         # 8192 and 14400 tiles of 8x8 pixels: both take the ordered path
    poses = [(base[0] + 0.03 * k, base[1] - 0.05 * k, base[2] - 0.02 * k, 0.02 * k, 0.0, -0.01 * k) for k in range(4)]
    plan = {t: [(0, (t + k) % 4) for k in range(6)] for t in range(6)}
    for t in (0, 1):
        plan[t] = [x for k in range(6) for x in ((0, (t + k) % 4), (1, (t + k) % 2))]
    want = {(si, k): so.render(sizes[si][0], sizes[si][1], scenes.scaled_K(sizes[si][0]), D, poses[k], threads=16, planes=False)["img"]
            for si in (0, 1) for k in range(4) if si == 0 or k < 2}
    so.close()
    bufs = {t: [torch.full((sizes[si][1], sizes[si][0] * 3), 0xCD, dtype=torch.uint8, device="cuda") for si, _ in plan[t]] for t in plan}
    streams = {t: torch.cuda.Stream() for t in plan}
    torch.cuda.synchronize()
    th = _Threads()
    go = th.barrier(len(plan))

    def worker(t):
        cams = [rt.Camera(w, hh, scenes.scaled_K(w), D) for w, hh in sizes]
        params = [(si, _params(rt, cams[si], poses[k])) for si, k in plan[t]]
        go.wait()
        for (si, p), b in zip(params, bufs[t]):
            rt.check(h.rt_render(handle, C.byref(p), b.data_ptr(), sizes[si][0] * 3, streams[t].cuda_stream, 0), "rt_render")
        streams[t].synchronize()

    for t in plan:
        th.start("stream-%d" % t, worker, t)
    th.join()
    torch.cuda.synchronize()
    for t in plan:
        for i, ((si, k), b) in enumerate(zip(plan[t], bufs[t])):
            w, hh = sizes[si]
            _same_frame(dict(img=b.cpu().numpy().reshape(hh, w, 3)), dict(img=want[(si, k)]), "thread %d frame %d (%dx%d)" % (t, i, w, hh), planes=())


# ---------------------------------------------------------------------------------------------------------------------------
def _same_tree(a, b):
    assert np.array_equal(a["child"], b["child"]) and np.array_equal(a["leaf_count"], b["leaf_count"])
    assert np.array_equal(a["leaf_idx"], b["leaf_idx"])
    assert np.array_equal(a["boxes"], b["boxes"])
    assert np.array_equal(a["tris"].view(np.uint32), b["tris"].view(np.uint32))


def test_rebuild_on_one_thread_while_another_renders_another_scene(rt, orc, scenes, blob5k):
    """The BVH build arena is one per process (rt_bvh_build.hip): a device-resident rebuild (rt_scene_rebuild_mesh_device) of scene X
    on one thread, GPU builds of new meshes (rt_bvh_build) on a second and renders of scene Y on a third, all at once.  X's frame
    after every rebuild equals the oracle's for those triangles, the GPU-built trees equal the host builder's node for node, and Y's
    frames stay what they were."""
    import torch
    import orc as orc_mod
    o = orc_mod.oracle()
    h = rt.libs()[0]
    W, H = 320, 180
    K, D, pose = scenes.scaled_K(W), scenes.D_REF, scenes.C2_CAMERAS["mid"]
    rest = rt.Mesh.load_obj(blob5k).dump()["tris"].copy()
    rng = np.random.default_rng(5)
    shapes = []
    for k in range(1, 5):                                       # new triangles, new trees: bent, shuffled, some dropped
        s = _deformed(rest, k, 0.3)
        s = s[rng.permutation(len(s))[: len(s) - 500 * k]]
        shapes.append(np.ascontiguousarray(s))
    shapes.append(rest)
    xd = sd.SceneDesc([((0.9, 0.5, 0.2), None)], [("tris", rest)], [(0, 0, (0.0, 0.0, 0.0, 0.1, 0.0, 0.2), (1.0, 0.9, 1.1))])
    sx = xd.build_product(rt)
    sx.upload_to_device()
    x_ref = []
    for s in shapes:
        so = sd.SceneDesc(xd.materials, [("tris", s)], xd.instances).build_oracle(orc)
        x_ref.append(so.render(W, H, K, D, pose, threads=16))
        so.close()
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (s[:, :9], s[:, 9:12], s[:, 12:18])) for s in shapes]
    yd = sd.multi_instance_scene(scenes, blob5k)
    sy = yd.build_product(rt)
    sy.upload_to_device()
    m = sd.MULTI_CAMERA
    so = yd.build_oracle(orc)
    y_ref = so.render(m["width"], m["height"], scenes.scaled_K(m["width"]), D, m["pose"], threads=16, planes=False)["img"]
    so.close()
    soups = [sd.random_triangles(n, seed=40 + n % 7, spread=1.0, size=0.2) for n in (1500, 3000, 700)]
    soups.append(_deformed(rest, 3, 0.2))
    host_trees = [rt.Mesh.from_triangles(t).dump() for t in soups]
    s1, s3 = torch.cuda.Stream(), torch.cuda.Stream()
    YN = 12
    y_imgs = torch.full((YN, m["height"], m["width"] * 3), 0xCD, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    th = _Threads()
    go = th.barrier(3)
    x_got, trees = [], []

    def rebuilder():
        cam = rt.Camera(W, H, K, D)
        p = _params(rt, cam, pose)
        go.wait()
        for k, (v, n, uv) in enumerate(dev):
            rt.check(h.rt_scene_rebuild_mesh_device(sx.device_handle, 0, v.data_ptr(), n.data_ptr(), uv.data_ptr(), v.shape[0], s1.cuda_stream),
                     "rt_scene_rebuild_mesh_device %d" % k)
            x_got.append(_debug_frame(rt, sx.device_handle, p, s1, W, H))

    def builder():
        go.wait()
        for t in soups:
            trees.append(rt.Mesh.from_triangles(t, gpu_build=True).dump())

    def renderer():
        cam = rt.Camera(m["width"], m["height"], scenes.scaled_K(m["width"]), D)
        p = _params(rt, cam, m["pose"])
        go.wait()
        for i in range(YN):
            rt.check(h.rt_render(sy.device_handle, C.byref(p), y_imgs[i].data_ptr(), m["width"] * 3, s3.cuda_stream, 0), "rt_render")
            if i % 3 == 2:
                s3.synchronize()
        s3.synchronize()

    th.start("rebuild-X", rebuilder)
    th.start("gpu-build", builder)
    th.start("render-Y", renderer)
    th.join()
    torch.cuda.synchronize()
    assert len(x_got) == len(shapes) and len(trees) == len(soups)
    for k, (got, ref) in enumerate(zip(x_got, x_ref)):
        _same_frame(got, ref, "scene X after rebuild %d" % k)
    assert not np.array_equal(x_ref[0]["img"], x_ref[-1]["img"])
    for k, (a, b) in enumerate(zip(trees, host_trees)):
        _same_tree(a, b)
    for i in range(YN):
        _same_frame(dict(img=y_imgs[i].cpu().numpy().reshape(m["height"], m["width"], 3)), dict(img=y_ref), "scene Y frame %d" % i, planes=())
