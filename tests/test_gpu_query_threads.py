"""Every query family (rays, points, crossings, nearby lists, triangle intersections, boxes, plane sections, regions, segments, triangle
distances) on ONE scene from ten host threads at once, beside renders, instance updates, refits and a device-resident rebuild ("Threads"): the entry points share scene_launch, which takes the scene's call lock for the launches of
one call (two nested calls for rt_signed_distance, a count launch and the scan's launches for the *_offsets calls, the distance launch
and the crossing or intersection launch of rt_closest_to_segments and rt_closest_to_triangles) and leaves it before any wait.  test_gpu_threads.test_four_threads_on_one_scene, whose phase scheme and helpers this reuses, predates the families and
queries with rt_trace_rays and rt_occluded only.  Every result of every call is compared bit for bit with the CPU shims' result for the
scene state of its phase, never with another GPU run.  Nothing retries; a thread still alive after its deadline fails the test."""
import ctypes as C
import threading

import numpy as np
import pytest

import box_oracle as bo
import crossing_list_oracle as xl
import crossing_oracle as xo
import nearby_oracle as nb
import point_oracle
import query_points as qp
import query_rays as qr
import query_segments as qsg
import query_triangles as qtr
import region_oracle as ro
import scene_defs as sd
import section_oracle as sc
import segment_oracle as sg
import tri_intersect_oracle as ti
import triangle_distance_oracle as tdo
from test_gpu_boxes import families as box_families
from test_gpu_crossings import _cam, _eq
from test_gpu_regions import families as region_families
from test_gpu_sections import families as section_families
from test_gpu_threads import _Threads, _deformed, _host_arrays, _params, _render_batch_fn, _same_frame
from test_gpu_tri_intersect import families as tri_families

pytestmark = pytest.mark.gpu
F32 = np.float32
_f = C.POINTER(C.c_float)
POINT_FIELDS = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")
XL_FIELDS = ("t", "instance", "triangle", "sign", "barycentric", "uv", "point")
TI_FIELDS = ("instance", "triangle", "normal", "segment")
BX_FIELDS = ("instance", "triangle")
SC_FIELDS = ("instance", "triangle", "segment", "normal")
RG_FIELDS = ("instance", "triangle", "inside", "normal")
GRID_DIMS = (5, 3, 2)
WORKERS = ("W1", "W2", "W3", "W4", "W5", "W6", "W7", "W8", "W9", "W10")


def _oracle_results(so, q, frames_of):
    """Everything the workers ask, from the shims, for the oracle scene's current state: name -> dict or array"""
    o, d, tmax, pts, md, radius, tris, skip = (q[k] for k in ("o", "d", "tmax", "pts", "md", "radius", "tris", "skip"))
    boxes, (origin, spacing), planes = q["boxes"], q["grid"], q["planes"]
    regions, segs, seg_md, qtris, qtri_md, qtri_skip = (q[k] for k in ("regions", "segs", "seg_md", "qtris", "qtri_md", "qtri_skip"))
    return {
        "closest": point_oracle.closest_points(so, pts),
        "closest_md": point_oracle.closest_points(so, pts, md),
        "sdf": xo.signed_distance(so, pts, md),
        "crossings": xo.count_crossings(so, o, d),
        "crossings_tmax": xo.count_crossings(so, o, d, tmax),
        "winding": xo.winding_numbers(so, pts),
        "xl_csr": xl.list_crossings(so, o, d),
        "xl_k3": xl.list_crossings(so, o, d, max_hits=3),
        "xl_k1": xl.list_crossings(so, o, d, max_hits=1),
        "nb_csr": nb.list_nearby(so, pts, radius),
        "nb_k4": nb.list_nearby(so, pts, radius, max_hits=4),
        "nb_k4_unbounded": nb.list_nearby(so, pts, None, max_hits=4),
        "ti_count": ti.count_intersecting(so, tris, skip),
        "ti_csr": ti.list_intersecting(so, tris, skip),
        "ti_k2": ti.list_intersecting(so, tris, skip, max_hits=2),
        "bx_count": bo.count_in_boxes(so, boxes),
        "bx_csr": bo.list_in_boxes(so, boxes),
        "bx_k4": bo.list_in_boxes(so, boxes, max_hits=4),
        "bx_grid": bo.count_in_boxes(so, bo.grid_boxes(origin, spacing, GRID_DIMS)).reshape(GRID_DIMS[::-1]),
        "sc_count": sc.count_sections(so, planes),
        "sc_csr": sc.list_sections(so, planes),
        "sc_k4": sc.list_sections(so, planes, max_hits=4),
        "rg_count": ro.count_in_regions(so, regions)["count"],
        "rg_csr": ro.list_in_regions(so, regions),
        "rg_k4": ro.list_in_regions(so, regions, max_hits=4),
        "sg_md": sg.closest_to_segments(so, segs, seg_md),
        "td_md_skip": tdo.closest_to_triangles(so, qtris, qtri_md, qtri_skip),
        "frames": frames_of(so),
    }


def _np(v):
    return v if isinstance(v, np.ndarray) else v.cpu().numpy()


def _same(got, ref, keys, where):
    for k in keys:
        _eq(_np(got[k]), ref[k], "%s %s" % (where, k))


def test_ten_query_threads_on_one_scene(rt, orc, scenes, blob5k):
    """Ten workers, each on its own torch stream with at least three calls per phase, and a mutator, through five phases that alternate
    two known states (S0: as uploaded; S1: instance 2 moved with rt_scene_update_instance_async and mesh 1 refitted from host arrays,
    both on the mutator's stream; the last change back to S0 is rt_scene_rebuild_mesh_device of the refitted mesh to its rest shape).
    W1: closest_points with every output, signed_distance (a nested call under one hold of the lock), closest_points bounded.
    W2: count_crossings, rt_render_batch of 4 frames (the view pool grows under contention), winding_numbers, count_crossings with tmax.
    W3: list_crossings CSR, max_hits = 3, max_hits = 1 without the key fields (the selection path).
    W4: list_nearby CSR with a radius per point, max_hits = 4 with it, max_hits = 4 unbounded with count.
    W5: count_intersecting and list_intersecting CSR and max_hits = 2, all with a skip_instance column.
    W6: W3's rays through the numpy path (synchronous, its own device buffers and workspace): list_crossings CSR, count_crossings, CSR
    again -- two CSR calls of one family in flight on one scene.
    W7: count_in_boxes for `any` alone (the kernel that stops at the first pair), list_in_boxes CSR (a count launch, the scan and the
    fill, whose rooms are heaps), max_hits = 4 without count (rooms that end the traversal early), occupancy_grid with both outputs
    on a (5, 3, 2) grid over the scene's box in S0.
    W8: count_sections for `any` alone (the kernel that stops at the first pair), list_sections CSR with all four fields (a count
    launch and the scan under one hold of the lock, then the fill, whose rooms are heaps that carry each pair's record slot),
    max_hits = 4 with the normal alone and without count (the slot travels in the normal, the rooms end the traversal early).
    W9: count_in_regions on K = 6 regions for `any` alone (the kernel that stops at the first pair), list_in_regions CSR with all four
    fields (a count launch and the scan under one hold of the lock, then the fill, whose rooms are heaps that carry each pair's inside
    flag and record slot), max_hits = 4 with the normal alone and without count (the slot travels in the normal, the rooms end the
    traversal early), max_hits = 4 with the inside flag alone.
    W10: the calls of two launches under one hold of the lock, which must see one scene state: closest_to_segments with every exact
    output, crossings, clearance and within among them, with a max_distance column (the distance launch, then the crossing launch
    that patches clearance and within); closest_to_triangles with a max_distance and a skip_instance column and every exact output,
    intersections, clearance and within among them; closest_to_segments for `within` alone (the kernel that ends at the first
    triangle in reach).
    Between phases the state change is ordered after every worker's last call and before every worker's next by events.  Every
    result of every call equals the shims' for its phase's state, every frame the oracle's, and no call fails."""
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
    o_ = orc_mod.oracle()
    render_batch = _render_batch_fn(rt)
    base = m["pose"]
    poses = [(base[0] + 0.02 * k - 0.04, base[1] + 0.05 * k, base[2] + 0.01 * k, base[3], base[4] + 0.004 * k, base[5]) for k in range(4)]
    # S1: instance 2 moved and turned, mesh 1 (the soup) deformed (test_four_threads_on_one_scene's states)
    rest1 = desc.product_meshes[1].dump()["tris"].copy()
    moved1 = _deformed(rest1, 2, 0.15)
    arrays = {0: _host_arrays(rest1), 1: _host_arrays(moved1)}
    inst2 = {0: desc.instances[2][2:], 1: ((0.7, 0.9, 0.9, 0.3, -0.2, 0.5), (0.6, 0.5, 0.7))}

    # the queries, drawn once in S0
    rng = np.random.default_rng(79)
    cam = _cam(scenes, 32, 18, base)
    o, d = qr.flatten(qr.families(rng, so, cam, n=340))
    pts = qp.flatten(qp.families(rng, o_, desc, so, cam, n=260))
    tris = np.ascontiguousarray(np.concatenate([f[1] for f in tri_families(rng, o_, desc, n=400)]), F32)
    # (a generator of their own: the draws below stay what they were before the boxes came)
    boxes = np.ascontiguousarray(np.concatenate([f[1] for f in box_families(np.random.default_rng(83), o_, desc, n=600)]), F32)
    planes = np.ascontiguousarray(np.concatenate([f[1] for f in section_families(np.random.default_rng(89), o_, desc, n=600)]), F32)
    regions = np.ascontiguousarray(np.concatenate([f[1] for f in region_families(rt, np.random.default_rng(97), o_, desc, n=800)[6]]), F32)
    segs = qsg.flatten(qsg.families(np.random.default_rng(101), o_, desc, so, cam, n=2600)[0])
    qtris = qtr.flatten(qtr.families(np.random.default_rng(103), o_, desc, so, cam, n=1300)[0])
    for name, a in (("rays", o), ("points", pts), ("triangles", tris), ("boxes", boxes), ("planes", planes), ("regions", regions),
                    ("segments", segs)):
        assert 2000 <= len(a) <= 4000, (name, len(a))
    assert 1000 <= len(qtris) <= 2000, len(qtris)               # (the shim of the triangle distances is the slowest of the set-up)
    assert regions.shape[1:] == (6, 2, 3)
    rng2 = np.random.default_rng(107)                           # (the new families' bounds: the draws below stay what they were)
    seg_md = qp.special_bounds(rng2, sg.closest_to_segments(so, segs)["distance"])
    qtri_md = qp.special_bounds(rng2, tdo.closest_to_triangles(so, qtris)["distance"])
    qtri_skip = rng2.integers(-1, len(desc.instances), len(qtris)).astype(np.int32)
    dist = point_oracle.closest_points(so, pts)["distance"]
    lo, hi = qp.scene_box(o_, desc, desc.oracle_meshes)
    diag = F32(np.linalg.norm((hi - lo).astype(np.float64)))
    assert (boxes[:, 0] <= lo).all(axis=1).any() and (boxes[:, 1] >= hi).all(axis=1).any()     # (the whole scene is among the boxes)
    span = np.maximum(hi - lo, F32(1e-3)).astype(F32)
    grid = ((lo - F32(0.05) * span).astype(F32), (F32(1.1) * span / np.asarray(GRID_DIMS, F32)).astype(F32))
    # radii: up to 1.5 times the closest distance; a point farther off than a tenth of the scene's diagonal reaches its closest
    # triangle alone (a multiple of its distance would list most of the scene for that point)
    near = (dist * rng.uniform(1.0, 1.5, len(pts)) + diag * F32(1e-3)).astype(F32)
    q = dict(o=o, d=d, tmax=qr.special_tmax(rng, len(o)), pts=pts, md=qp.special_bounds(rng, dist),
             radius=np.ascontiguousarray(np.where(dist > F32(0.1) * diag, np.nextafter(dist, F32(np.inf)), near), F32), tris=tris,
             skip=rng.integers(-1, len(desc.instances), len(tris)).astype(np.int32), boxes=boxes, grid=grid, planes=planes,
             regions=regions, segs=segs, seg_md=seg_md, qtris=qtris, qtri_md=qtri_md, qtri_skip=qtri_skip)

    def frames_of(scene):
        return [scene.render(W, H, K, D, p, threads=16, planes=False)["img"] for p in poses]
    want = {0: _oracle_results(so, q, frames_of)}
    so.update_instance(2, 0, 2, *inst2[1])
    o_.mesh_refit(desc.oracle_meshes[1], moved1)
    want[1] = _oracle_results(so, q, frames_of)
    so.close()
    for name, key in (("closest", "distance"), ("xl_csr", "offsets"), ("nb_csr", "offsets"), ("ti_csr", "offsets"),
                      ("bx_csr", "offsets"), ("sc_csr", "offsets"), ("rg_csr", "offsets"), ("sg_md", "distance")):
        assert not np.array_equal(want[0][name][key], want[1][name][key]), name + ": the two states give one result"
    assert any(not np.array_equal(a, b) for a, b in zip(want[0]["frames"], want[1]["frames"]))

    phases = [0, 1, 0, 1, 0]
    streams = {w: torch.cuda.Stream() for w in WORKERS if w != "W6"}
    mut = torch.cuda.Stream()
    dq = {k: torch.from_numpy(v).cuda() for k, v in q.items() if k != "grid"}
    img = torch.full((len(phases), len(poses), H, W * 3), 0xCD, dtype=torch.uint8, device="cuda")
    rest_dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rest1[:, :9], rest1[:, 9:12], rest1[:, 12:18]))
    torch.cuda.synchronize()

    th = _Threads()
    end_phase, next_phase = th.barrier(len(WORKERS) + 1), th.barrier(len(WORKERS) + 1)
    done = {w: [torch.cuda.Event() for _ in phases] for w in streams}
    ready = [torch.cuda.Event() for _ in phases]
    results = {w: {} for w in WORKERS}

    def worker(name, calls):
        """calls(stream) -> the phase's results; then the phase protocol of test_four_threads_on_one_scene"""
        s = streams[name]
        with torch.cuda.stream(s):
            for ph in range(len(phases)):
                results[name][ph] = calls(s, ph)
                done[name][ph].record(s)
                end_phase.wait()
                next_phase.wait()
                s.wait_event(ready[ph])

    def w1(s, ph):
        return dict(closest=sp.closest_points(dq["pts"], outputs=POINT_FIELDS + ("pops",), stream=s),
                    sdf=sp.signed_distance(dq["pts"], dq["md"], stream=s),
                    closest_md=sp.closest_points(dq["pts"], dq["md"], outputs=POINT_FIELDS, stream=s))

    cam_obj = rt.Camera(W, H, K, D)
    cams = (rt.RtCameraParams * len(poses))(*[_params(rt, cam_obj, p) for p in poses])

    def w2(s, ph):
        r = dict(crossings=sp.count_crossings(dq["o"], dq["d"], outputs=("count", "winding", "pops"), stream=s))
        ptrs = (C.c_void_p * len(poses))(*[img[ph, i].data_ptr() for i in range(len(poses))])
        rt.check(render_batch(handle, cams, ptrs, W * 3, len(poses), s.cuda_stream, 0), "rt_render_batch")
        r["winding"] = sp.winding_numbers(dq["pts"], stream=s)
        r["crossings_tmax"] = sp.count_crossings(dq["o"], dq["d"], dq["tmax"], stream=s)
        return r

    def w3(s, ph):
        return dict(xl_csr=sp.list_crossings(dq["o"], dq["d"], stream=s),
                    xl_k3=sp.list_crossings(dq["o"], dq["d"], max_hits=3, stream=s),
                    xl_k1=_select_k1(rt, handle, dq["o"], dq["d"], s))

    def w4(s, ph):
        return dict(nb_csr=sp.list_nearby(dq["pts"], dq["radius"], outputs=POINT_FIELDS, stream=s),
                    nb_k4=sp.list_nearby(dq["pts"], dq["radius"], max_hits=4, outputs=POINT_FIELDS, stream=s),
                    nb_k4_unbounded=sp.list_nearby(dq["pts"], max_hits=4, outputs=POINT_FIELDS + ("count",), stream=s))

    def w5(s, ph):
        return dict(ti_count=sp.count_intersecting(dq["tris"], dq["skip"], outputs=("count", "any", "pops"), stream=s),
                    ti_csr=sp.list_intersecting(dq["tris"], dq["skip"], outputs=TI_FIELDS, stream=s),
                    ti_k2=sp.list_intersecting(dq["tris"], dq["skip"], max_hits=2, outputs=TI_FIELDS + ("count",), stream=s))

    def w7(s, ph):
        return dict(bx_any=sp.count_in_boxes(dq["boxes"], outputs=("any",), stream=s),
                    bx_csr=sp.list_in_boxes(dq["boxes"], outputs=BX_FIELDS, stream=s),
                    bx_k4=sp.list_in_boxes(dq["boxes"], max_hits=4, outputs=BX_FIELDS, stream=s),
                    bx_grid=sp.occupancy_grid(grid[0], grid[1], GRID_DIMS, outputs=("occupied", "count"), stream=s))

    def w8(s, ph):
        return dict(sc_any=sp.count_sections(dq["planes"], outputs=("any",), stream=s),
                    sc_csr=sp.list_sections(dq["planes"], outputs=SC_FIELDS, stream=s),
                    sc_k4=sp.list_sections(dq["planes"], max_hits=4, outputs=("normal",), stream=s))

    def w9(s, ph):
        return dict(rg_any=sp.count_in_regions(dq["regions"], outputs=("any",), stream=s),
                    rg_csr=sp.list_in_regions(dq["regions"], outputs=RG_FIELDS, stream=s),
                    rg_k4_normal=sp.list_in_regions(dq["regions"], max_hits=4, outputs=("normal",), stream=s),
                    rg_k4_inside=sp.list_in_regions(dq["regions"], max_hits=4, outputs=("inside",), stream=s))

    def w10(s, ph):
        return dict(sg_md=sp.closest_to_segments(dq["segs"], dq["seg_md"], outputs=sg.OUTPUTS, stream=s),
                    td_md_skip=sp.closest_to_triangles(dq["qtris"], dq["qtri_md"], dq["qtri_skip"], outputs=tdo.OUTPUTS, stream=s),
                    sg_within=sp.closest_to_segments(dq["segs"], dq["seg_md"], outputs=("within",), stream=s))

    def w6():
        for ph in range(len(phases)):
            results["W6"][ph] = dict(xl_csr=sp.list_crossings(q["o"], q["d"]),
                                     crossings=sp.count_crossings(q["o"], q["d"]),
                                     xl_csr_again=sp.list_crossings(q["o"], q["d"], outputs=("t", "sign")))
            end_phase.wait()                                    # (synchronous calls: nothing of this phase is still in flight)
            next_phase.wait()
            ready[ph].synchronize()                             # (its launches go to the NULL stream, which no torch event orders)

    for name, calls in (("W1", w1), ("W2", w2), ("W3", w3), ("W4", w4), ("W5", w5), ("W7", w7), ("W8", w8), ("W9", w9),
                        ("W10", w10)):
        th.start(name, worker, name, calls)
    th.start("W6", w6)
    try:
        for ph in range(len(phases)):
            end_phase.wait()
            for w in streams:
                mut.wait_event(done[w][ph])
            if ph + 1 < len(phases):
                to = phases[ph + 1]
                sp.update_mesh_instance(2, 0, 2, *inst2[to], stream=mut.cuda_stream)
                if ph + 2 == len(phases):                       # the last change: a new tree, built on the device from the rest shape
                    v, n, uv = rest_dev
                    rt.check(h.rt_scene_rebuild_mesh_device(handle, 1, v.data_ptr(), n.data_ptr(), uv.data_ptr(), v.shape[0], mut.cuda_stream),
                             "rt_scene_rebuild_mesh_device")
                else:
                    v, n = arrays[to]
                    rt.check(h.rt_scene_refit_mesh(handle, 1, v.ctypes.data_as(_f), n.ctypes.data_as(_f), len(v), mut.cuda_stream),
                             "rt_scene_refit_mesh")
            ready[ph].record(mut)
            next_phase.wait()
    except threading.BrokenBarrierError:
        pass                                                    # (a worker failed: join says which and why)
    th.join()
    torch.cuda.synchronize()

    for ph, state in enumerate(phases):
        ref = want[state]
        at = "phase %d (S%d)" % (ph, state)
        r = results["W1"][ph]
        _same(r["closest"], ref["closest"], POINT_FIELDS, at + " closest_points")
        _same(r["closest_md"], ref["closest_md"], POINT_FIELDS, at + " closest_points bounded")
        _eq(_np(r["sdf"]), ref["sdf"], at + " signed_distance")
        r = results["W2"][ph]
        _same(r["crossings"], ref["crossings"], ("count", "winding"), at + " count_crossings")
        _same(r["crossings_tmax"], ref["crossings_tmax"], ("count", "winding"), at + " count_crossings tmax")
        _eq(_np(r["winding"]), ref["winding"], at + " winding_numbers")
        for i in range(len(poses)):
            _same_frame(dict(img=img[ph, i].cpu().numpy().reshape(H, W, 3)), dict(img=ref["frames"][i]), at + " frame %d" % i, planes=())
        r = results["W3"][ph]
        _same(r["xl_csr"], ref["xl_csr"], XL_FIELDS + ("offsets", "ray", "count"), at + " list_crossings CSR")
        _same(r["xl_k3"], ref["xl_k3"], XL_FIELDS + ("count",), at + " list_crossings K=3")
        _same(r["xl_k1"], {k: ref["xl_k1"][k].reshape((len(o),) + ref["xl_k1"][k].shape[2:]) for k in ("sign", "point")},
              ("sign", "point"), at + " list_crossings K=1 selection")
        r = results["W4"][ph]
        _same(r["nb_csr"], ref["nb_csr"], POINT_FIELDS + ("offsets", "point_index", "count"), at + " list_nearby CSR")
        _same(r["nb_k4"], ref["nb_k4"], POINT_FIELDS, at + " list_nearby K=4")
        _same(r["nb_k4_unbounded"], ref["nb_k4_unbounded"], POINT_FIELDS + ("count",), at + " list_nearby K=4 unbounded")
        r = results["W5"][ph]
        _eq(_np(r["ti_count"]["count"]), ref["ti_count"], at + " count_intersecting")
        assert np.array_equal(_np(r["ti_count"]["any"]), ref["ti_count"] > 0), at + " count_intersecting any"
        _same(r["ti_csr"], ref["ti_csr"], TI_FIELDS + ("offsets", "query_index", "count"), at + " list_intersecting CSR")
        _same(r["ti_k2"], ref["ti_k2"], TI_FIELDS + ("count",), at + " list_intersecting K=2")
        r = results["W6"][ph]
        _same(r["xl_csr"], ref["xl_csr"], XL_FIELDS + ("offsets", "ray", "count"), at + " list_crossings CSR (numpy)")
        _same(r["crossings"], ref["crossings"], ("count", "winding"), at + " count_crossings (numpy)")
        _same(r["xl_csr_again"], ref["xl_csr"], ("t", "sign", "offsets", "ray", "count"), at + " list_crossings CSR again (numpy)")
        r = results["W7"][ph]
        assert set(r["bx_any"]) == {"any"} and set(r["bx_k4"]) == set(BX_FIELDS)
        assert np.array_equal(_np(r["bx_any"]["any"]), ref["bx_count"] > 0), at + " count_in_boxes any alone"
        _same(r["bx_csr"], ref["bx_csr"], BX_FIELDS + ("offsets", "query_index", "count"), at + " list_in_boxes CSR")
        _same(r["bx_k4"], ref["bx_k4"], BX_FIELDS, at + " list_in_boxes K=4 without count")
        _eq(_np(r["bx_grid"]["count"]), ref["bx_grid"], at + " occupancy_grid count")
        assert np.array_equal(_np(r["bx_grid"]["occupied"]), ref["bx_grid"] > 0), at + " occupancy_grid occupied"
        r = results["W8"][ph]
        assert set(r["sc_any"]) == {"any"} and set(r["sc_k4"]) == {"normal"}
        assert np.array_equal(_np(r["sc_any"]["any"]), ref["sc_count"] > 0), at + " count_sections any alone"
        _same(r["sc_csr"], ref["sc_csr"], SC_FIELDS + ("offsets", "query_index", "count"), at + " list_sections CSR")
        _same(r["sc_k4"], ref["sc_k4"], ("normal",), at + " list_sections K=4, the normal alone, without count")
        r = results["W9"][ph]
        assert set(r["rg_any"]) == {"any"} and set(r["rg_k4_normal"]) == {"normal"} and set(r["rg_k4_inside"]) == {"inside"}
        assert np.array_equal(_np(r["rg_any"]["any"]), ref["rg_count"] > 0), at + " count_in_regions any alone"
        _same(r["rg_csr"], ref["rg_csr"], RG_FIELDS + ("offsets", "query_index", "count"), at + " list_in_regions CSR")
        _same(r["rg_k4_normal"], ref["rg_k4"], ("normal",), at + " list_in_regions K=4, the normal alone, without count")
        _same(r["rg_k4_inside"], ref["rg_k4"], ("inside",), at + " list_in_regions K=4, the inside flag alone, without count")
        r = results["W10"][ph]
        assert set(r["sg_md"]) == set(sg.OUTPUTS) and set(r["td_md_skip"]) == set(tdo.OUTPUTS) and set(r["sg_within"]) == {"within"}
        assert {"crossings", "clearance", "within"} <= set(sg.OUTPUTS) and {"intersections", "clearance", "within"} <= set(tdo.OUTPUTS)
        _same(r["sg_md"], ref["sg_md"], sg.OUTPUTS, at + " closest_to_segments")
        _same(r["td_md_skip"], ref["td_md_skip"], tdo.OUTPUTS, at + " closest_to_triangles")
        _same(r["sg_within"], ref["sg_md"], ("within",), at + " closest_to_segments within alone")
    sp.close()


def _select_k1(rt, handle, d_o, d_d, stream):
    """rt_list_crossings with max_hits = 1 and only sign and point given (no key field: the selection path), on `stream`, which is
    the calling thread's current torch stream -> dict(sign [n], point [n, 3])"""
    import torch
    n = d_o.shape[0]
    sign = torch.empty((n,), dtype=torch.int8, device="cuda")
    point = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    lst = rt.RtCrossingList(sign=sign.data_ptr(), point=point.data_ptr())
    rt.check(rt.libs()[0].rt_list_crossings(handle, d_o.data_ptr(), d_d.data_ptr(), None, n, None, 1, C.byref(lst), stream.cuda_stream, 0),
             "rt_list_crossings")
    return dict(sign=sign, point=point)
