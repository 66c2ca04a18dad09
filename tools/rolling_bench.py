#!/usr/bin/env python3
"""Throughput of rolling frames and rolling clouds (rt_render_gbuffer_rolling, rt_point_cloud_offsets_rolling + _fill_rolling) on the
GPU, with device events.  Prints one JSON line: per workload and variant ms per FRAME -- the median of `--repeats` timed windows of
`--calls` calls each, with the fastest and slowest window as the spread.  The variants of a process are alternated window by window.

Workloads, `--frames` (32) frames per launch, t + instance + triangle without images, frame i rolling from pose i to pose i + 1 of
bench.py's camera path:
  panorama_atrium   a 2048x1024 equirectangular sensor inside the atrium (c4's scene), 256 column slices of 8
  lidar_atrium      a 64 x 2048 spinning lidar at the same place, 256 column slices of 8
  shutter_c2_mid    c2 from its mid camera at 1920x1080, the table from rt_camera_directions, 135 row slices of 8
Variants:
  rolling        (a) the rolling call
  static_plain   (b) the floor: rt_render_gbuffer_table on the same table, one pose per frame, with RT_VIEW_RECORDS=0 -- the same
                     plain-record kernel form, an entry point rolling frames do not touch
  static_views   (c) the same static call with view records: what rolling forgoes
  detour         (d) one rt_trace_rays over all pixels' rays of one rolling frame, the rays prepared beforehand and not timed
  cloud_rolling / cloud_static_plain / cloud_static_views   the two-step cloud with the default fields (local, range, pixel), the
                     total read on the host in between as the wrappers do, against rt_point_cloud_offsets_table + rt_point_cloud_fill
RT_VIEW_RECORDS is read once per process, so the script runs two children: `plain` (RT_VIEW_RECORDS=0: a, b, d and the clouds) and
`views` (a, c and the clouds); the ratios compare variants of the SAME child.

   python tools/rolling_bench.py [--repeats 7] [--calls 3] [--frames 32] [--out profiles/rolling_line.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    r = {}
    for k, w in ms.items():
        r[k] = dict(ms=round(float(np.median(w)), 4), ms_min=round(min(w), 4), ms_max=round(max(w), 4))
    return r


def ratio(r, a, b):
    """a / b with the larger of the two min-max spreads relative to b"""
    spread = max(r[a]["ms_max"] - r[a]["ms_min"], r[b]["ms_max"] - r[b]["ms_min"])
    return dict(ratio=round(r[a]["ms"] / r[b]["ms"], 4), difference_ms=round(r[a]["ms"] - r[b]["ms"], 4), larger_spread_ms=round(spread, 4))


def child(a):
    import torch
    rt = importlib.import_module("cuda-raytracing_amd")
    scenes = importlib.import_module("cuda-raytracing_amd.scenes")
    sensors = importlib.import_module("cuda-raytracing_amd.sensors")
    import bench  # noqa: E402  (scene files, parts and the camera path exactly as bench.py builds them)
    from gbuffer_bench import timed  # noqa: E402
    from ray_query_bench import product_scene  # noqa: E402
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("rolling_bench.py needs a GPU")
    h, host = rt.libs()
    F, views = a.frames, a.mode == "views"
    f32, i32 = torch.float32, torch.int32
    st = lambda: torch.cuda.current_stream().cuda_stream    # noqa: E731
    ids = ("t", "instance", "triangle")
    fields = rt.RT_CLOUD_BITS["local"] | rt.RT_CLOUD_BITS["range"] | rt.RT_CLOUD_BITS["pixel"]
    out = {}

    def inverse(p):
        q = np.zeros(6, np.float32)
        host.rth_invert_lre(p.ctypes.data_as(C.POINTER(C.c_float)), q.ctypes.data_as(C.POINTER(C.c_float)))
        return q

    def workload(name, scene, d_dirs, W, H, axis, sp, pose):
        px = W * H
        sh = scene.device_handle
        if views:
            scene.reserve_views(F)                              # (the pool grown before the clock runs; refused where views are off)
        table = C.c_void_p()
        rt.check(h.rt_ray_table_create(C.c_void_p(d_dirs.data_ptr()), W, H, None, 1, C.byref(table)), "rt_ray_table_create")
        n = C.c_int32()
        rt.check(h.rt_rolling_slices(W, H, axis, sp, C.byref(n)), "rt_rolling_slices")
        S = n.value
        path = [np.asarray(p, np.float32) for p in bench.camera_path(pose, F + 1)]
        cp = (rt.RtCameraParams * F)()
        rp = (rt.RtRollingPose * (F * S))()
        for i in range(F):
            q = inverse(path[i])
            cp[i].width, cp[i].height = W, H
            for j in range(6):
                cp[i].camera_pose[j], cp[i].inv_camera_pose[j] = float(path[i][j]), float(q[j])
            for s_, p in enumerate(sensors.rolling_poses(path[i], path[i + 1], S)):
                q = inverse(p)
                for j in range(6):
                    rp[i * S + s_].camera_pose[j], rp[i * S + s_].inv_camera_pose[j] = float(p[j]), float(q[j])
        planes = dict(t=torch.empty((F, H, W), dtype=f32, device="cuda"), instance=torch.empty((F, H, W), dtype=i32, device="cuda"),
                      triangle=torch.empty((F, H, W), dtype=i32, device="cuda"))
        gb = rt.RtGBuffer(**{k: planes[k].data_ptr() for k in ids})
        rws_bytes = int(h.rt_rolling_workspace_bytes(F, S))
        rws = torch.empty((rws_bytes,), dtype=torch.uint8, device="cuda")

        def rolling():
            rt.check(h.rt_render_gbuffer_rolling(sh, table, rp, F, axis, sp, None, 0, C.byref(gb), None, rws.data_ptr(), rws_bytes, st(), 0),
                     "rt_render_gbuffer_rolling")

        def static():
            rt.check(h.rt_render_gbuffer_table(sh, table, cp, F, None, 0, C.byref(gb), st(), 0), "rt_render_gbuffer_table")

        v = {"rolling": (rolling, F), "static_views" if views else "static_plain": (static, F)}
        if not views:
            # (d) the rays of rolling frame 0, assembled per slice beforehand
            ro, rd = torch.empty((H, W, 3), dtype=f32, device="cuda"), torch.empty((H, W, 3), dtype=f32, device="cuda")
            o1, d1 = torch.empty_like(ro), torch.empty_like(rd)
            one = (rt.RtCameraParams * 1)()
            one[0].width, one[0].height = W, H
            for s_ in range(S):
                for j in range(6):
                    one[0].camera_pose[j], one[0].inv_camera_pose[j] = rp[s_].camera_pose[j], rp[s_].inv_camera_pose[j]
                rt.check(h.rt_ray_table_rays(table, C.byref(one[0]), o1.data_ptr(), d1.data_ptr(), st(), 1), "rt_ray_table_rays")
                at = (slice(s_ * sp, (s_ + 1) * sp), slice(None)) if axis else (slice(None), slice(s_ * sp, (s_ + 1) * sp))
                ro[at], rd[at] = o1[at], d1[at]
            del o1, d1
            hits = rt.RtRayHits(**{k: planes[k].data_ptr() for k in ids})
            v["detour"] = (lambda: rt.check(h.rt_trace_rays(sh, ro.data_ptr(), rd.data_ptr(), px, C.byref(hits), None, 0, st(), 0), "rt_trace_rays"), 1)
        r = stats(timed(v, a.repeats, a.calls))
        torch.cuda.synchronize()
        del planes

        # ---- clouds, default fields
        off = torch.empty((F + 1,), dtype=torch.int64, device="cuda")
        cws_bytes = int(h.rt_point_cloud_rolling_workspace_bytes(W, H, F, fields, S))
        sws_bytes = int(h.rt_point_cloud_workspace_bytes(W, H, F, fields))
        cws = torch.empty((cws_bytes,), dtype=torch.uint8, device="cuda")
        cap = F * px
        local, rng, pix = torch.empty((cap, 3), dtype=f32, device="cuda"), torch.empty((cap,), dtype=f32, device="cuda"), torch.empty((cap,), dtype=i32, device="cuda")
        cloud = rt.RtPointCloud(local=local.data_ptr(), range=rng.data_ptr(), pixel=pix.data_ptr())
        inf = float("inf")
        kept = {}

        def cloud_rolling():
            rt.check(h.rt_point_cloud_offsets_rolling(sh, table, rp, F, axis, sp, 0.0, inf, None, fields, off.data_ptr(), cws.data_ptr(), cws_bytes, st(), 0),
                     "rt_point_cloud_offsets_rolling")
            total = int(off[F].item())                                  # (the one host read of the wrappers)
            kept["rolling"] = total
            rt.check(h.rt_point_cloud_fill_rolling(W, H, F, axis, sp, fields, cws.data_ptr(), cws_bytes, total, C.byref(cloud), st(), 0),
                     "rt_point_cloud_fill_rolling")

        def cloud_static():
            rt.check(h.rt_point_cloud_offsets_table(sh, table, cp, F, 0.0, inf, None, fields, off.data_ptr(), cws.data_ptr(), sws_bytes, st(), 0),
                     "rt_point_cloud_offsets_table")
            total = int(off[F].item())
            kept["static"] = total
            rt.check(h.rt_point_cloud_fill(cp, F, fields, cws.data_ptr(), sws_bytes, total, C.byref(cloud), st(), 0), "rt_point_cloud_fill")

        c = stats(timed({"cloud_rolling": (cloud_rolling, F), "cloud_static_views" if views else "cloud_static_plain": (cloud_static, F)}, a.repeats, a.calls))
        r.update(c)
        r["slices"] = S
        r["kept_fraction"] = {k: round(n_ / cap, 4) for k, n_ in kept.items()}
        torch.cuda.synchronize()
        rt.check(h.rt_ray_table_destroy(table), "rt_ray_table_destroy")
        out[name] = r

    s = product_scene("c4")
    workload("panorama_atrium", s, torch.from_numpy(sensors.equirectangular(2048, 1024)).to("cuda"), 2048, 1024, 0, 8, scenes.C4["cam_pose"])
    workload("lidar_atrium", s, torch.from_numpy(sensors.spinning_lidar(np.radians(np.linspace(-25.0, 15.0, 64)), 2048)).to("cuda"), 2048, 64, 0, 8,
             scenes.C4["cam_pose"])
    s.close()
    s = product_scene("c2")
    cam = rt.Camera(1920, 1080, scenes.scaled_K(1920), scenes.D_REF)
    workload("shutter_c2_mid", s, cam.directions(), 1920, 1080, 1, 8, scenes.C2_CAMERAS["mid"])
    cam.close()
    s.close()
    print("ROLLING_CHILD " + json.dumps({"mode": a.mode, "code_hash": rt.library_hash(), "workloads": out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mode", default=None, choices=("plain", "views"))
    a = ap.parse_args()
    if a.mode:
        return child(a)
    result = {"metric": "rolling_ms_per_frame", "unit": "ms per frame", "repeats": a.repeats, "calls": a.calls, "frames_per_launch": a.frames, "workloads": {}}
    for mode in ("plain", "views"):                                     # one after the other: a fresh process each, never two on the GPU
        env = dict(os.environ, RT_VIEW_RECORDS="0" if mode == "plain" else "1")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", mode, "--repeats", str(a.repeats), "--calls", str(a.calls),
                            "--frames", str(a.frames)], env=env, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            raise SystemExit("the %s child ended with %d" % (mode, p.returncode))
        got = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("ROLLING_CHILD ")][-1][len("ROLLING_CHILD "):])
        result["code_hash"] = got["code_hash"]
        for name, r in got["workloads"].items():
            w = result["workloads"].setdefault(name, {"slices": r["slices"]})
            w[mode] = r
            if mode == "plain":
                w["rolling_over_floor"] = ratio(r, "rolling", "static_plain")                   # (a) / (b)
                w["detour_over_rolling"] = ratio(r, "detour", "rolling")                        # (d) / (a): > 1 = the call is faster
                w["cloud_rolling_over_static_plain"] = ratio(r, "cloud_rolling", "cloud_static_plain")
            else:
                w["rolling_over_static_views"] = ratio(r, "rolling", "static_views")            # (a) / (c): what rolling forgoes
                w["cloud_rolling_over_static_views"] = ratio(r, "cloud_rolling", "cloud_static_views")
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
