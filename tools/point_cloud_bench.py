#!/usr/bin/env python3
"""Throughput of point clouds (rt_point_cloud_offsets(_table) + rt_point_cloud_fill) on the GPU, in one process, with device events.
Prints one JSON line: per workload and variant ms per FRAME -- the median of `--repeats` timed windows of `--calls` calls each, with
the fastest and slowest window as the spread.  The variants of a workload are alternated window by window.  Per workload:

    cloud    offsets + fill on one stream, the outputs allocated once at the exact total (the asynchronous use: no host read between)
    floor    rt_render_gbuffer(_table) of the planes the cloud call stages, alone: what any compaction has to pay first
    detour   what the call replaces: rt_render_gbuffer(_table) of t, instance, location, then on the device in torch the mask, nonzero
             (a host round trip), the gathers and the rotation into the sensor frame (range, pixel, local: the default fields)

  (a) camera_c2_<far|mid|near>: c2 (blob70k) at 1920x1080, `--frames` (32) frames per launch, local + range + pixel
  (b) panorama_atrium: the 2048x1024 equirectangular sensor inside the atrium (c4's scene and camera position), max_range = the median
      range of the first frame's returns, so that about half of them are kept; local + range + pixel
  (c) camera_c2_mid_every_field: (a)'s mid camera with all nine fields: the staging traffic a fused epilogue would save; no detour
  call_over_floor: the price of compaction; detour_over_call: the gain (> 1 = the call is faster).  The min-max ranges are there
  so that a reader can see whether two variants overlap.

   python tools/point_cloud_bench.py [--repeats 7] [--calls 5] [--frames 32] [--out profiles/point_cloud_line.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
rt = importlib.import_module("cuda-raytracing_amd")
scenes = importlib.import_module("cuda-raytracing_amd.scenes")
sensors = importlib.import_module("cuda-raytracing_amd.sensors")
import bench  # noqa: E402  (scene files, parts and the camera path exactly as bench.py builds them)
from gbuffer_bench import timed  # noqa: E402
from ray_query_bench import product_scene  # noqa: E402
from sensor_bench import table_of  # noqa: E402

BITS = rt.RT_CLOUD_BITS
DEFAULT = ("local", "range", "pixel")
STAGED = dict(triangle="triangle", position="location", local="location", normal="normal", uv="uv")     # field -> the plane it stages


def stats(ms):
    return {k: dict(ms=round(float(np.median(w)), 4), ms_min=round(min(w), 4), ms_max=round(max(w), 4)) for k, w in ms.items()}


def rotations(host, cp, n):
    """[n, 3, 3] and [n, 3] float32: local = R (location - position), R's columns from the host library's apply_lre on the axes"""
    R, pos = np.zeros((n, 3, 3), np.float32), np.zeros((n, 3), np.float32)
    fp = C.POINTER(C.c_float)
    for i in range(n):
        pose = np.array(list(cp[i].camera_pose), np.float32)
        pos[i] = pose[:3]
        rot = pose.copy()
        rot[:3] = 0
        for k in range(3):
            e, out = np.zeros(3, np.float32), np.zeros(3, np.float32)
            e[k] = 1
            host.rth_apply_lre(rot.ctypes.data_as(fp), e.ctypes.data_as(fp), out.ctypes.data_as(fp))
            R[i, :, k] = out
    return R, pos


def workload(h, host, sh, table, cp, F, W, H, fields, max_range, repeats, calls, with_detour):
    """the three variants of one workload; `table`: None = the cameras' own rays"""
    import torch
    f32, i32 = torch.float32, torch.int32
    st = lambda: torch.cuda.current_stream().cuda_stream
    px = W * H
    mask = 0
    for k in fields:
        mask |= BITS[k]
    ws_bytes = int(h.rt_point_cloud_workspace_bytes(W, H, F, mask))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    off = torch.empty((F + 1,), dtype=torch.int64, device="cuda")

    def offsets():
        if table is None:
            rc = h.rt_point_cloud_offsets(sh, cp, F, 0.0, max_range, None, mask, off.data_ptr(), ws.data_ptr(), ws_bytes, st(), 0)
        else:
            rc = h.rt_point_cloud_offsets_table(sh, table, cp, F, 0.0, max_range, None, mask, off.data_ptr(), ws.data_ptr(), ws_bytes, st(), 0)
        rt.check(rc, "rt_point_cloud_offsets")

    offsets()
    total = int(off[F].item())
    shape = dict(range=(), pixel=(), frame=(), instance=(), triangle=(), position=(3,), local=(3,), normal=(3,), uv=(2,))
    out = {k: torch.empty((total,) + shape[k], dtype=i32 if k in ("pixel", "frame", "instance", "triangle") else f32, device="cuda") for k in fields}
    cloud = rt.RtPointCloud(**{k: v.data_ptr() for k, v in out.items()})

    def call():
        offsets()
        rt.check(h.rt_point_cloud_fill(cp, F, mask, ws.data_ptr(), ws_bytes, total, C.byref(cloud), st(), 0), "rt_point_cloud_fill")

    staged = ("t", "instance") + tuple(sorted({STAGED[k] for k in fields if k in STAGED}))
    width = dict(t=(), instance=(), triangle=(), location=(3,), normal=(3,), uv=(2,))
    planes = {k: torch.empty((F, H, W) + width[k], dtype=i32 if k in ("instance", "triangle") else f32, device="cuda") for k in staged}
    gb = rt.RtGBuffer(**{k: v.data_ptr() for k, v in planes.items()})

    def floor():
        if table is None:
            rt.check(h.rt_render_gbuffer(sh, cp, F, None, 0, C.byref(gb), st(), 0), "rt_render_gbuffer")
        else:
            rt.check(h.rt_render_gbuffer_table(sh, table, cp, F, None, 0, C.byref(gb), st(), 0), "rt_render_gbuffer_table")

    variants = {"cloud": (call, F), "floor": (floor, F)}
    if with_detour:
        Rn, pn = rotations(host, cp, F)
        R, pos = torch.from_numpy(Rn).cuda(), torch.from_numpy(pn).cuda()

        def detour():
            floor()
            t, inst = planes["t"].reshape(-1), planes["instance"].reshape(-1)
            idx = ((inst >= 0) & (t >= 0.0) & (t <= max_range)).nonzero().squeeze(1)
            rng = t[idx]
            frame = idx // px
            pixel = (idx - frame * px).to(i32)
            v = planes["location"].reshape(-1, 3)[idx] - pos[frame]
            local = (R[frame] * v[:, None, :]).sum(-1)
            return rng, pixel, local
        variants["detour"] = (detour, F)
    r = stats(timed(variants, repeats, calls))
    r["kept_fraction"] = round(total / (F * px), 4)
    r["workspace_bytes_per_pixel"] = round(ws_bytes / (F * px), 2)
    r["call_over_floor"] = round(r["cloud"]["ms"] / r["floor"]["ms"], 3)
    if with_detour:
        r["detour_over_call"] = round(r["detour"]["ms"] / r["cloud"]["ms"], 3)
    torch.cuda.synchronize()
    return r


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("point_cloud_bench.py needs a GPU")
    h, host = rt.libs()
    F = a.frames
    result = {"metric": "point_cloud_ms_per_frame", "unit": "ms per frame", "repeats": a.repeats, "calls": a.calls, "frames_per_launch": F,
              "code_hash": rt.library_hash(), "workloads": {}}
    inf = float("inf")

    # ---- (a), (c) the c2 cameras
    W, H = 1920, 1080
    s = product_scene("c2")
    sh = s.device_handle
    s.reserve_views(F)
    for name, pose in scenes.C2_CAMERAS.items():
        cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
        cp = (rt.RtCameraParams * F)()
        for i, ps in enumerate(bench.camera_path(pose, F)):
            cam.set_pose(ps)
            cp[i] = cam.params()
        cam.close()
        result["workloads"]["camera_c2_%s" % name] = workload(h, host, sh, None, cp, F, W, H, DEFAULT, inf, a.repeats, a.calls, True)
        if name == "mid":
            result["workloads"]["camera_c2_mid_every_field"] = workload(h, host, sh, None, cp, F, W, H, tuple(BITS), inf, a.repeats, a.calls, False)
    s.close()

    # ---- (b) the panorama inside the atrium, a gate at the median range
    W, H = 2048, 1024
    s = product_scene("c4")
    sh = s.device_handle
    s.reserve_views(F)
    table = table_of(h, torch.from_numpy(sensors.equirectangular(W, H)).to("cuda"), W, H)
    cp = (rt.RtCameraParams * F)()
    inv = np.zeros(6, np.float32)
    for i, ps in enumerate(bench.camera_path(scenes.C4["cam_pose"], F)):
        p = np.asarray(ps, np.float32)
        host.rth_invert_lre(p.ctypes.data_as(C.POINTER(C.c_float)), inv.ctypes.data_as(C.POINTER(C.c_float)))
        cp[i].width, cp[i].height = W, H
        for j in range(6):
            cp[i].camera_pose[j], cp[i].inv_camera_pose[j] = float(p[j]), float(inv[j])
    t0 = torch.empty((1, H, W), dtype=torch.float32, device="cuda")
    i0 = torch.empty((1, H, W), dtype=torch.int32, device="cuda")
    gb = rt.RtGBuffer(t=t0.data_ptr(), instance=i0.data_ptr())
    rt.check(h.rt_render_gbuffer_table(sh, table, cp, 1, None, 0, C.byref(gb), None, 1), "rt_render_gbuffer_table")
    gate = float(t0[i0 >= 0].median().item())
    r = workload(h, host, sh, table, cp, F, W, H, DEFAULT, gate, a.repeats, a.calls, True)
    r["max_range"] = gate
    result["workloads"]["panorama_atrium"] = r
    torch.cuda.synchronize()
    rt.check(h.rt_ray_table_destroy(table), "rt_ray_table_destroy")
    s.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
