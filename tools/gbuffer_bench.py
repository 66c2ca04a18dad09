#!/usr/bin/env python3
"""Throughput of G-buffer frames (rt_render_gbuffer) on the GPU, in one process, with device events.  Prints one JSON line: per
workload and variant ms per FRAME and Grays/s (1e9 primary rays per second) -- the median of `--repeats` timed windows of `--calls`
calls each, with the fastest and slowest window as the spread.  The variants of a workload are alternated window by window.
1920x1080; c2 (blob70k) from its far / mid / near cameras and the demo scene; `--frames` (32) frames per batched launch along bench.py's
camera path.

  (1) batch            rt_render_batch, 32 frames: the floor (colour bytes only)
  (2) gbuf_ids_img     rt_render_gbuffer, 32 frames, t + instance + triangle, with images
  (3) gbuf_ids         (2) without images
  (4) gbuf_all         rt_render_gbuffer, 32 frames, every plane (no images)
  (5) detour_ids / detour_all   what the call replaces, one frame per call: rt_camera_rays + rt_trace_rays (input order) for the
                       planes of (2) and of (4) (`depth` has no counterpart there and is left out)
  (6) gbuf_one / render_ids_one  one frame per launch: rt_render_gbuffer (t + ids + image) against rt_render_ids

   python tools/gbuffer_bench.py [--repeats 7] [--calls 5] [--frames 32] [--out file]"""
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
import bench  # noqa: E402  (scene files, parts and the camera path exactly as bench.py builds them)
from ray_query_bench import product_scene  # noqa: E402


def timed(variants, repeats, calls):
    """variants: {name: (zero-argument callable enqueuing one call on the current stream, frames per call)} -> {name: stats per frame}"""
    import torch
    for f, _n in variants.values():                             # warm-up: code objects, the view pool, the allocator
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, (f, n) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / (calls * n))
    return ms


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
        raise SystemExit("gbuffer_bench.py needs a GPU")
    h = rt.libs()[0]
    W, H, F = 1920, 1080, a.frames
    px = W * H
    result = {"metric": "gbuffer_ms_per_frame", "unit": "ms per 1920x1080 frame, Grays/s (1e9 primary rays/s)", "repeats": a.repeats,
              "calls": a.calls, "frames_per_launch": F, "code_hash": rt.library_hash(), "workloads": {}}
    f32, i32 = torch.float32, torch.int32
    planes = dict(t=torch.empty((F, H, W), dtype=f32, device="cuda"), depth=torch.empty((F, H, W), dtype=f32, device="cuda"),
                  instance=torch.empty((F, H, W), dtype=i32, device="cuda"), triangle=torch.empty((F, H, W), dtype=i32, device="cuda"),
                  location=torch.empty((F, H, W, 3), dtype=f32, device="cuda"), normal=torch.empty((F, H, W, 3), dtype=f32, device="cuda"),
                  uv=torch.empty((F, H, W, 2), dtype=f32, device="cuda"))
    img = torch.empty((F, H, W * 3), dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * F)(*[img[i].data_ptr() for i in range(F)])
    rays = torch.empty((2, H, W, 3), dtype=f32, device="cuda")
    ids = ("t", "instance", "triangle")
    gb_ids = rt.RtGBuffer(**{k: planes[k].data_ptr() for k in ids})
    gb_all = rt.RtGBuffer(**{k: v.data_ptr() for k, v in planes.items()})
    hits_ids = rt.RtRayHits(**{k: planes[k].data_ptr() for k in ids})
    hits_all = rt.RtRayHits(**{k: planes[k].data_ptr() for k in ids + ("location", "normal", "uv")})
    st = lambda: torch.cuda.current_stream().cuda_stream
    for workload, cams in (("c2", scenes.C2_CAMERAS), ("demo", {"demo": scenes.DEMO["cam_pose"]})):
        s = product_scene(workload)
        sh = s.device_handle
        s.reserve_views(F)
        for name, pose in cams.items():
            cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
            cp = (rt.RtCameraParams * F)()
            for i, ps in enumerate(bench.camera_path(pose, F)):
                cam.set_pose(ps)
                cp[i] = cam.params()
            cam.close()

            def gbuf(n, gb, with_img):
                return lambda: rt.check(h.rt_render_gbuffer(sh, cp, n, ptrs if with_img else None, W * 3, C.byref(gb), st(), 0), "rt_render_gbuffer")

            def detour(hits):
                def call():
                    rt.check(h.rt_camera_rays(C.byref(cp[0]), rays[0].data_ptr(), rays[1].data_ptr(), st(), 0), "rt_camera_rays")
                    rt.check(h.rt_trace_rays(sh, rays[0].data_ptr(), rays[1].data_ptr(), px, C.byref(hits), None, 0, st(), 0), "rt_trace_rays")
                return call

            v = {"batch": (lambda: rt.check(h.rt_render_batch(sh, cp, ptrs, W * 3, F, st(), 0), "rt_render_batch"), F),
                 "gbuf_ids_img": (gbuf(F, gb_ids, True), F), "gbuf_ids": (gbuf(F, gb_ids, False), F), "gbuf_all": (gbuf(F, gb_all, False), F),
                 "detour_ids": (detour(hits_ids), 1), "detour_all": (detour(hits_all), 1),
                 "gbuf_one": (gbuf(1, gb_ids, True), 1),
                 "render_ids_one": (lambda: rt.check(h.rt_render_ids(sh, cp, ptrs[0], W * 3, planes["instance"].data_ptr(), planes["triangle"].data_ptr(),
                                                                     st(), 0), "rt_render_ids"), 1)}
            ms = timed(v, a.repeats, a.calls)
            r = {}
            for k, w in ms.items():
                med = float(np.median(w))
                r[k] = dict(ms=round(med, 4), ms_min=round(min(w), 4), ms_max=round(max(w), 4), grays=round(px / med / 1e6, 3))
            # the yardsticks: the detour for the feature (> 1 = the G-buffer is faster), the colour-only batch for its overhead (> 1 = slower)
            r["detour_ids_over_gbuf_ids_img"] = round(r["detour_ids"]["ms"] / r["gbuf_ids_img"]["ms"], 3)
            r["detour_all_over_gbuf_all"] = round(r["detour_all"]["ms"] / r["gbuf_all"]["ms"], 3)
            r["gbuf_ids_img_over_batch"] = round(r["gbuf_ids_img"]["ms"] / r["batch"]["ms"], 3)
            r["gbuf_all_over_batch"] = round(r["gbuf_all"]["ms"] / r["batch"]["ms"], 3)
            r["gbuf_one_over_render_ids_one"] = round(r["gbuf_one"]["ms"] / r["render_ids_one"]["ms"], 3)
            result["workloads"]["%s_%s" % (workload, name)] = r
        torch.cuda.synchronize()
        s.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
