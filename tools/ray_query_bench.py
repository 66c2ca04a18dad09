#!/usr/bin/env python3
"""Throughput of the ray queries (Scene.trace_rays / Scene.occluded) on the GPU, in one process, with device events.  Prints one JSON
line: per workload and variant the rate in Grays/s (1e9 rays per second) and ms per call -- the median of `--repeats` timed windows of
`--calls` calls each, with the fastest and slowest window as the spread.  The variants of a workload are alternated window by window.

  (a) c2 (blob70k, 1920x1080; cameras far / mid / near): Camera.rays() in pixel order through trace_rays (ids + t), binning off and on,
      next to rt_render_ids on the same frame (the production render kernel writing the same ids)
  (b) the same rays randomly permuted, binning off and on
  (c) 4 M random rays in c2's bounding box (uniform origins, uniform directions on the sphere), binning off and on
  (d) shadow rays from (a)'s hit locations (mid camera) toward the sun of raycast.cu:249-250 through occluded, binning off and on
  (e) the demo scene (bench.py --workload demo: two posed, textured instances): (a) and (c)

   python tools/ray_query_bench.py [--repeats 7] [--calls 5] [--out file]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
rt = importlib.import_module("cuda-raytracing_amd")
scenes = importlib.import_module("cuda-raytracing_amd.scenes")
import bench  # noqa: E402  (scene files and parts exactly as bench.py builds them)


def product_scene(workload):
    wl = scenes.WORKLOADS[workload]
    obj = bench.scene_path(workload)
    mats, objs, insts = bench.scene_parts(workload, wl, obj)
    s = rt.Scene()
    for albedo, tex, extra in mats:
        s.add_material(albedo, texture_bgr=tex, **extra)
    for p in objs:
        s.add_mesh(rt.Mesh.load_obj(p))
    for mesh, mat, pose, scale in insts:
        s.add_mesh_instance(mesh, mat, pose, scale)
    s.upload_to_device()
    return s


def timed(variants, n_rays, repeats, calls):
    """variants: {name: zero-argument callable enqueuing one call on the current stream} -> {name: stats}, windows alternated"""
    import torch
    for f in variants.values():                                 # warm-up: code objects, allocator
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, f in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    out = {}
    for k, v in ms.items():
        med = float(np.median(v))
        out[k] = dict(ms=round(med, 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4), grays=round(n_rays / med / 1e6, 3))
    return out


def trace_variants(s, o, d, outputs=("t", "instance", "triangle")):
    return {"trace": lambda: s.trace_rays(o, d, outputs=outputs, binning=False),
            "trace_binned": lambda: s.trace_rays(o, d, outputs=outputs, binning=True)}


def random_rays(s_box, n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    lo, hi = (torch.tensor(v, dtype=torch.float32, device="cuda") for v in s_box)
    o = (lo + (hi - lo) * torch.rand((n, 3), device="cuda", generator=g)).contiguous()
    d = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=g), dim=1).contiguous()
    return o, d


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--random-rays", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("ray_query_bench.py needs a GPU")
    h = rt.libs()[0]
    W, H = 1920, 1080
    result = {"metric": "ray_query_grays", "unit": "Grays/s (1e9 rays/s), ms per call", "repeats": a.repeats, "calls": a.calls,
              "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]
    for workload, cams in (("c2", scenes.C2_CAMERAS), ("demo", {"demo": scenes.DEMO["cam_pose"]})):
        s = product_scene(workload)
        img = torch.empty((H, W * 3), dtype=torch.uint8, device="cuda")
        ids = torch.empty((2, H, W), dtype=torch.int32, device="cuda")
        for name, pose in cams.items():
            cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
            cam.set_pose(pose)
            p = cam.params()
            o, d = cam.rays()
            st = lambda: torch.cuda.current_stream().cuda_stream
            v = trace_variants(s, o, d)
            v["render_ids"] = lambda: rt.check(h.rt_render_ids(s.device_handle, p, img.data_ptr(), W * 3, ids[0].data_ptr(), ids[1].data_ptr(),
                                                               st(), 0), "rt_render_ids")
            r = timed(v, W * H, a.repeats, a.calls)
            r["trace_over_render_ids"] = round(r["render_ids"]["ms"] / r["trace"]["ms"], 3)
            wls["a_%s_%s" % (workload, name)] = r
            if workload == "c2":
                perm = torch.randperm(W * H, device="cuda")
                po, pd = o.reshape(-1, 3)[perm].contiguous(), d.reshape(-1, 3)[perm].contiguous()
                wls["b_c2_%s_shuffled" % name] = timed(trace_variants(s, po, pd), W * H, a.repeats, a.calls)
            if name in ("mid", "demo"):
                hit = s.trace_rays(o, d, outputs=("instance", "location"), binning=False)
                keep = (hit["instance"] >= 0).reshape(-1)
                loc = hit["location"].reshape(-1, 3)[keep].contiguous()
                if workload == "c2":
                    sun = torch.tensor([-0.2, 0.0, 1.0], dtype=torch.float32, device="cuda")
                    sun = (sun / torch.linalg.vector_norm(sun)).expand_as(loc).contiguous()
                    n = loc.shape[0]
                    wls["d_c2_mid_shadow"] = timed({"occluded": lambda: s.occluded(loc, sun, binning=False),
                                                    "occluded_binned": lambda: s.occluded(loc, sun, binning=True)}, n, a.repeats, a.calls)
                    wls["d_c2_mid_shadow"]["rays"] = n
                # the scene's bounding box, as far as the camera sees it (every hit location), for the random rays of (c)
                box = (loc.min(dim=0).values.tolist(), loc.max(dim=0).values.tolist())
                ro, rd = random_rays(box, a.random_rays, 7)
                r = timed(trace_variants(s, ro, rd), a.random_rays, a.repeats, a.calls)
                r["rays"], r["box"] = a.random_rays, [[round(x, 4) for x in b] for b in box]
                wls["%s_%s_random" % ("c" if workload == "c2" else "e", workload)] = r
        s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
