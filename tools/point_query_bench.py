#!/usr/bin/env python3
"""Throughput of the closest-point queries (Scene.closest_points) on the GPU, in one process, with device events.  Prints one JSON line:
per workload the rate in Gqueries/s (1e9 points per second), ms per call and mean interior nodes visited (pops) -- the median of
`--repeats` timed windows of `--calls` calls each, with the fastest and slowest window as the spread -- and trace_rays on the same number
of camera rays as a reference point.  The variants of a workload are alternated window by window.

  (a) c2 (blob70k, mid camera, 1920x1080): every hit location offset by 1e-3 of the scene diagonal along its normal, in pixel order
  (b) the same points randomly permuted
  (c) 4 M random points in c2's bounding box (as far as the camera sees it)
  (d) (a) with max_distance = 1e-2 of the diagonal
  (e) the demo scene (bench.py --workload demo): its camera's hit locations

   python tools/point_query_bench.py [--repeats 7] [--calls 5] [--out file]"""
import argparse
import importlib
import json
import os
import sys


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
rt = importlib.import_module("cuda-raytracing_amd")
scenes = importlib.import_module("cuda-raytracing_amd.scenes")
from ray_query_bench import product_scene, timed  # noqa: E402  (the same scenes and timing as the ray-query line)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--random-points", type=int, default=1 << 22)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("point_query_bench.py needs a GPU")
    W, H = 1920, 1080
    result = {"metric": "point_query_gqps", "unit": "Gqueries/s (1e9 points/s), ms per call, mean pops", "repeats": a.repeats,
              "calls": a.calls, "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]
    outs = ("distance", "instance", "triangle")

    def run(name, s, pts, md=None, extra=None):
        v = {"closest_points": lambda: s.closest_points(pts, md, outputs=outs)}
        v.update(extra or {})
        r = timed(v, pts.shape[0], a.repeats, a.calls)
        for k in v:
            r[k]["gqps" if k == "closest_points" else "grays"] = r[k].pop("grays")
        got = s.closest_points(pts, md, outputs=("instance", "pops"))
        r["points"] = int(pts.shape[0])
        r["mean_pops"] = round(float(got["pops"].double().mean()), 2)
        r["hit_frac"] = round(float((got["instance"] >= 0).double().mean()), 4)
        wls[name] = r

    for workload, pose in (("c2", scenes.C2_CAMERAS["mid"]), ("demo", scenes.DEMO["cam_pose"])):
        s = product_scene(workload)
        cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
        cam.set_pose(pose)
        o, d = cam.rays()
        hit = s.trace_rays(o, d, outputs=("instance", "location", "normal"), binning=False)
        keep = (hit["instance"] >= 0).reshape(-1)
        loc = hit["location"].reshape(-1, 3)[keep].contiguous()
        nrm = hit["normal"].reshape(-1, 3)[keep].contiguous()
        lo, hi = loc.min(dim=0).values, loc.max(dim=0).values
        diag = float(torch.linalg.vector_norm(hi - lo))
        n = loc.shape[0]
        ro, rd = o.reshape(-1, 3)[:n].contiguous(), d.reshape(-1, 3)[:n].contiguous()
        ref = {"trace_rays": lambda: s.trace_rays(ro, rd, outputs=("t", "instance", "triangle"), binning=False)}
        if workload == "c2":
            pts = (loc + nrm * (1e-3 * diag)).contiguous()
            run("a_c2_mid_offset", s, pts, extra=ref)
            perm = torch.randperm(n, device="cuda")
            run("b_c2_mid_offset_shuffled", s, pts[perm].contiguous())
            g = torch.Generator(device="cuda").manual_seed(7)
            rp = (lo + (hi - lo) * torch.rand((a.random_points, 3), device="cuda", generator=g)).contiguous()
            run("c_c2_random", s, rp)
            wls["c_c2_random"]["box"] = [[round(x, 4) for x in v.tolist()] for v in (lo, hi)]
            md = torch.full((n,), 1e-2 * diag, dtype=torch.float32, device="cuda")
            run("d_c2_mid_offset_bounded", s, pts, md)
            wls["diag_c2"] = round(diag, 4)
        else:
            run("e_demo_surface", s, loc, extra=ref)
        s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
