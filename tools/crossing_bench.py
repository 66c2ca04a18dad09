#!/usr/bin/env python3
"""Throughput of the crossing queries (Scene.count_crossings / winding_numbers / signed_distance) on the GPU, in one process, with
device events.  Prints one JSON line: per workload the rate in Gqueries/s (1e9 rays or points per second), ms per call and mean
interior nodes visited (pops) -- the median of `--repeats` timed windows of `--calls` calls each, with the fastest and slowest window
as the spread -- against trace_rays or closest_points on the same inputs.  The variants of a workload are alternated window by window.

  (a) c2 (blob70k, mid camera, 1920x1080) camera rays: count_crossings, against trace_rays on the same rays
  (b) winding_numbers of c2 surface points +- 1e-3 of the scene diagonal along the normal (half each, in pixel order), against
      closest_points on the same points
  (c) winding_numbers of 4 M random points in c2's bounding box (as far as the camera sees it)
  (d) signed_distance on (b)'s points
  (e) the demo scene (bench.py --workload demo): count_crossings of its camera rays, winding_numbers of its surface points +- offset

   python tools/crossing_bench.py [--repeats 7] [--calls 5] [--out file]"""
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
        raise SystemExit("crossing_bench.py needs a GPU")
    W, H = 1920, 1080
    result = {"metric": "crossing_query_gqps", "unit": "Gqueries/s (1e9 rays or points/s), ms per call, mean pops", "repeats": a.repeats,
              "calls": a.calls, "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]

    def run(name, variants, n, pops):
        r = timed(variants, n, a.repeats, a.calls)
        for k in variants:
            r[k]["gqps"] = r[k].pop("grays")                     # (timed's rate: n / ms / 1e6 = 1e9 queries per second)
        r["queries"] = int(n)
        r["mean_pops"] = {k: round(float(v.double().mean()), 2) for k, v in pops.items()}
        wls[name] = r
        return r

    for workload, pose in (("c2", scenes.C2_CAMERAS["mid"]), ("demo", scenes.DEMO["cam_pose"])):
        s = product_scene(workload)
        cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
        cam.set_pose(pose)
        o, d = cam.rays()
        o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
        hit = s.trace_rays(o, d, outputs=("instance", "location", "normal", "pops"), binning=False)
        keep = hit["instance"] >= 0
        loc, nrm = hit["location"][keep].contiguous(), hit["normal"][keep].contiguous()
        lo, hi = loc.min(dim=0).values, loc.max(dim=0).values
        diag = float(torch.linalg.vector_norm(hi - lo))
        side = torch.where(torch.arange(loc.shape[0], device="cuda") % 2 == 0, 1.0, -1.0)[:, None]
        pts = (loc + nrm * side * (1e-3 * diag)).contiguous()
        cross = s.count_crossings(o, d, outputs=("count", "pops"))
        run(("a_c2_camera_rays" if workload == "c2" else "e_demo_camera_rays"),
            {"count_crossings": lambda: s.count_crossings(o, d, outputs=("count", "winding")),
             "trace_rays": lambda: s.trace_rays(o, d, outputs=("t", "instance", "triangle"), binning=False)}, o.shape[0],
            {"count_crossings": cross["pops"], "trace_rays": hit["pops"]})
        wls["a_c2_camera_rays" if workload == "c2" else "e_demo_camera_rays"]["mean_count"] = round(float(cross["count"].double().mean()), 3)

        if workload == "c2":
            cp = s.closest_points(pts, outputs=("distance", "pops"))
            r = run("b_c2_surface_pm_offset",
                    {"winding_numbers": lambda: s.winding_numbers(pts), "closest_points": lambda: s.closest_points(pts, outputs=("distance",))},
                    pts.shape[0], {"winding_numbers": point_pops(s, pts), "closest_points": cp["pops"]})
            r["inside_frac"] = round(float((s.winding_numbers(pts) != 0).double().mean()), 4)
            g = torch.Generator(device="cuda").manual_seed(7)
            rp = (lo + (hi - lo) * torch.rand((a.random_points, 3), device="cuda", generator=g)).contiguous()
            r = run("c_c2_random", {"winding_numbers": lambda: s.winding_numbers(rp)}, rp.shape[0],
                    {"winding_numbers": point_pops(s, rp)})
            r["inside_frac"] = round(float((s.winding_numbers(rp) != 0).double().mean()), 4)
            r["box"] = [[round(x, 4) for x in v.tolist()] for v in (lo, hi)]
            run("d_c2_signed_distance", {"signed_distance": lambda: s.signed_distance(pts)}, pts.shape[0], {})
            wls["diag_c2"] = round(diag, 4)
        else:
            run("e_demo_surface_pm_offset", {"winding_numbers": lambda: s.winding_numbers(pts)}, pts.shape[0],
                {"winding_numbers": point_pops(s, pts)})
        s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def point_pops(s, pts):
    """interior nodes visited per point by winding_numbers (all three directions): the C-ABI's pops output of the point form is not
    exposed, so the three directions' rays are counted through count_crossings"""
    import torch
    dirs = torch.tensor([[float.fromhex(x) for x in row.split()] for row in (
        "0x1.24b5dcp-1 0x1.3e5c92p-2 0x1.84c2f8p-1", "-0x1.3f212ep-1 0x1.6d9e84p-1 0x1.46594ap-2",
        "0x1.2809d4p-2 0x1.488ce8p-1 -0x1.6bac72p-1")], dtype=torch.float32, device="cuda")
    total = None
    for k in range(3):
        p = s.count_crossings(pts, dirs[k].expand_as(pts).contiguous(), outputs=("pops",))["pops"]
        total = p if total is None else total + p
    return total


if __name__ == "__main__":
    main()
