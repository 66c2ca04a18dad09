#!/usr/bin/env python3
"""Throughput of the sphere sweeps (Scene.sweep_spheres) on the GPU, in one process, with device events.  Prints one JSON line: per
workload the rate in Gqueries/s (1e9 sweeps per second), ms per call, mean interior nodes visited (pops), the share of sweeps that
touch something and the share that start in contact -- the median of `--repeats` timed windows of `--calls` calls each, with the
fastest and slowest window as the spread.  The variants of a workload are alternated window by window.  All on c2 (blob70k, mid
camera, 1920x1080), `--sweeps` of its hit locations in pixel order, radius 1e-3 of the scene diagonal:

  (a) sweeps of 1e-3 of the diagonal, starting two radii off the surface along the normal, in a random direction; beside it the
      workaround, Scene.closest_points with max_distance = r on 8 samples per sweep, with the share of sweeps the sampling calls free
      that the sweep says touch, and the reverse
  (b) (a) randomly permuted
  (c) the same starts with lengths 1e-2, 1e-1 and 1 diagonal (the box bound's weak case, until the first contact is found)
  (d) `hit` alone (the first-candidate traversal) on (a) and on the sweeps of 1e-1

   python tools/sweep_bench.py [--repeats 7] [--calls 5] [--sweeps 1048576] [--out file]"""
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
    ap.add_argument("--sweeps", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("sweep_bench.py needs a GPU")
    W, H = 1920, 1080
    result = {"metric": "sweep_query_gqps", "unit": "Gqueries/s (1e9 sweeps/s), ms per call, mean pops", "repeats": a.repeats,
              "calls": a.calls, "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]
    outs = ("time", "instance", "triangle")
    s = product_scene("c2")
    cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
    cam.set_pose(scenes.C2_CAMERAS["mid"])
    o, d = cam.rays()
    hit = s.trace_rays(o, d, outputs=("instance", "location", "normal"), binning=False)
    keep = (hit["instance"] >= 0).reshape(-1)
    loc = hit["location"].reshape(-1, 3)[keep]
    nrm = hit["normal"].reshape(-1, 3)[keep]
    lo, hi = loc.min(dim=0).values, loc.max(dim=0).values
    diag = float(torch.linalg.vector_norm(hi - lo))
    n = min(a.sweeps, loc.shape[0])
    sel = torch.linspace(0, loc.shape[0] - 1, n, device="cuda").long()        # (pixel order kept, the whole frame covered)
    r = 1e-3 * diag
    p0 = (loc[sel] + nrm[sel] * (2.0 * r)).contiguous()
    g = torch.Generator(device="cuda").manual_seed(7)
    u = torch.randn((n, 3), device="cuda", generator=g)
    u = u / torch.linalg.vector_norm(u, dim=1, keepdim=True)
    rad = torch.full((n,), r, dtype=torch.float32, device="cuda")
    result["sweeps"], result["diag_c2"], result["radius"] = n, round(diag, 4), r

    def sweeps(length):
        return torch.stack([p0, p0 + u * (length * diag)], dim=1).contiguous()

    def run(name, segs, outputs=outs, extra=None):
        v = {"sweep_spheres": lambda: s.sweep_spheres(segs, rad, outputs=outputs)}
        v.update(extra or {})
        res = timed(v, segs.shape[0], a.repeats, a.calls)
        for k in v:
            res[k]["gqps"] = res[k].pop("grays")
        got = s.sweep_spheres(segs, rad, outputs=tuple(outputs) + ("pops",))     # (pops: of the traversal the workload runs)
        res["mean_pops"] = round(float(got["pops"].double().mean()), 2)
        got = s.sweep_spheres(segs, rad, outputs=("time", "hit"))
        res["hit_frac"] = round(float((got["hit"] > 0).double().mean()), 4)
        res["start_in_contact_frac"] = round(float(((got["hit"] > 0) & (got["time"] == 0)).double().mean()), 4)
        wls[name] = res
        return res

    short = sweeps(1e-3)
    t8 = torch.linspace(0.0, 1.0, 8, device="cuda").reshape(1, 8, 1)
    samples = (short[:, :1] + t8 * (short[:, 1:] - short[:, :1])).contiguous()        # [n, 8, 3]
    rad8 = rad.reshape(n, 1).expand(n, 8).contiguous()
    ra = run("a_c2_1e-3_pixel_order", short,
             extra={"closest_points_8_samples": lambda: s.closest_points(samples, rad8, outputs=("distance", "instance"))})
    swept = s.sweep_spheres(short, rad, outputs=("hit",))["hit"] > 0
    sampled = (s.closest_points(samples, rad8, outputs=("instance",))["instance"] >= 0).any(dim=1)
    ra["sweep_hit_samples_free_frac"] = round(float((swept & ~sampled).double().mean()), 4)
    ra["samples_hit_sweep_free"] = int((sampled & ~swept).sum())
    perm = torch.randperm(n, device="cuda", generator=g)
    run("b_c2_1e-3_shuffled", short[perm].contiguous())
    rc2 = run("c_c2_1e-2", sweeps(1e-2))
    long = sweeps(1e-1)
    rc1 = run("c_c2_1e-1", long)
    rc0 = run("c_c2_1", sweeps(1.0))
    run("d_c2_1e-3_hit_only", short, outputs=("hit",))
    run("d_c2_1e-1_hit_only", long, outputs=("hit",))
    base = ra["sweep_spheres"]["ms"]
    result["ratio_c_1e-2_to_a"] = round(rc2["sweep_spheres"]["ms"] / base, 2)
    result["ratio_c_1e-1_to_a"] = round(rc1["sweep_spheres"]["ms"] / base, 2)
    result["ratio_c_1_to_a"] = round(rc0["sweep_spheres"]["ms"] / base, 2)
    s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
