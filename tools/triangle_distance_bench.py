#!/usr/bin/env python3
"""Throughput of the triangle distance queries (Scene.closest_to_triangles) on the GPU, in one process, with device events.  Prints one
JSON line: per workload the rate in Gqueries/s (1e9 triangles per second), ms per call and mean interior nodes visited (pops) -- the
median of `--repeats` timed windows of `--calls` calls each, with the fastest and slowest window as the spread.  The variants of a
workload are alternated window by window.  All on c2 (blob70k, mid camera, 1920x1080), `--triangles` of its hit locations in pixel
order:

  (a) triangles of 1e-3 of the scene diagonal: one vertex 1e-3 of the diagonal off the surface along the normal, the other two that
      far from it in random directions; beside it the workaround, Scene.closest_to_segments on the three edges plus
      Scene.closest_points on 4 interior samples, with the share of triangles on which the nearest of its answers is farther than the
      triangle query's
  (b) (a) randomly permuted
  (c) the same first vertices with sizes 1e-2 and 1e-1 of the diagonal (the box bound's weak case)
  (d) (a) with max_distance = 1e-2 of the diagonal: the three default fields, and `within` alone (the first-candidate traversal)
  (e) the intersection half alone (outputs = intersections) on (a) and on the 1e-1 triangles

   python tools/triangle_distance_bench.py [--repeats 7] [--calls 5] [--triangles 1048576] [--out file]"""
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
    ap.add_argument("--triangles", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("triangle_distance_bench.py needs a GPU")
    W, H = 1920, 1080
    result = {"metric": "triangle_distance_gqps", "unit": "Gqueries/s (1e9 triangles/s), ms per call, mean pops", "repeats": a.repeats,
              "calls": a.calls, "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]
    outs = ("distance", "instance", "triangle")
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
    n = min(a.triangles, loc.shape[0])
    sel = torch.linspace(0, loc.shape[0] - 1, n, device="cuda").long()        # (pixel order kept, the whole frame covered)
    p0 = (loc[sel] + nrm[sel] * (1e-3 * diag)).contiguous()
    g = torch.Generator(device="cuda").manual_seed(7)
    u = torch.randn((2, n, 3), device="cuda", generator=g)
    u = u / torch.linalg.vector_norm(u, dim=2, keepdim=True)
    result["triangles"], result["diag_c2"] = n, round(diag, 4)

    def triangles(size):
        return torch.stack([p0, p0 + u[0] * (size * diag), p0 + u[1] * (size * diag)], dim=1).contiguous()

    def run(name, tris, md=None, outputs=outs, extra=None):
        v = {"closest_to_triangles": lambda: s.closest_to_triangles(tris, md, outputs=outputs)}
        v.update(extra or {})
        r = timed(v, tris.shape[0], a.repeats, a.calls)
        for k in v:
            r[k]["gqps"] = r[k].pop("grays")
        if outputs != ("intersections",):                       # (pops: of the traversal the workload runs, full or first-candidate)
            got = s.closest_to_triangles(tris, md, outputs=tuple(outputs) + ("pops",))
            r["mean_pops"] = round(float(got["pops"].double().mean()), 2)
        got = s.closest_to_triangles(tris, md, outputs=("within", "intersections"))
        r["within_frac"] = round(float((got["within"] > 0).double().mean()), 4)
        r["intersecting_frac"] = round(float((got["intersections"] > 0).double().mean()), 4)
        wls[name] = r
        return r

    small = triangles(1e-3)
    edges = torch.stack([small[:, [0, 1]], small[:, [1, 2]], small[:, [2, 0]]], dim=1).contiguous()         # [n, 3, 2, 3]
    cen = small.mean(dim=1, keepdim=True)
    samples = torch.cat([cen, (cen + small) * 0.5], dim=1).contiguous()                                     # [n, 4, 3]

    def workaround():
        s.closest_to_segments(edges, outputs=("distance",))
        s.closest_points(samples, outputs=("distance",))
    ra = run("a_c2_1e-3_pixel_order", small, extra={"segments_on_3_edges_plus_points_on_4_samples": workaround})
    tri = s.closest_to_triangles(small, outputs=("distance", "intersections"))
    wd = torch.minimum(s.closest_to_segments(edges, outputs=("distance",))["distance"].min(dim=1).values,
                       s.closest_points(samples, outputs=("distance",))["distance"].min(dim=1).values)
    free = tri["intersections"] == 0
    ra["workaround_farther_frac"] = round(float((wd > tri["distance"]).double().mean()), 4)
    # the workaround's points are points of the triangle up to rounding, so it is closer only by that rounding -- or where the triangle
    # intersects a surface, which `intersections` reports instead of the distance
    ra["workaround_closer_not_intersecting"] = int(((wd < tri["distance"]) & free).sum())
    ra["workaround_closer_not_intersecting_max_rel"] = float((((tri["distance"] - wd) / diag)[free]).max())
    ra["workaround_closer_intersecting"] = int(((wd < tri["distance"]) & ~free).sum())
    ra["intersecting"] = int((~free).sum())
    perm = torch.randperm(n, device="cuda", generator=g)
    run("b_c2_1e-3_shuffled", small[perm].contiguous())
    rc2 = run("c_c2_1e-2", triangles(1e-2))
    large = triangles(1e-1)
    rc1 = run("c_c2_1e-1", large)
    md = torch.full((n,), 1e-2 * diag, dtype=torch.float32, device="cuda")
    run("d_c2_1e-3_bounded_full", small, md)
    run("d_c2_1e-3_bounded_within_only", small, md, outputs=("within",))
    run("e_c2_1e-3_intersections_only", small, outputs=("intersections",))
    run("e_c2_1e-1_intersections_only", large, outputs=("intersections",))
    base = ra["closest_to_triangles"]["ms"]
    result["ratio_workaround_to_a"] = round(ra["segments_on_3_edges_plus_points_on_4_samples"]["ms"] / base, 2)
    result["ratio_c_1e-2_to_a"] = round(rc2["closest_to_triangles"]["ms"] / base, 2)
    result["ratio_c_1e-1_to_a"] = round(rc1["closest_to_triangles"]["ms"] / base, 2)
    s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
