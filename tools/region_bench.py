#!/usr/bin/env python3
"""Throughput of the region queries (Scene.count_in_regions / rt_region_offsets + rt_list_in_regions) on the GPU, in one process, with
device events.  Prints one JSON line: per workload the rate in Mqueries/s (1e6 regions per second) and ms per call -- the median of
`--repeats` timed windows of `--calls` calls each, with the fastest and slowest window as the spread -- the mean pops and the pairs per
region.  The variants of a workload are alternated window by window.  All on c2 (blob70k, an identity instance), six planes a region:

  (a) 1 M random oriented cubes of 1e-3 of the diagonal: `any`, `count`, `count+inside`, `offsets+fill` (CSR with the inside flags,
      into preallocated outputs), against the workaround they replace: count_in_boxes on the cubes' world-aligned bounding boxes, which
      returns a superset that the caller still has to test
  (b) 4096 frusta of a 64 x 64 tiling of the c2 mid camera's view, through the eye and the pixel rays at the tiles' corners: `any`,
      `count`, `count+inside`, `offsets+fill`
  (c) 4096 oriented boxes half the diagonal across (the known weak case: every triangle in a large volume is tested): `any`, `count`,
      `count+inside`, `offsets+fill`

   python tools/region_bench.py [--repeats 7] [--calls 5] [--out file]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
rt = importlib.import_module("cuda-raytracing_amd")
scenes = importlib.import_module("cuda-raytracing_amd.scenes")
import bench  # noqa: E402  (scene files and parts exactly as bench.py builds them)
from ray_query_bench import product_scene, timed  # noqa: E402  (the same scenes and timing as the ray-query line)


class Prealloc:
    """Device buffers for one set of regions [n, K, 2, 3]: offsets, workspace, the key fields and the inside flags at the CSR total"""

    def __init__(self, s, regions):
        import torch
        self.s, self.q, self.n, self.K = s, regions, regions.shape[0], regions.shape[1]
        self.h = rt.libs()[0]
        self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device="cuda")
        self.ws = torch.empty(max(int(self.h.rt_region_offsets_workspace_bytes(self.n)), 1), dtype=torch.uint8, device="cuda")
        self.offsets_call()
        self.total = int(self.offsets[-1].item())
        self.count_max = int((self.offsets[1:] - self.offsets[:-1]).max().item()) if self.n else 0
        self.keys = [torch.empty(max(self.total, 1), dtype=torch.int32, device="cuda") for _ in range(2)]
        self.flag = torch.empty(max(self.total, 1), dtype=torch.uint8, device="cuda")
        self.lst = rt.RtRegionList(instance=self.keys[0].data_ptr(), triangle=self.keys[1].data_ptr(), inside=self.flag.data_ptr())

    def _st(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def offsets_call(self):
        rt.check(self.h.rt_region_offsets(self.s.device_handle, self.q.data_ptr(), self.n, self.K, self.offsets.data_ptr(),
                                          self.ws.data_ptr(), self.ws.numel(), self._st(), 0), "rt_region_offsets")

    def fill(self):
        rt.check(self.h.rt_list_in_regions(self.s.device_handle, self.q.data_ptr(), self.n, self.K, self.offsets.data_ptr(), 0,
                                           C.byref(self.lst), self._st(), 0), "rt_list_in_regions")


def random_frames(n, g):
    """n random rotations [n, 3, 3] (rows orthonormal), from normalised random quaternions"""
    import torch
    q = torch.nn.functional.normalize(torch.randn((n, 4), device="cuda", generator=g), dim=1)
    w, x, y, z = q.unbind(1)
    return torch.stack([torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                        torch.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                        torch.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1).contiguous()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("region_bench.py needs a GPU")
    result = {"metric": "region_mqps", "unit": "Mqueries/s (1e6 regions/s), ms per call, mean pops", "repeats": a.repeats, "calls": a.calls,
              "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]
    s = product_scene("c2")
    v = rt.Mesh.load_obj(bench.scene_path("c2")).dump()["tris"][:, :9].reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    diag = float(np.linalg.norm(hi - lo))
    wls["diag_c2"] = round(diag, 4)
    g = torch.Generator(device="cuda").manual_seed(5)
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float32, device="cuda"), torch.tensor(hi, dtype=torch.float32, device="cuda")

    def mean_pops(res):
        return round(float(res["pops"].double().mean()), 2)

    def run(regions, n, boxes=None):
        r = {}
        pa = Prealloc(s, regions)
        r.update({"queries": pa.n, "planes": pa.K, "total_pairs": pa.total, "mean_count": round(pa.total / max(pa.n, 1), 3), "max_count": pa.count_max})
        r["mean_inside"] = round(float(s.count_in_regions(regions, outputs=("inside",))["inside"].double().mean()), 3)
        var = {"any": lambda: s.count_in_regions(regions, outputs=("any",)), "count": lambda: s.count_in_regions(regions, outputs=("count",)),
               "count+inside": lambda: s.count_in_regions(regions, outputs=("count", "inside")),
               "offsets+fill": lambda: (pa.offsets_call(), pa.fill())}
        pops = {"any": lambda: s.count_in_regions(regions, outputs=("any", "pops")),
                "count": lambda: s.count_in_regions(regions, outputs=("count", "pops"))}
        if boxes is not None:
            var["workaround_count_in_boxes"] = lambda: s.count_in_boxes(boxes, outputs=("count",))
            pops["workaround_count_in_boxes"] = lambda: s.count_in_boxes(boxes, outputs=("count", "pops"))
            r["workaround_mean_count"] = round(float(s.count_in_boxes(boxes, outputs=("count",))["count"].double().mean()), 3)
        r.update(timed(var, n, a.repeats, a.calls))
        for k in var:
            r[k].pop("grays")                                   # (1e9 per second, rounded too coarsely for the large regions)
            r[k]["mqps"] = round(n / r[k]["ms"] / 1e3, 4)
        r["mean_pops"] = {k: mean_pops(f()) for k, f in pops.items()}
        print("workload done: " + json.dumps(r), file=sys.stderr, flush=True)    # (kept if a later workload is cut short)
        return r

    def cubes(n, side):
        c = lo_t + (hi_t - lo_t) * torch.rand((n, 3), device="cuda", generator=g)
        q = random_frames(n, g)
        half = torch.full((n, 3), 0.5 * side, dtype=torch.float32, device="cuda")
        reach = (q.abs() * half[:, :, None]).sum(1)             # the world-aligned bounding box of the rotated cube
        return rt.regions_from_obbs(c, q, half).contiguous(), torch.stack([c - reach, c + reach], 1).contiguous()

    # (a) small oriented cubes, beside count_in_boxes on their bounding boxes
    n = 1 << 20
    regions, boxes = cubes(n, 1e-3 * diag)
    wls["a_c2_oriented_cubes_1e-3_1m"] = run(regions, n, boxes)
    del regions, boxes
    # (b) the frusta of a 64 x 64 tiling of the mid camera's view
    cam = rt.Camera(scenes.C2["width"], scenes.C2["height"], scenes.scaled_K(scenes.C2["width"]), scenes.D_REF)
    cam.set_pose(scenes.C2_CAMERAS["mid"])
    o, d = cam.rays()
    xs = torch.round(torch.arange(65, device="cuda") * (cam.width - 1) / 64).long()
    ys = torch.round(torch.arange(65, device="cuda") * (cam.height - 1) / 64).long()
    dg = d[ys][:, xs]                                           # [65, 65, 3] the pixel rays at the tiles' corners
    eye = o[0, 0].expand(64 * 64, 3).contiguous()
    corner = torch.stack([dg[:-1, :-1], dg[:-1, 1:], dg[1:, 1:], dg[1:, :-1]], 2).reshape(-1, 4, 3)
    centre = torch.nn.functional.normalize(corner.sum(1), dim=1)
    near, far = 1e-3 * diag, 4.0 * diag

    def frusta(cn):
        return rt.regions_from_frusta(eye, (eye[:, None] + cn).contiguous(), near, far).contiguous()
    regions = frusta(corner)
    probe = eye + centre * diag                                 # a point on each tile's middle ray: inside when the corners run the right way
    if not bool((((probe[:, None] - regions[:, :, 0]) * regions[:, :, 1]).sum(2) > 0).all()):
        regions = frusta(corner.flip(1))
    assert bool((((probe[:, None] - regions[:, :, 0]) * regions[:, :, 1]).sum(2) > 0).all()), "the tiles' corners are not convex seen from the eye"
    wls["b_c2_mid_camera_frusta_64x64"] = run(regions, 64 * 64)
    # (c) large oriented boxes
    n = 4096
    regions, _boxes = cubes(n, 0.5 * diag)
    wls["c_c2_oriented_boxes_half_diag_4096"] = run(regions, n)
    s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
