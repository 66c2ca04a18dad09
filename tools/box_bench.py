#!/usr/bin/env python3
"""Throughput of the box queries (Scene.count_in_boxes / rt_box_offsets + rt_list_in_boxes / Scene.occupancy_grid) on the GPU, in one
process, with device events.  Prints one JSON line: per workload the rate in Gqueries/s (1e9 boxes per second) and ms per call -- the
median of `--repeats` timed windows of `--calls` calls each, with the fastest and slowest window as the spread -- and the mean pops.
The variants of a workload are alternated window by window.  All on c2 (blob70k, an identity instance):

  (a) 1 M random cubes with an edge of 1e-3 of c2's diagonal in c2's box: `any`, `count`, `offsets+fill` (CSR, into preallocated
      outputs), against count_intersecting on triangles of the same size and closest_points on the centres
  (b) a 256^3 occupancy grid over the scene box: the grid call (`grid_occupied`, `grid_count`) against count_in_boxes on the same
      cells staged as an array (`boxes_any`, `boxes_count`)
  (c) 4096 cubes half the diagonal across around the centre: `count`, `offsets+fill` (the weak case: long lists, poor pruning)

   python tools/box_bench.py [--repeats 7] [--calls 5] [--grid 256] [--out file]"""
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
import bench  # noqa: E402  (scene files and parts exactly as bench.py builds them)
from ray_query_bench import product_scene, timed  # noqa: E402  (the same scenes and timing as the ray-query line)


class Prealloc:
    """Device buffers for one set of boxes: offsets, workspace and the key fields at the CSR total"""

    def __init__(self, s, boxes):
        import torch
        self.s, self.boxes, self.n = s, boxes, boxes.shape[0]
        self.h = rt.libs()[0]
        self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device="cuda")
        self.ws = torch.empty(max(int(self.h.rt_box_offsets_workspace_bytes(self.n)), 1), dtype=torch.uint8, device="cuda")
        self.offsets_call()
        self.total = int(self.offsets[-1].item())
        self.count_max = int((self.offsets[1:] - self.offsets[:-1]).max().item()) if self.n else 0
        self.bufs = [torch.empty(max(self.total, 1), dtype=torch.int32, device="cuda") for _ in range(2)]
        self.lst = rt.RtBoxList(*[b.data_ptr() for b in self.bufs])

    def _st(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def offsets_call(self):
        rt.check(self.h.rt_box_offsets(self.s.device_handle, self.boxes.data_ptr(), self.n, self.offsets.data_ptr(), self.ws.data_ptr(),
                                       self.ws.numel(), self._st(), 0), "rt_box_offsets")

    def fill(self):
        rt.check(self.h.rt_list_in_boxes(self.s.device_handle, self.boxes.data_ptr(), self.n, self.offsets.data_ptr(), 0, C.byref(self.lst),
                                         self._st(), 0), "rt_list_in_boxes")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("box_bench.py needs a GPU")
    result = {"metric": "box_gqps", "unit": "Gqueries/s (1e9 boxes/s), ms per call, mean pops", "repeats": a.repeats, "calls": a.calls,
              "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]
    s = product_scene("c2")
    v = rt.Mesh.load_obj(bench.scene_path("c2")).dump()["tris"][:, :9].reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    diag = float(np.linalg.norm(hi - lo))
    centre = (lo + hi) * 0.5
    wls["diag_c2"] = round(diag, 4)
    g = torch.Generator(device="cuda").manual_seed(5)
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float32, device="cuda"), torch.tensor(hi, dtype=torch.float32, device="cuda")

    def mean_pops(res):
        return round(float(res["pops"].double().mean()), 2)

    def lists(boxes, r):
        pa = Prealloc(s, boxes)
        r.update(queries=int(boxes.shape[0]), total_pairs=pa.total, mean_count=round(pa.total / max(pa.n, 1), 3), max_count=pa.count_max)
        return pa

    # (a) 1 M small cubes, against triangles of the same size and the centres' closest points
    n = 1 << 20
    e = 1e-3 * diag
    c = lo_t + (hi_t - lo_t) * torch.rand((n, 3), device="cuda", generator=g)
    boxes = torch.stack([c - e / 2, c + e / 2], dim=1).contiguous()
    u = torch.nn.functional.normalize(torch.randn((n, 2, 3), device="cuda", generator=g), dim=-1) * e
    tris = torch.cat([c[:, None], c[:, None] + u[:, :1], c[:, None] + u[:, 1:]], dim=1).contiguous()
    r = {}
    pa = lists(boxes, r)
    var = {"any": lambda: s.count_in_boxes(boxes, outputs=("any",)), "count": lambda: s.count_in_boxes(boxes, outputs=("count",)),
           "offsets+fill": lambda: (pa.offsets_call(), pa.fill()),
           "count_intersecting": lambda: s.count_intersecting(tris, outputs=("count",)),
           "closest_points": lambda: s.closest_points(c, outputs=("distance", "instance", "triangle"))}
    r.update(timed(var, n, a.repeats, a.calls))
    for k in var:
        r[k]["gqps"] = r[k].pop("grays")
    r["mean_pops"] = {"any": mean_pops(s.count_in_boxes(boxes, outputs=("any", "pops"))),
                      "count": mean_pops(s.count_in_boxes(boxes, outputs=("count", "pops"))),
                      "count_intersecting": mean_pops(s.count_intersecting(tris, outputs=("count", "pops"))),
                      "closest_points": mean_pops(s.closest_points(c, outputs=("pops",)))}
    wls["a_c2_small_cubes_1m"] = r
    del boxes, tris, u, c, pa
    # (b) the occupancy grid against the same cells staged as boxes
    G = a.grid
    span = (hi - lo).astype(np.float32)
    origin = (lo - 0.01 * span).astype(np.float32)
    spacing = (1.02 * span / G).astype(np.float32)
    edges = [torch.tensor(origin[k] + np.arange(G + 1, dtype=np.float32) * spacing[k], dtype=torch.float32, device="cuda") for k in range(3)]
    cells = torch.empty((G, G, G, 2, 3), dtype=torch.float32, device="cuda")
    for k in range(3):
        shape = [1, 1, 1]
        shape[2 - k] = G
        cells[..., 0, k] = edges[k][:-1].reshape(shape)
        cells[..., 1, k] = edges[k][1:].reshape(shape)
    var = {"grid_occupied": lambda: s.occupancy_grid(origin, spacing, (G, G, G), outputs=("occupied",)),
           "boxes_any": lambda: s.count_in_boxes(cells, outputs=("any",)),
           "grid_count": lambda: s.occupancy_grid(origin, spacing, (G, G, G), outputs=("count",)),
           "boxes_count": lambda: s.count_in_boxes(cells, outputs=("count",))}
    r = timed(var, G ** 3, a.repeats, a.calls)
    for k in var:
        r[k]["gqps"] = r[k].pop("grays")
    cg, cb = s.occupancy_grid(origin, spacing, (G, G, G), outputs=("count",))["count"], s.count_in_boxes(cells, outputs=("count", "pops"))
    r.update(cells=G ** 3, grid_equals_boxes=bool(torch.equal(cg, cb["count"])), occupied_cells=int((cg > 0).sum().item()),
             total_pairs=int(cg.sum(dtype=torch.int64).item()), mean_pops={"boxes_count": mean_pops(cb)})
    wls["b_c2_grid_%d" % G] = r
    del cells, cg, cb
    # (c) long lists: cubes half the diagonal across, centred within a tenth of the diagonal of the centre
    m = 4096
    ctr = torch.tensor(centre, dtype=torch.float32, device="cuda") + (torch.rand((m, 3), device="cuda", generator=g) - 0.5) * (0.1 * diag)
    big = torch.stack([ctr - diag / 4, ctr + diag / 4], dim=1).contiguous()
    r = {}
    pb = lists(big, r)
    var = {"count": lambda: s.count_in_boxes(big, outputs=("count",)), "offsets+fill": lambda: (pb.offsets_call(), pb.fill())}
    r.update(timed(var, m, a.repeats, a.calls))
    for k in var:
        r[k]["gqps"] = r[k].pop("grays")
    r["mean_pops"] = {"count": mean_pops(s.count_in_boxes(big, outputs=("count", "pops")))}
    wls["c_c2_big_cubes_4096"] = r
    s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
