#!/usr/bin/env python3
"""Throughput of the plane sections (Scene.count_sections / rt_section_offsets + rt_list_sections) on the GPU, in one process, with
device events.  Prints one JSON line: per workload the rate in Mqueries/s (1e6 planes per second) and ms per call -- the median of
`--repeats` timed windows of `--calls` calls each, with the fastest and slowest window as the spread -- the mean pops and the pairs per
plane.  The variants of a workload are alternated window by window.  All on c2 (blob70k, an identity instance):

  (a) 4096 random planes through c2's box: `any`, `count`, `offsets+fill` (CSR with segments, into preallocated outputs), against the
      workaround they replace: count_intersecting / rt_intersecting_offsets + rt_list_intersecting on two triangles that cover each
      plane's cut of the scene box (8192 query triangles)
  (b) 256 parallel slices along z (the slicer's shape: four waves, the known weak case): `any`, `count`, `offsets+fill`
  (c) 1 M planes that miss the scene: `any`, `count`, `offsets+fill`

   python tools/section_bench.py [--repeats 7] [--calls 5] [--out file]"""
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
    """Device buffers for one set of queries: offsets, workspace, the key fields and the segments at the CSR total.  kind: "section"
    (planes [n, 2, 3]) or "intersecting" (triangles [n, 3, 3], no skip_instance)"""

    def __init__(self, s, kind, queries):
        import torch
        self.s, self.kind, self.q, self.n = s, kind, queries, queries.shape[0]
        self.h = rt.libs()[0]
        self.extra = () if kind == "section" else (None,)       # (rt_*_intersecting take skip_instance after the triangles)
        self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device="cuda")
        self.ws = torch.empty(max(int(getattr(self.h, "rt_%s_offsets_workspace_bytes" % kind)(self.n)), 1), dtype=torch.uint8, device="cuda")
        self.offsets_call()
        self.total = int(self.offsets[-1].item())
        self.count_max = int((self.offsets[1:] - self.offsets[:-1]).max().item()) if self.n else 0
        self.keys = [torch.empty(max(self.total, 1), dtype=torch.int32, device="cuda") for _ in range(2)]
        self.segment = torch.empty((max(self.total, 1), 2, 3), dtype=torch.float32, device="cuda")
        if kind == "section":
            self.lst = rt.RtSectionList(instance=self.keys[0].data_ptr(), triangle=self.keys[1].data_ptr(), segment=self.segment.data_ptr())
        else:
            self.lst = rt.RtIntersectList(instance=self.keys[0].data_ptr(), triangle=self.keys[1].data_ptr(), segment=self.segment.data_ptr())

    def _st(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def offsets_call(self):
        name = "rt_%s_offsets" % self.kind
        rt.check(getattr(self.h, name)(self.s.device_handle, self.q.data_ptr(), *self.extra, self.n, self.offsets.data_ptr(),
                                       self.ws.data_ptr(), self.ws.numel(), self._st(), 0), name)

    def fill(self):
        name = "rt_list_sections" if self.kind == "section" else "rt_list_intersecting"
        rt.check(getattr(self.h, name)(self.s.device_handle, self.q.data_ptr(), *self.extra, self.n, self.offsets.data_ptr(), 0,
                                       C.byref(self.lst), self._st(), 0), name)


def covering_triangles(planes, centre, reach):
    """two world triangles per plane [n, 2, 3, 3] that cover the plane within `reach` of `centre`'s foot on it"""
    import torch
    P, N = planes[:, 0], torch.nn.functional.normalize(planes[:, 1], dim=1)
    foot = centre - ((centre - P) * N).sum(1, keepdim=True) * N
    helper = torch.zeros_like(N)
    helper[torch.arange(len(N), device=N.device), N.abs().argmin(1)] = 1.0     # the axis least along N
    u = torch.nn.functional.normalize(torch.cross(N, helper, dim=1), dim=1) * reach
    v = torch.cross(N, u, dim=1)
    c = [foot - u - v, foot + u - v, foot + u + v, foot - u + v]
    return torch.stack([torch.stack([c[0], c[1], c[2]], dim=1), torch.stack([c[0], c[2], c[3]], dim=1)], dim=1).contiguous()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("section_bench.py needs a GPU")
    result = {"metric": "section_mqps", "unit": "Mqueries/s (1e6 planes/s), ms per call, mean pops", "repeats": a.repeats, "calls": a.calls,
              "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]
    s = product_scene("c2")
    v = rt.Mesh.load_obj(bench.scene_path("c2")).dump()["tris"][:, :9].reshape(-1, 3).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    diag = float(np.linalg.norm(hi - lo))
    wls["diag_c2"] = round(diag, 4)
    g = torch.Generator(device="cuda").manual_seed(5)
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float32, device="cuda"), torch.tensor(hi, dtype=torch.float32, device="cuda")
    centre = (lo_t + hi_t) * 0.5

    def mean_pops(res):
        return round(float(res["pops"].double().mean()), 2)

    def lists(pa, r, prefix=""):
        r.update({prefix + "queries": pa.n, prefix + "total_pairs": pa.total, prefix + "mean_count": round(pa.total / max(pa.n, 1), 3),
                  prefix + "max_count": pa.count_max})

    def run(planes, n, workaround=False):
        r = {}
        pa = Prealloc(s, "section", planes)
        lists(pa, r)
        var = {"any": lambda: s.count_sections(planes, outputs=("any",)), "count": lambda: s.count_sections(planes, outputs=("count",)),
               "offsets+fill": lambda: (pa.offsets_call(), pa.fill())}
        pops = {"any": lambda: s.count_sections(planes, outputs=("any", "pops")), "count": lambda: s.count_sections(planes, outputs=("count", "pops"))}
        if workaround:
            tris = covering_triangles(planes, centre, diag).reshape(-1, 3, 3)
            pw = Prealloc(s, "intersecting", tris)
            lists(pw, r, "workaround_")
            var["workaround_count"] = lambda: s.count_intersecting(tris, outputs=("count",))
            var["workaround_offsets+fill"] = lambda: (pw.offsets_call(), pw.fill())
            pops["workaround_count"] = lambda: s.count_intersecting(tris, outputs=("count", "pops"))
        r.update(timed(var, n, a.repeats, a.calls))
        for k in var:
            r[k]["mqps"] = round(r[k].pop("grays") * 1e3, 3)   # (timed gives 1e9 per second)
        r["mean_pops"] = {k: mean_pops(f()) for k, f in pops.items()}
        return r

    # (a) random planes through the scene box, against two covering triangles per plane
    n = 4096
    P = lo_t + (hi_t - lo_t) * torch.rand((n, 3), device="cuda", generator=g)
    N = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=g), dim=1)
    wls["a_c2_random_planes_4096"] = run(torch.stack([P, N], dim=1).contiguous(), n, workaround=True)
    # (b) parallel slices along z
    m = 256
    z = lo_t[2] + (hi_t[2] - lo_t[2]) * (torch.arange(m, device="cuda", dtype=torch.float32) + 0.5) / m
    P = torch.stack([centre[0].expand(m), centre[1].expand(m), z], dim=1)
    N = torch.tensor([0.0, 0.0, 1.0], device="cuda").expand(m, 3)
    wls["b_c2_z_slices_256"] = run(torch.stack([P, N], dim=1).contiguous(), m)
    # (c) planes that miss the scene: beyond the box along their own normal
    n = 1 << 20
    u = torch.nn.functional.normalize(torch.randn((n, 3), device="cuda", generator=g), dim=1)
    P = centre + u * diag * (1.0 + torch.rand((n, 1), device="cuda", generator=g))
    wls["c_c2_missing_planes_1m"] = run(torch.stack([P, u], dim=1).contiguous(), n)
    s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
