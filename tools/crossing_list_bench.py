#!/usr/bin/env python3
"""Throughput of the crossing lists (Scene.list_crossings: rt_crossing_offsets + rt_list_crossings) on the GPU, in one process, with
device events.  Prints one JSON line: per workload the rate in Gqueries/s (1e9 rays per second) and ms per call -- the median of
`--repeats` timed windows of `--calls` calls each, with the fastest and slowest window as the spread -- against count_crossings on
the same rays.  The variants of a workload are alternated window by window.

  (a) c2 (blob70k, mid camera, 1920x1080) camera rays, CSR: `offsets` (rt_crossing_offsets alone), `fill` (rt_list_crossings alone
      into preallocated outputs, every field), `list_crossings` (the Python call: offsets, the one read of the total, allocation,
      fill, ray index)
  (b) the same rays in fixed rooms: max_hits = 4 and max_hits = 1 (every field)
  (c) the demo scene's camera rays, CSR (offsets + fill, preallocated)
  (d) segments between c2 surface points (tmax 1), CSR (offsets + fill, preallocated)
  (e) a stack of 1200 parallel quads (2400 triangles): 64 K rays crossing 1200 each, CSR (offsets + fill) and max_hits = 4 --
      the worst case of the insertion, every hit arriving in tree order

   python tools/crossing_list_bench.py [--repeats 7] [--calls 5] [--out file]"""
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
from ray_query_bench import product_scene, timed  # noqa: E402  (the same scenes and timing as the ray-query line)

FIELDS = ("t", "instance", "triangle", "sign", "barycentric", "uv", "point")


class Prealloc:
    """Device buffers for one set of rays: offsets, workspace and every output field at the CSR total (or n*K)"""

    def __init__(self, s, o, d, tmax=None):
        import torch
        self.s, self.o, self.d, self.tmax, self.n = s, o, d, tmax, o.shape[0]
        self.h = rt.libs()[0]
        self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device="cuda")
        self.ws = torch.empty(max(int(self.h.rt_crossing_offsets_workspace_bytes(self.n)), 1), dtype=torch.uint8, device="cuda")
        self.offsets_call()
        self.total = int(self.offsets[-1].item())
        self.count = torch.empty(self.n, dtype=torch.int32, device="cuda")
        self.bufs = {}

    def outs(self, rows):
        import torch
        if rows not in self.bufs:
            shp = dict(t=(), instance=(), triangle=(), sign=(), barycentric=(2,), uv=(2,), point=(3,))
            dt = dict(t=torch.float32, instance=torch.int32, triangle=torch.int32, sign=torch.int8, barycentric=torch.float32,
                      uv=torch.float32, point=torch.float32)
            b = {k: torch.empty((max(rows, 1),) + shp[k], dtype=dt[k], device="cuda") for k in FIELDS}
            self.bufs[rows] = (b, rt.RtCrossingList(*[b[k].data_ptr() for k in FIELDS], self.count.data_ptr()))
        return self.bufs[rows][1]

    def _ins(self):
        import torch
        return (self.o.data_ptr(), self.d.data_ptr(), None if self.tmax is None else self.tmax.data_ptr(),
                torch.cuda.current_stream().cuda_stream)

    def offsets_call(self):
        o, d, tm, st = self._ins()
        rt.check(self.h.rt_crossing_offsets(self.s.device_handle, o, d, tm, self.n, self.offsets.data_ptr(), self.ws.data_ptr(),
                                            self.ws.numel(), st, 0), "rt_crossing_offsets")

    def fill(self, k=None):
        o, d, tm, st = self._ins()
        lst = self.outs(self.total if k is None else self.n * k)
        rt.check(self.h.rt_list_crossings(self.s.device_handle, o, d, tm, self.n, None if k else self.offsets.data_ptr(), k or 0,
                                          C.byref(lst), st, 0), "rt_list_crossings")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("crossing_list_bench.py needs a GPU")
    W, H = 1920, 1080
    result = {"metric": "crossing_list_gqps", "unit": "Gqueries/s (1e9 rays/s), ms per call", "repeats": a.repeats, "calls": a.calls,
              "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]

    def run(name, variants, n, pa):
        r = timed(variants, n, a.repeats, a.calls)
        for k in variants:
            r[k]["gqps"] = r[k].pop("grays")
        r["queries"] = int(n)
        r["total_hits"] = pa.total
        r["mean_count"] = round(pa.total / max(n, 1), 3)
        r["max_count"] = int(pa.count_max)
        wls[name] = r

    def prep(s, o, d, tmax=None):
        pa = Prealloc(s, o, d, tmax)
        pa.count_max = int(s.count_crossings(o, d, tmax, outputs=("count",))["count"].max()) if o.shape[0] else 0
        return pa

    def count(s, o, d, tmax=None):
        return lambda: s.count_crossings(o, d, tmax, outputs=("count",))

    for workload, pose in (("c2", scenes.C2_CAMERAS["mid"]), ("demo", scenes.DEMO["cam_pose"])):
        s = product_scene(workload)
        cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
        cam.set_pose(pose)
        o, d = cam.rays()
        o, d = o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()
        pa = prep(s, o, d)
        if workload == "c2":
            run("a_c2_camera_rays_csr", {"count_crossings": count(s, o, d), "offsets": pa.offsets_call, "fill": pa.fill,
                                         "offsets+fill": lambda: (pa.offsets_call(), pa.fill()),
                                         "list_crossings": lambda: s.list_crossings(o, d)}, o.shape[0], pa)
            run("b_c2_camera_rays_fixed", {"count_crossings": count(s, o, d), "max_hits_4": lambda: pa.fill(4),
                                           "max_hits_1": lambda: pa.fill(1)}, o.shape[0], pa)
            hit = s.trace_rays(o, d, outputs=("instance", "location"), binning=False)
            loc = hit["location"][hit["instance"] >= 0].contiguous()
            g = torch.Generator(device="cuda").manual_seed(5)
            m = min(loc.shape[0], 1 << 20)
            ia = torch.randint(0, loc.shape[0], (m,), device="cuda", generator=g)
            ib = torch.randint(0, loc.shape[0], (m,), device="cuda", generator=g)
            so, sdir = loc[ia].contiguous(), (loc[ib] - loc[ia]).contiguous()
            tm = torch.ones(m, dtype=torch.float32, device="cuda")
            ps = prep(s, so, sdir, tm)
            run("d_c2_segments_csr", {"count_crossings": count(s, so, sdir, tm), "offsets+fill": lambda: (ps.offsets_call(), ps.fill())},
                m, ps)
        else:
            run("c_demo_camera_rays_csr", {"count_crossings": count(s, o, d), "offsets+fill": lambda: (pa.offsets_call(), pa.fill())},
                o.shape[0], pa)
        s.close()

    # (e) 1200 parallel quads, shuffled in z so that tree order is not t order
    rng = np.random.default_rng(3)
    zs = rng.permutation(1200).astype(np.float32) * np.float32(0.01)
    v = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], np.float32)
    tris = []
    for z in zs:                                                # tris18: v0 v1 v2, normal (+z), uv 0
        for f in ((0, 1, 2), (0, 2, 3)):
            tris.append(np.concatenate([np.concatenate([[v[i][0], v[i][1], z] for i in f]), [0, 0, 1], np.zeros(6)]))
    s = rt.Scene()
    s.add_material((1.0, 1.0, 1.0))
    s.add_mesh(rt.Mesh.from_triangles(np.stack(tris).astype(np.float32)))
    s.add_mesh_instance(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))
    s.upload_to_device()
    n = 1 << 16
    g = torch.Generator(device="cuda").manual_seed(9)
    o = torch.cat([0.05 + 0.9 * torch.rand((n, 2), device="cuda", generator=g), torch.full((n, 1), -1.0, device="cuda")], 1).contiguous()
    d = torch.cat([(torch.rand((n, 2), device="cuda", generator=g) - 0.5) * 0.02, torch.ones((n, 1), device="cuda")], 1).contiguous()
    pq = prep(s, o, d)
    run("e_quads_1200", {"count_crossings": count(s, o, d), "offsets+fill": lambda: (pq.offsets_call(), pq.fill()),
                         "max_hits_4": lambda: pq.fill(4)}, n, pq)
    s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
