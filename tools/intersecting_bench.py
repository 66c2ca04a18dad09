#!/usr/bin/env python3
"""Throughput of the triangle intersection queries (Scene.count_intersecting / rt_intersecting_offsets + rt_list_intersecting) on the
GPU, in one process, with device events.  Prints one JSON line: per workload the rate in Gqueries/s (1e9 query triangles per second)
and ms per call -- the median of `--repeats` timed windows of `--calls` calls each, with the fastest and slowest window as the spread
-- against closest_points on the query triangles' centroids.  The variants of a workload are alternated window by window.  The list
outputs are the keys (instance, triangle).

  (a) c2 (blob70k): its 69 936 triangles under a second pose (5 degrees about its centre, moved by 1 % of the diagonal), so that the
      copy cuts the blob: `any`, `count`, `offsets+fill` (CSR, into preallocated outputs)
  (b) 1 M random triangles with edges of 1e-3 of c2's diagonal in c2's box: the same variants
  (c) the demo scene (bench.py --workload demo): every instance's own world triangles against the scene with skip_instance = that
      instance ("what does it touch?"): the same variants
  (d) long lists: 4096 triangles with edges of half c2's diagonal through the blob's centre: `count`, `offsets+fill`

   python tools/intersecting_bench.py [--repeats 7] [--calls 5] [--out file]"""
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
    """Device buffers for one set of query triangles: offsets, workspace and the key fields at the CSR total"""

    def __init__(self, s, tris, skip):
        import torch
        self.s, self.tris, self.skip, self.n = s, tris, skip, tris.shape[0]
        self.h = rt.libs()[0]
        self.offsets = torch.empty(self.n + 1, dtype=torch.int64, device="cuda")
        self.ws = torch.empty(max(int(self.h.rt_intersecting_offsets_workspace_bytes(self.n)), 1), dtype=torch.uint8, device="cuda")
        self.offsets_call()
        self.total = int(self.offsets[-1].item())
        self.count_max = int((self.offsets[1:] - self.offsets[:-1]).max().item()) if self.n else 0
        rows = max(self.total, 1)
        self.bufs = [torch.empty(rows, dtype=torch.int32, device="cuda") for _ in range(2)]
        self.lst = rt.RtIntersectList(*[b.data_ptr() for b in self.bufs])

    def _st(self):
        import torch
        return torch.cuda.current_stream().cuda_stream

    def _skip(self):
        return None if self.skip is None else self.skip.data_ptr()

    def offsets_call(self):
        rt.check(self.h.rt_intersecting_offsets(self.s.device_handle, self.tris.data_ptr(), self._skip(), self.n, self.offsets.data_ptr(),
                                                self.ws.data_ptr(), self.ws.numel(), self._st(), 0), "rt_intersecting_offsets")

    def fill(self):
        rt.check(self.h.rt_list_intersecting(self.s.device_handle, self.tris.data_ptr(), self._skip(), self.n, self.offsets.data_ptr(), 0,
                                             C.byref(self.lst), self._st(), 0), "rt_list_intersecting")


def _rotation(axis, deg):
    ax = np.asarray(axis, np.float64)
    ax /= np.linalg.norm(ax)
    a = np.radians(deg)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


def _world(host, pose, scale, v):
    """mesh vertices v [m, 3] of an instance -> world: apply_lre(invert_lre(pose), v * scale), the host library's fp32 functions"""
    fp = C.POINTER(C.c_float)
    p = np.ascontiguousarray(pose, np.float32)
    inv = np.zeros(6, np.float32)
    host.rth_invert_lre(p.ctypes.data_as(fp), inv.ctypes.data_as(fp))
    out = np.zeros(v.shape, np.float32)
    vs = np.ascontiguousarray(v * np.asarray(scale, np.float32), np.float32)
    for j in range(len(vs)):
        host.rth_apply_lre(inv.ctypes.data_as(fp), vs[j].ctypes.data_as(fp), out[j].ctypes.data_as(fp))
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("intersecting_bench.py needs a GPU")
    result = {"metric": "intersecting_gqps", "unit": "Gqueries/s (1e9 query triangles/s), ms per call, mean pops", "repeats": a.repeats,
              "calls": a.calls, "code_hash": rt.library_hash(), "workloads": {}}
    wls = result["workloads"]

    def run(name, s, tris, skip, with_any=True):
        cen = tris.mean(dim=1).contiguous()
        pa = Prealloc(s, tris, skip)
        v = {"closest_points": lambda: s.closest_points(cen, outputs=("distance", "instance", "triangle")),
             "count": lambda: s.count_intersecting(tris, skip, outputs=("count",)),
             "offsets+fill": lambda: (pa.offsets_call(), pa.fill())}
        if with_any:
            v["any"] = lambda: s.count_intersecting(tris, skip, outputs=("any",))
        r = timed(v, tris.shape[0], a.repeats, a.calls)
        for k in v:
            r[k]["gqps"] = r[k].pop("grays")
        c = s.count_intersecting(tris, skip, outputs=("count", "pops"))
        r["queries"] = int(tris.shape[0])
        r["total_pairs"] = pa.total
        r["mean_count"] = round(pa.total / max(pa.n, 1), 3)
        r["max_count"] = pa.count_max
        r["mean_pops"] = {"closest_points": round(float(s.closest_points(cen, outputs=("pops",))["pops"].double().mean()), 2),
                          "count": round(float(c["pops"].double().mean()), 2)}
        if with_any:
            r["mean_pops"]["any"] = round(float(s.count_intersecting(tris, skip, outputs=("any", "pops"))["pops"].double().mean()), 2)
        wls[name] = r

    host = rt.libs()[1]
    # c2: the blob as an identity instance, so mesh space is world space
    s = product_scene("c2")
    v = rt.Mesh.load_obj(bench.scene_path("c2")).dump()["tris"][:, :9].reshape(-1, 3, 3).astype(np.float64)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    diag = float(np.linalg.norm(hi - lo))
    centre = (lo + hi) * 0.5
    shift = np.array([0.6, -0.3, 0.75]) / np.linalg.norm([0.6, -0.3, 0.75]) * 0.01 * diag
    moved = (v - centre) @ _rotation((1.0, 1.0, 0.3), 5.0).T + centre + shift
    run("a_c2_posed_copy", s, torch.from_numpy(moved.astype(np.float32)).cuda().contiguous(), None)
    g = torch.Generator(device="cuda").manual_seed(5)
    n = 1 << 20
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float32, device="cuda"), torch.tensor(hi, dtype=torch.float32, device="cuda")
    c = lo_t + (hi_t - lo_t) * torch.rand((n, 1, 3), device="cuda", generator=g)
    u = torch.nn.functional.normalize(torch.randn((n, 2, 3), device="cuda", generator=g), dim=-1) * (1e-3 * diag)
    run("b_c2_random_1m", s, torch.cat([c, c + u[:, :1], c + u[:, 1:]], dim=1).contiguous(), None)
    # (d) long lists: equilateral triangles of edge diag / 2 around the centre, in random planes
    m = 4096
    r = diag / 2 / np.sqrt(3.0)
    e1 = torch.nn.functional.normalize(torch.randn((m, 3), device="cuda", generator=g), dim=-1)
    e2 = torch.nn.functional.normalize(torch.linalg.cross(e1, torch.randn((m, 3), device="cuda", generator=g)), dim=-1)
    th = torch.rand((m, 1), device="cuda", generator=g) * 2 * np.pi
    ctr = torch.tensor(centre, dtype=torch.float32, device="cuda")
    verts = [ctr + r * (torch.cos(th + k * 2 * np.pi / 3) * e1 + torch.sin(th + k * 2 * np.pi / 3) * e2) for k in range(3)]
    run("d_c2_long_lists", s, torch.stack(verts, dim=1).contiguous(), None, with_any=False)
    wls["diag_c2"] = round(diag, 4)
    s.close()
    # (c) demo: each instance's own world triangles against the rest of the scene
    wl = scenes.WORKLOADS["demo"]
    _mats, objs, insts = bench.scene_parts("demo", wl, bench.scene_path("demo"))
    s = product_scene("demo")
    tris, skip = [], []
    for k, (mesh, _mat, pose, scale) in enumerate(insts):
        t = rt.Mesh.load_obj(objs[mesh]).dump()["tris"][:, :9].reshape(-1, 3)
        tris.append(_world(host, pose, scale, t).reshape(-1, 3, 3))
        skip.append(np.full(len(tris[-1]), k, np.int32))
    run("c_demo_instances_vs_rest", s, torch.from_numpy(np.concatenate(tris)).cuda().contiguous(),
        torch.from_numpy(np.concatenate(skip)).cuda().contiguous())
    s.close()
    torch.cuda.synchronize()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
