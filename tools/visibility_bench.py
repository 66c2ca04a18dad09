#!/usr/bin/env python3
"""Throughput of visibility masks (rt_visibility) on the GPU, with device events.  Prints one JSON line: per workload, K and variant
ms per FRAME AND POINT -- the median of `--repeats` timed windows of `--calls` calls each, with the fastest and slowest window as the
spread.  The variants of a workload are alternated window by window.

Workloads, `--frames` (32) frames per launch along bench.py's camera path, K = 1 and 4 points near the camera (a stereo partner 0.2 to
the right, a projector above, two lights):
  panorama_atrium   a 2048x1024 equirectangular sensor inside the atrium (c4's scene)
  c2_mid            c2 from its mid camera at 1920x1080
Variants:
  visibility          (a) rt_visibility (`visible`) on planes already rendered
  detour_occluded     (b) the detour's rt_occluded launches alone, one per point, on rays prepared beforehand and not timed
  detour_occluded_binned  the same with octant binning
  detour_whole        (c) the whole detour: the rays and bounds made in torch by the rule, rt_occluded per point, the bits packed
  render_visibility   (d) Camera / Sensor.render_visibility end to end (G-buffer launch + masks)
  render_gbuffer      the G-buffer launch of (d) alone: instance + location
The detour variants run on `--detour-frames` (4) frames -- their rays take 28 bytes per pixel and point -- and are reported per frame
and point like the others.

   python tools/visibility_bench.py [--repeats 7] [--calls 3] [--frames 32] [--out profiles/visibility_line.json]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--detour-frames", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    rt = importlib.import_module("cuda-raytracing_amd")
    scenes = importlib.import_module("cuda-raytracing_amd.scenes")
    sensors = importlib.import_module("cuda-raytracing_amd.sensors")
    import bench  # noqa: E402  (scene files, parts and the camera path exactly as bench.py builds them)
    from gbuffer_bench import timed  # noqa: E402
    from ray_query_bench import product_scene  # noqa: E402
    from rolling_bench import ratio, stats  # noqa: E402
    rt.build()
    if rt.device_count() < 1:
        raise SystemExit("visibility_bench.py needs a GPU")
    h = rt.libs()[0]
    F, FD = a.frames, min(a.detour_frames, a.frames)
    st = lambda: torch.cuda.current_stream().cuda_stream    # noqa: E731
    bias = 2.0 ** -10
    out = {}

    def workload(name, scene, owner, pose):
        W, H = owner.width, owner.height
        sh = scene.device_handle
        path = np.float32(bench.camera_path(pose, F))
        planes = owner.render_gbuffer(scene, path, outputs=("instance", "location"))
        inst, loc = planes["instance"], planes["location"]
        hits = float((inst >= 0).float().mean().item())
        res = {"hit_fraction": round(hits, 4)}
        offsets = np.float32([(0.2, 0.0, 0.0), (0.0, 0.0, 0.5), (-0.6, 0.3, 0.4), (0.5, -0.4, 0.8)])
        for K in (1, 4):
            pts_host = np.ascontiguousarray(path[:, None, :3] + offsets[None, :K])          # [F, K, 3]
            pts = torch.from_numpy(pts_host).cuda()
            vis = torch.empty((F, H, W), dtype=torch.int32, device="cuda")
            masks = rt.RtVisibility(visible=vis.data_ptr())

            def visibility():
                rt.check(h.rt_visibility(sh, inst.data_ptr(), loc.data_ptr(), None, W, H, F, pts.data_ptr(), K, bias, C.byref(masks), st(), 0),
                         "rt_visibility")

            # the detour's rays by the rule, [K][FD, H, W]: prepared beforehand for (b), made inside the clock for (c)
            def make_rays(k):
                L = pts[:FD, k].reshape(FD, 1, 1, 3).expand(FD, H, W, 3).contiguous()
                v = loc[:FD] - L
                tmax = torch.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2]) * (1.0 - bias)
                return L, v, tmax

            rays = [make_rays(k) for k in range(K)]
            n = FD * H * W
            occ = torch.empty((FD, H, W), dtype=torch.uint8, device="cuda")
            ws_bytes = int(h.rt_trace_workspace_bytes(n))
            ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")

            def occluded(r, binned):
                rt.check(h.rt_occluded(sh, r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), n, occ.data_ptr(), ws.data_ptr() if binned else None,
                                       ws_bytes if binned else 0, st(), 0), "rt_occluded")

            def detour_occluded():
                for r in rays:
                    occluded(r, False)

            def detour_binned():
                for r in rays:
                    occluded(r, True)

            def detour_whole():
                word = torch.zeros((FD, H, W), dtype=torch.int32, device="cuda")
                hit = inst[:FD] >= 0
                for k in range(K):
                    occluded(make_rays(k), False)
                    word |= ((occ == 0) & hit).to(torch.int32) << k
                return word

            def render_visibility():
                owner.render_visibility(scene, pts_host, path, bias=bias)

            def render_gbuffer():
                owner.render_gbuffer(scene, path, outputs=("instance", "location"))

            r = stats(timed({"visibility": (visibility, F * K), "detour_occluded": (detour_occluded, FD * K),
                             "detour_occluded_binned": (detour_binned, FD * K), "detour_whole": (detour_whole, FD * K),
                             "render_visibility": (render_visibility, F * K), "render_gbuffer": (render_gbuffer, F * K)}, a.repeats, a.calls))
            torch.cuda.synchronize()
            # the two ways agree on the frames the detour covers
            visibility()
            same = bool((detour_whole() == vis[:FD]).all().item())
            r["detour_equals_visibility"] = same
            r["visible_fraction_of_hits"] = round(float(((vis != 0) & (inst >= 0)).float().sum().item() / max(1.0, float((inst >= 0).sum().item()))), 4)
            r["occluded_over_visibility"] = ratio(r, "detour_occluded", "visibility")              # (b) / (a): > 1 = the call is faster
            r["occluded_binned_over_visibility"] = ratio(r, "detour_occluded_binned", "visibility")
            r["whole_detour_over_visibility"] = ratio(r, "detour_whole", "visibility")             # (c) / (a)
            r["masks_share_of_render_visibility"] = round((r["render_visibility"]["ms"] - r["render_gbuffer"]["ms"]) / r["render_visibility"]["ms"], 4)
            res["K%d" % K] = r
            del rays, occ, ws, vis
        out[name] = res

    s = product_scene("c4")
    pano = rt.Sensor(sensors.equirectangular(2048, 1024))
    workload("panorama_atrium", s, pano, scenes.C4["cam_pose"])
    pano.close()
    s.close()
    s = product_scene("c2")
    cam = rt.Camera(1920, 1080, scenes.scaled_K(1920), scenes.D_REF)
    workload("c2_mid", s, cam, scenes.C2_CAMERAS["mid"])
    cam.close()
    s.close()
    result = {"metric": "visibility_ms_per_frame_and_point", "unit": "ms per frame and point", "repeats": a.repeats, "calls": a.calls,
              "frames_per_launch": F, "detour_frames": FD, "bias": bias, "code_hash": rt.library_hash(), "workloads": out}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
