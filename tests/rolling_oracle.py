"""The CPU oracle of rolling frames (rt_render_gbuffer_rolling / Sensor.render_rolling) and rolling clouds: per slice,
sensor_oracle.rays on that slice's part of the table with that slice's pose; the assembled rays through ONE ray_oracle.cast_rays;
`depth` and `local` through gbuffer_oracle's and point_cloud_oracle's shims (the oracle's own apply_lre) with the slice's pose; the
cloud by point_cloud_oracle's numpy compaction.  TEST INFRASTRUCTURE ONLY: no shim of its own."""
import numpy as np

import gbuffer_oracle
import point_cloud_oracle
import ray_oracle
import sensor_oracle

PLANES = gbuffer_oracle.PLANES + ("local",)
AXES = {"x": 0, "y": 1, 0: 0, 1: 1}


def slices(width, height, axis, slice_pixels):
    extent = height if AXES[axis] else width
    return -(-extent // slice_pixels)


def parts(width, height, axis, slice_pixels):
    """[(slice index, index expression of the slice's pixels in a [height, width, ...] array)]"""
    n = slices(width, height, axis, slice_pixels)
    if AXES[axis]:
        return [(s, (slice(s * slice_pixels, min(height, (s + 1) * slice_pixels)), slice(None))) for s in range(n)]
    return [(s, (slice(None), slice(s * slice_pixels, min(width, (s + 1) * slice_pixels)))) for s in range(n)]


def rays(dirs, slice_poses, axis, slice_pixels):
    """(origins, directions) [height, width, 3] of one rolling frame: slice_poses [slices, 6]"""
    dirs = np.ascontiguousarray(dirs, np.float32)
    h, w = dirs.shape[:2]
    P = np.asarray(slice_poses, np.float32)
    assert P.shape == (slices(w, h, axis, slice_pixels), 6), P.shape
    o, d = np.zeros_like(dirs), np.zeros_like(dirs)
    for s, at in parts(w, h, axis, slice_pixels):
        o[at], d[at] = sensor_oracle.rays(np.ascontiguousarray(dirs[at]), P[s])
    return o, d


def frame(scene, dirs, slice_poses, axis, slice_pixels, threads=8):
    """Every plane of PLANES of one rolling frame [height, width](, k)"""
    h, w = dirs.shape[:2]
    P = np.asarray(slice_poses, np.float32)
    o, d = rays(dirs, P, axis, slice_pixels)
    ref = ray_oracle.cast_rays(scene, o, d, threads=threads)
    out = {k: ref[k] for k in gbuffer_oracle.PLANES if k != "depth"}
    depth = np.zeros((h, w), np.float32)
    local = np.zeros((h, w, 3), np.float32)
    for s, at in parts(w, h, axis, slice_pixels):
        inst = np.ascontiguousarray(ref["instance"][at])
        loc = np.ascontiguousarray(ref["location"][at])
        depth[at] = gbuffer_oracle.depth(P[s], loc, inst)
        local[at] = np.where((inst >= 0)[..., None], point_cloud_oracle.apply_lre(P[s], loc), np.float32(0.0))
    out["depth"], out["local"] = depth, local
    return out


def frames(scene, dirs, poses, axis, slice_pixels, threads=8):
    """[count, height, width](, k) planes: poses [count, slices, 6]"""
    per = [frame(scene, dirs, p, axis, slice_pixels, threads) for p in np.asarray(poses, np.float32)]
    return {k: np.stack([f[k] for f in per]) for k in PLANES}


def cloud(planes, min_range=0.0, max_range=np.inf, mask=None):
    """point_cloud_oracle.cloud of rolling planes: every field by its numpy compaction, `local` the compacted `local` plane (the
    pose of each point's slice is already in it)"""
    count = planes["t"].shape[0]
    out = point_cloud_oracle.cloud(planes, np.zeros((count, 6), np.float32), min_range, max_range, mask)
    out["local"] = planes["local"][out["kept"]]
    return out
