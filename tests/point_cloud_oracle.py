"""The CPU oracle of point clouds (rt_point_cloud_offsets + rt_point_cloud_fill / Camera.point_cloud / Sensor.point_cloud): the
keep rule, the (frame, y, x) order, the offsets and every field in numpy from G-buffer planes -- gbuffer_oracle.frames' or
sensor_oracle.frames' for the reference cloud, the library's own for the compaction test -- with `local` through
tests/point_cloud_oracle.c, which applies the oracle's own apply_lre.  TEST INFRASTRUCTURE ONLY.  Built like tests/gbuffer_oracle.py."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "point_cloud_oracle.c")
DEPS = (SRC, os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libpoint_cloud_oracle.so")
FIELDS = ("range", "pixel", "frame", "instance", "triangle", "position", "local", "normal", "uv")
_lib = None
_lock = threading.Lock()


def _stale():
    return not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in DEPS)


def build():
    """Compile the shim when it is missing or stale (into a temporary name first: concurrent builders never load half a file)."""
    if _stale():
        tmp = "%s.%d.tmp" % (SO, os.getpid())
        subprocess.run([os.environ.get("CC", "gcc")] + FLAGS + ["-o", tmp, SRC, "-lm"], check=True)
        os.replace(tmp, SO)
    return SO


def lib():
    global _lib
    with _lock:
        if _lib is None:
            L = C.CDLL(build())
            L.orcx_cloud_local.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            L.orcx_cloud_local.restype = None
            _lib = L
    return _lib


def apply_lre(pose, location):
    """apply_lre(pose, location), all three components: location [..., 3] float32 -> [..., 3]"""
    loc = np.ascontiguousarray(location, np.float32)
    assert loc.shape[-1] == 3
    P = np.ascontiguousarray(pose, np.float32)
    assert P.shape == (6,)
    out = np.zeros_like(loc)
    lib().orcx_cloud_local(P.ctypes.data, loc.size // 3, loc.ctypes.data, out.ctypes.data)
    return out


def keep(planes, min_range=0.0, max_range=np.inf, mask=None):
    """bool [count, height, width]: the keep rule on planes t and instance, float32 comparisons, the mask shared by the frames"""
    t = planes["t"]
    assert t.dtype == np.float32
    with np.errstate(invalid="ignore"):
        k = (planes["instance"] >= 0) & (t >= np.float32(min_range)) & (t <= np.float32(max_range))
    if mask is not None:
        k = k & (np.asarray(mask).astype(np.uint8) != 0)[None]
    return k


def cloud(planes, poses, min_range=0.0, max_range=np.inf, mask=None):
    """The reference cloud of planes [count, height, width](, k) (t, instance, triangle, location, normal, uv) rendered at `poses`:
    every field of FIELDS [total](, k) in (frame, y, x) order plus offsets int64 [count + 1] and `kept`, the boolean planes."""
    k = keep(planes, min_range, max_range, mask)
    count, h, w = k.shape
    poses = np.asarray(poses, np.float32).reshape(count, 6)
    out = dict(range=planes["t"][k], instance=planes["instance"][k], triangle=planes["triangle"][k], position=planes["location"][k],
               normal=planes["normal"][k], uv=planes["uv"][k])      # (boolean indexing is row-major: frame, then y, then x)
    f, y, x = np.nonzero(k)
    out["pixel"] = (y * w + x).astype(np.int32)
    out["frame"] = f.astype(np.int32)
    per = k.reshape(count, -1).sum(axis=1)
    out["offsets"] = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    local = np.zeros((len(f), 3), np.float32)
    for i in range(count):
        a, b = out["offsets"][i], out["offsets"][i + 1]
        if b > a:
            local[a:b] = apply_lre(poses[i], out["position"][a:b])
    out["local"] = local
    out["kept"] = k
    return out
