"""The CPU oracle of sensor frames (rt_render_gbuffer_table / Sensor.render_gbuffer): the rays of a direction table through
tests/sensor_oracle.c -- the oracle's own invert_lre, apply_euler and normalize3 -- then ray_oracle's cast_ray_lp on them and
gbuffer_oracle's depth.  TEST INFRASTRUCTURE ONLY.  Built like tests/gbuffer_oracle.py."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

import gbuffer_oracle
import ray_oracle
from ray_oracle import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "sensor_oracle.c")
DEPS = (SRC, os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libsensor_oracle.so")
PLANES = gbuffer_oracle.PLANES
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
            L.orcx_sensor_rays.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            L.orcx_sensor_rays.restype = None
            L.orcx_sensor_normalize.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
            L.orcx_sensor_normalize.restype = None
            _lib = L
    return _lib


def rays(dirs, pose):
    """(origins, directions) float32 shaped like dirs [..., 3]: normalize3(apply_euler(invert_lre(pose).ypr, c)) of every entry"""
    c = np.ascontiguousarray(dirs, np.float32)
    assert c.shape[-1] == 3
    P = np.ascontiguousarray(pose, np.float32)
    assert P.shape == (6,)
    o, d = np.zeros_like(c), np.zeros_like(c)
    lib().orcx_sensor_rays(P.ctypes.data, c.size // 3, c.ctypes.data, o.ctypes.data, d.ctypes.data)
    return o, d


def normalize(dirs):
    c = np.ascontiguousarray(dirs, np.float32)
    out = np.zeros_like(c)
    lib().orcx_sensor_normalize(c.size // 3, c.ctypes.data, out.ctypes.data)
    return out


def frame(scene, dirs, pose, threads=8):
    """Every plane of one frame [height, width](, k) of the table dirs [height, width, 3] (scene: an orc.OracleScene)"""
    o, d = rays(dirs, pose)
    ref = ray_oracle.cast_rays(scene, o, d, threads=threads)
    out = {k: ref[k] for k in PLANES if k != "depth"}
    out["depth"] = gbuffer_oracle.depth(pose, ref["location"], ref["instance"])
    return out


def frames(scene, dirs, poses, threads=8):
    """[count, height, width](, k) planes of the poses"""
    per = [frame(scene, dirs, p, threads) for p in poses]
    return {k: np.stack([f[k] for f in per]) for k in PLANES}
