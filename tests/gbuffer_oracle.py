"""The CPU oracle of G-buffer frames (rt_render_gbuffer / Camera.render_gbuffer): ray_oracle's camera_ray and cast_ray_lp for every
pixel, plus the `depth` plane through tests/gbuffer_oracle.c, which applies the oracle's own apply_lre.  TEST INFRASTRUCTURE ONLY.
Built like tests/ray_oracle.py: compiled with the oracle's flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

import ray_oracle
from ray_oracle import FLAGS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "gbuffer_oracle.c")
DEPS = (SRC, os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libgbuffer_oracle.so")
PLANES = ("t", "depth", "instance", "triangle", "location", "normal", "uv")
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
            L.orcx_gbuffer_depth.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            L.orcx_gbuffer_depth.restype = None
            _lib = L
    return _lib


def depth(pose, location, instance):
    """apply_lre(pose, location).z where instance >= 0, FLT_MAX elsewhere: location [..., 3] float32, instance [...] int32"""
    loc = np.ascontiguousarray(location, np.float32)
    inst = np.ascontiguousarray(instance, np.int32)
    assert loc.shape == inst.shape + (3,)
    out = np.zeros(inst.shape, np.float32)
    P = np.ascontiguousarray(pose, np.float32)
    lib().orcx_gbuffer_depth(P.ctypes.data, inst.size, loc.ctypes.data, inst.ctypes.data, out.ctypes.data)
    return out


def frame(scene, width, height, K, D, pose, threads=8):
    """Every plane of one frame [height, width](, k) as the oracle computes it (scene: an orc.OracleScene)"""
    o, d = ray_oracle.camera_rays(width, height, K, D, pose, threads=threads)
    ref = ray_oracle.cast_rays(scene, o, d, threads=threads)
    out = {k: ref[k] for k in PLANES if k != "depth"}
    out["depth"] = depth(pose, ref["location"], ref["instance"])
    return out


def frames(scene, width, height, K, D, poses, threads=8):
    """[count, height, width](, k) planes of the poses"""
    per = [frame(scene, width, height, K, D, p, threads) for p in poses]
    return {k: np.stack([f[k] for f in per]) for k in PLANES}
