"""ctypes bindings of tests/point_oracle.c: the brute-force closest point of an oracle scene to arbitrary points (the specification of
rt_closest_points / Scene.closest_points).  TEST INFRASTRUCTURE ONLY.  Built like tests/ray_oracle.py: compiled with the oracle's flags
next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "point_oracle.c")
DEPS = (SRC, os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libpoint_oracle.so")
OUTPUTS = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")
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
            L.orcx_closest_points.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7
            L.orcx_closest_points.restype = None
            L.orcx_closest_on_triangle.argtypes = [C.c_void_p] * 5
            L.orcx_closest_on_triangle.restype = None
            _lib = L
    return _lib


def closest_points(scene, points, max_distance=None, only_instance=-1, threads=8):
    """The rule of rt_closest_points on every point of points [..., 3] (scene: an orc.OracleScene), by brute force -> dict of
    OUTPUTS shaped like the product's Scene.closest_points.  only_instance >= 0: that instance alone."""
    L = lib()
    p = np.ascontiguousarray(points, np.float32)
    lead = p.shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    p = p.reshape(n, 3)
    md = None if max_distance is None else np.ascontiguousarray(max_distance, np.float32).reshape(n)
    out = dict(distance=np.zeros(n, np.float32), instance=np.zeros(n, np.int32), triangle=np.zeros(n, np.int32),
               point=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), barycentric=np.zeros((n, 2), np.float32),
               uv=np.zeros((n, 2), np.float32))

    def run(a, b):
        L.orcx_closest_points(scene.h, b - a, p[a:].ctypes.data, None if md is None else md[a:].ctypes.data, only_instance,
                              *[out[k][a:].ctypes.data for k in OUTPUTS])
    _parallel(n, 256, run, threads)
    return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}


def on_triangle(q, a, ab, ac):
    """The rule on one triangle given in scaled mesh space -> (b1, b2, d2) as float32."""
    L = lib()
    arrs = [np.ascontiguousarray(v, np.float32).reshape(3) for v in (q, a, ab, ac)]
    out = np.zeros(3, np.float32)
    L.orcx_closest_on_triangle(*[v.ctypes.data for v in arrs], out.ctypes.data)
    return out[0], out[1], out[2]
