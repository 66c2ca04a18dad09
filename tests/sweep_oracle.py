"""ctypes bindings of tests/sweep_oracle.c: the brute-force first contact of a sphere moving along a segment with an oracle scene (the
specification of rt_sweep_spheres / Scene.sweep_spheres).  TEST INFRASTRUCTURE ONLY.  Built like tests/segment_oracle.py: compiled
with the oracle's flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "sweep_oracle.c")
DEPS = (SRC, os.path.join(HERE, "point_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libsweep_oracle.so")
# the product's fields in RtSweepHits' order (pops is no part of the rule), then `which`: the winning candidate 0..7 = start, face,
# edges AB / AC / BC, vertices A / B / C
OUTPUTS = ("time", "distance", "instance", "triangle", "centre", "point", "normal", "contact_normal", "barycentric", "uv", "hit")
_SHAPES = dict(time=((), np.float32), distance=((), np.float32), instance=((), np.int32), triangle=((), np.int32),
               centre=((3,), np.float32), point=((3,), np.float32), normal=((3,), np.float32), contact_normal=((3,), np.float32),
               barycentric=((2,), np.float32), uv=((2,), np.float32), hit=((), np.int32), which=((), np.int32))
# rule 16 step 3's constants, as the shim was compiled: reach = (r + r * KR) + M * KM
KR = 2.0 ** -20
KM = 2.0 ** -20
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
            L.orcx_sweep_spheres.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 12
            L.orcx_sweep_spheres.restype = None
            L.orcx_sweep_on_triangle.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.orcx_sweep_on_triangle.restype = None
            L.orcx_sweep_reach2.argtypes = [C.c_void_p, C.c_void_p, C.c_float]
            L.orcx_sweep_reach2.restype = C.c_float
            _lib = L
    return _lib


def sweep_spheres(scene, segments, radius, only_instance=-1, threads=8):
    """Rule 16 on every sweep of segments [..., 2, 3] with radius [...] (scene: an orc.OracleScene), by brute force -> dict of OUTPUTS
    shaped like the product's Scene.sweep_spheres, plus `which`.  only_instance >= 0: that instance alone."""
    L = lib()
    s = np.ascontiguousarray(segments, np.float32)
    lead = s.shape[:-2]
    n = int(np.prod(lead, dtype=np.int64))
    s = s.reshape(n, 6)
    rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32), lead)).reshape(n)
    names = OUTPUTS + ("which",)
    out = {k: np.zeros((n,) + _SHAPES[k][0], _SHAPES[k][1]) for k in names}

    def run(a, b):
        L.orcx_sweep_spheres(scene.h, b - a, s[a:].ctypes.data, rad[a:].ctypes.data, only_instance, *[out[k][a:].ctypes.data for k in names])
    _parallel(n, 64, run, threads)
    return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}


def on_triangle(q0, q1, r, a, ab, ac):
    """Steps 2-3 on one triangle given in scaled mesh space -> (s, b1, b2, d2) as float32 and the winning candidate 0..7 (-1: none)"""
    L = lib()
    arrs = [np.ascontiguousarray(v, np.float32).reshape(3) for v in (q0, q1, a, ab, ac)]
    out = np.zeros(5, np.float32)
    L.orcx_sweep_on_triangle(arrs[0].ctypes.data, arrs[1].ctypes.data, np.float32(r), arrs[2].ctypes.data, arrs[3].ctypes.data,
                             arrs[4].ctypes.data, out.ctypes.data)
    return out[0], out[1], out[2], out[3], int(out[4])


def reach2(q0, q1, r):
    """Step 3's bound in d2 for the mapped ends q0, q1 and the radius r, as float32"""
    L = lib()
    a, b = (np.ascontiguousarray(v, np.float32).reshape(3) for v in (q0, q1))
    return np.float32(L.orcx_sweep_reach2(a.ctypes.data, b.ctypes.data, np.float32(r)))
