"""ctypes bindings of tests/triangle_distance_oracle.c: the brute-force nearest point of an oracle scene to arbitrary triangles, with the
intersection count (the specification of rt_closest_to_triangles / Scene.closest_to_triangles).  TEST INFRASTRUCTURE ONLY.  Built like
tests/segment_oracle.py: compiled with the oracle's flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "triangle_distance_oracle.c")
DEPS = (SRC, os.path.join(HERE, "tri_intersect_oracle.c"), os.path.join(HERE, "crossing_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libtriangle_distance_oracle.so")
# the product's fields in RtTriangleHits' order (pops is no part of the rule), then `which`: the winning candidate 0..14
OUTPUTS = ("distance", "instance", "triangle", "query_barycentric", "query_point", "point", "normal", "barycentric", "uv", "intersections",
           "clearance", "within")
_SHAPES = dict(distance=((), np.float32), instance=((), np.int32), triangle=((), np.int32), query_barycentric=((2,), np.float32),
               query_point=((3,), np.float32), point=((3,), np.float32), normal=((3,), np.float32), barycentric=((2,), np.float32),
               uv=((2,), np.float32), intersections=((), np.int32), clearance=((), np.float32), within=((), np.int32),
               which=((), np.int32))
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
            L.orcd_closest_to_triangles.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_void_p] * 13
            L.orcd_closest_to_triangles.restype = None
            L.orcd_on_triangle.argtypes = [C.c_void_p] * 5
            L.orcd_on_triangle.restype = None
            _lib = L
    return _lib


def closest_to_triangles(scene, triangles, max_distance=None, skip_instance=None, threads=8):
    """Rule 14 on every triangle of triangles [..., 3, 3] (scene: an orc.OracleScene), by brute force -> dict of OUTPUTS shaped like the
    product's Scene.closest_to_triangles, plus `which`."""
    L = lib()
    t = np.ascontiguousarray(triangles, np.float32)
    lead = t.shape[:-2]
    n = int(np.prod(lead, dtype=np.int64))
    t = t.reshape(n, 9)
    md = None if max_distance is None else np.ascontiguousarray(max_distance, np.float32).reshape(n)
    sk = None if skip_instance is None else np.ascontiguousarray(skip_instance, np.int32).reshape(n)
    names = OUTPUTS + ("which",)
    out = {k: np.zeros((n,) + _SHAPES[k][0], _SHAPES[k][1]) for k in names}

    def run(a, b):
        L.orcd_closest_to_triangles(scene.h, b - a, t[a:].ctypes.data, None if md is None else md[a:].ctypes.data,
                                    None if sk is None else sk[a:].ctypes.data, *[out[k][a:].ctypes.data for k in names])
    _parallel(n, 64, run, threads)
    return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}


def on_triangle(q9, a, ab, ac):
    """Steps 1-3 on one pair given in scaled mesh space (q9: the query's three mapped vertices) -> (q1, q2, b1, b2, d2) as float32 and
    the winning candidate 0..14"""
    L = lib()
    arrs = [np.ascontiguousarray(q9, np.float32).reshape(9)] + [np.ascontiguousarray(v, np.float32).reshape(3) for v in (a, ab, ac)]
    out = np.zeros(6, np.float32)
    L.orcd_on_triangle(*[v.ctypes.data for v in arrs], out.ctypes.data)
    return out[0], out[1], out[2], out[3], out[4], int(out[5])
