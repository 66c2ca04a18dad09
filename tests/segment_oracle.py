"""ctypes bindings of tests/segment_oracle.c: the brute-force nearest point of an oracle scene to arbitrary segments, with the capsule
test (the specification of rt_closest_to_segments / Scene.closest_to_segments).  TEST INFRASTRUCTURE ONLY.  Built like
tests/point_oracle.py: compiled with the oracle's flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "segment_oracle.c")
DEPS = (SRC, os.path.join(HERE, "crossing_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libsegment_oracle.so")
# the product's fields in RtSegmentHits' order (pops is no part of the rule), then `which`: the winning candidate 0..4 = (a)..(e)
OUTPUTS = ("distance", "instance", "triangle", "parameter", "segment_point", "point", "normal", "barycentric", "uv", "crossings",
           "clearance", "within")
_SHAPES = dict(distance=((), np.float32), instance=((), np.int32), triangle=((), np.int32), parameter=((), np.float32),
               segment_point=((3,), np.float32), point=((3,), np.float32), normal=((3,), np.float32), barycentric=((2,), np.float32),
               uv=((2,), np.float32), crossings=((), np.int32), clearance=((), np.float32), within=((), np.int32), which=((), np.int32))
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
            L.orcx_closest_to_segments.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 13
            L.orcx_closest_to_segments.restype = None
            L.orcx_segment_on_triangle.argtypes = [C.c_void_p] * 6
            L.orcx_segment_on_triangle.restype = None
            L.orcx_segment_segment.argtypes = [C.c_void_p] * 5
            L.orcx_segment_segment.restype = None
            _lib = L
    return _lib


def closest_to_segments(scene, segments, max_distance=None, only_instance=-1, threads=8):
    """Rule 13 on every segment of segments [..., 2, 3] (scene: an orc.OracleScene), by brute force -> dict of OUTPUTS shaped like the
    product's Scene.closest_to_segments, plus `which`.  only_instance >= 0: that instance alone in the distance half."""
    L = lib()
    s = np.ascontiguousarray(segments, np.float32)
    lead = s.shape[:-2]
    n = int(np.prod(lead, dtype=np.int64))
    s = s.reshape(n, 6)
    md = None if max_distance is None else np.ascontiguousarray(max_distance, np.float32).reshape(n)
    names = OUTPUTS + ("which",)
    out = {k: np.zeros((n,) + _SHAPES[k][0], _SHAPES[k][1]) for k in names}

    def run(a, b):
        L.orcx_closest_to_segments(scene.h, b - a, s[a:].ctypes.data, None if md is None else md[a:].ctypes.data, only_instance,
                                   *[out[k][a:].ctypes.data for k in names])
    _parallel(n, 64, run, threads)
    return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}


def on_triangle(q0, q1, a, ab, ac):
    """Steps 2-3 on one triangle given in scaled mesh space -> (s, b1, b2, d2) as float32 and the winning candidate 0..4"""
    L = lib()
    arrs = [np.ascontiguousarray(v, np.float32).reshape(3) for v in (q0, q1, a, ab, ac)]
    out = np.zeros(5, np.float32)
    L.orcx_segment_on_triangle(*[v.ctypes.data for v in arrs], out.ctypes.data)
    return out[0], out[1], out[2], out[3], int(out[4])


def segment_segment(q0, d, e0, f):
    """Step 4 alone -> (s, u) as float32"""
    L = lib()
    arrs = [np.ascontiguousarray(v, np.float32).reshape(3) for v in (q0, d, e0, f)]
    out = np.zeros(2, np.float32)
    L.orcx_segment_segment(*[v.ctypes.data for v in arrs], out.ctypes.data)
    return out[0], out[1]
