"""ctypes bindings of tests/crossing_oracle.c: brute-force crossing counts, winding numbers and signed distance over an oracle scene
(the specification of rt_count_crossings / rt_winding_numbers / rt_signed_distance).  TEST INFRASTRUCTURE ONLY.  Built like
tests/point_oracle.py: compiled with the oracle's flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

import point_oracle
from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "crossing_oracle.c")
DEPS = (SRC, os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libcrossing_oracle.so")
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
            L.orcx_count_crossings.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 5
            L.orcx_count_crossings.restype = None
            L.orcx_crossing_ts.argtypes = [C.c_void_p] * 3 + [C.c_float, C.c_void_p, C.c_int]
            L.orcx_crossing_ts.restype = C.c_int
            L.orcx_winding_numbers.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            L.orcx_winding_numbers.restype = None
            L.orcx_crossing_on_triangle.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_void_p]
            L.orcx_crossing_on_triangle.restype = C.c_int
            _lib = L
    return _lib


def count_crossings(scene, origins, directions, tmax=None, threads=8):
    """The rule of rt_count_crossings on every ray (scene: an orc.OracleScene) -> dict(count, winding), int32 of the rays' leading
    shape."""
    L = lib()
    o = np.ascontiguousarray(origins, np.float32)
    lead = o.shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    o = o.reshape(n, 3)
    d = np.ascontiguousarray(directions, np.float32).reshape(n, 3)
    tm = None if tmax is None else np.ascontiguousarray(tmax, np.float32).reshape(n)
    cnt, wn = np.zeros(n, np.int32), np.zeros(n, np.int32)

    def run(a, b):
        L.orcx_count_crossings(scene.h, b - a, o[a:].ctypes.data, d[a:].ctypes.data, None if tm is None else tm[a:].ctypes.data,
                               cnt[a:].ctypes.data, wn[a:].ctypes.data)
    _parallel(n, 256, run, threads)
    return dict(count=cnt.reshape(lead), winding=wn.reshape(lead))


def crossing_ts(scene, origin, direction, tmax=np.inf):
    """The sorted counted t of one ray (float32)"""
    L = lib()
    o = np.ascontiguousarray(origin, np.float32).reshape(3)
    d = np.ascontiguousarray(direction, np.float32).reshape(3)
    cap = 4096
    ts = np.zeros(cap, np.float32)
    c = L.orcx_crossing_ts(scene.h, o.ctypes.data, d.ctypes.data, float(tmax), ts.ctypes.data, cap)
    assert c <= cap
    return np.sort(ts[:c])


def winding_numbers(scene, points, per_direction=False, threads=8):
    """The median winding of every point (rule 6) -> int32 of the points' leading shape; per_direction: also the three windings
    [..., 3]."""
    L = lib()
    p = np.ascontiguousarray(points, np.float32)
    lead = p.shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    p = p.reshape(n, 3)
    wn, per = np.zeros(n, np.int32), np.zeros((n, 3), np.int32)

    def run(a, b):
        L.orcx_winding_numbers(scene.h, b - a, p[a:].ctypes.data, wn[a:].ctypes.data, per[a:].ctypes.data)
    _parallel(n, 64, run, threads)
    if per_direction:
        return wn.reshape(lead), per.reshape(lead + (3,))
    return wn.reshape(lead)


def signed_distance(scene, points, max_distance=None, threads=8):
    """rule 7: point_oracle's distance, negated where the median winding is not 0 -> float32 of the points' leading shape"""
    d = point_oracle.closest_points(scene, points, max_distance, threads=threads)["distance"]
    w = winding_numbers(scene, points, threads=threads)
    return np.where(w != 0, -d, d).astype(np.float32)


def on_triangle(o, d, a, ab, ac, tmax=np.inf):
    """The rule on one triangle given in scaled mesh space -> (sign, t); sign 0 = not counted"""
    L = lib()
    arrs = [np.ascontiguousarray(v, np.float32).reshape(3) for v in (o, d, a, ab, ac)]
    t = np.zeros(1, np.float32)
    s = L.orcx_crossing_on_triangle(*[v.ctypes.data for v in arrs], float(tmax), t.ctypes.data)
    return s, t[0]
