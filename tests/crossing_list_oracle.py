"""ctypes bindings of tests/crossing_list_oracle.c: brute-force crossing lists over an oracle scene (the specification of
rt_crossing_offsets / rt_list_crossings).  TEST INFRASTRUCTURE ONLY.  Built like tests/crossing_oracle.py: compiled with the oracle's
flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "crossing_list_oracle.c")
DEPS = (SRC, os.path.join(HERE, "crossing_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libcrossing_list_oracle.so")
FIELDS = dict(t=((), np.float32), instance=((), np.int32), triangle=((), np.int32), sign=((), np.int8), barycentric=((2,), np.float32),
              uv=((2,), np.float32), point=((3,), np.float32))
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
            L.orcl_list_crossings.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 8
            L.orcl_list_crossings.restype = None
            L.orcl_on_triangle.argtypes = [C.c_void_p] * 5 + [C.c_float, C.c_void_p]
            L.orcl_on_triangle.restype = C.c_int
            _lib = L
    return _lib


def rooms(scene, origins, directions, tmax=None, offsets=None, max_hits=None, slots=None, fill=None, threads=8):
    """The rule on every ray, written into rooms (offsets int64 [n + 1], or max_hits K: ray i at [i*K, i*K + K)) of flat per-slot
    arrays of `slots` entries (default offsets[n] or n*K), each first set to `fill` (dict field -> value; default 0) -> dict of the
    FIELDS, flat, plus count [n]."""
    L = lib()
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    n = len(o)
    d = np.ascontiguousarray(directions, np.float32).reshape(n, 3)
    tm = None if tmax is None else np.ascontiguousarray(tmax, np.float32).reshape(n)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64).reshape(n + 1)
    if slots is None:
        slots = int(off[n]) if off is not None else n * int(max_hits)
    fill = fill or {}
    out = {k: np.full((slots,) + tr, fill.get(k, 0), dt) for k, (tr, dt) in FIELDS.items()}
    cnt = np.zeros(n, np.int32)

    def run(a, b):
        L.orcl_list_crossings(scene.h, b - a, o[a:].ctypes.data, d[a:].ctypes.data, None if tm is None else tm[a:].ctypes.data,
                              None if off is None else off[a:].ctypes.data,
                              0 if max_hits is None else int(max_hits), *[out[k].ctypes.data if off is not None
                                                                         else out[k][a * int(max_hits):].ctypes.data for k in FIELDS],
                              cnt[a:].ctypes.data)
    _parallel(n, 64, run, threads)
    out["count"] = cnt
    return out


def list_crossings(scene, origins, directions, tmax=None, max_hits=None, threads=8):
    """Shaped like the product's Scene.list_crossings: CSR (max_hits None: offsets, flat fields, ray, count) or fixed rooms of
    max_hits (fields [..., K(, 2|3)], count [...])."""
    o = np.ascontiguousarray(origins, np.float32)
    lead = o.shape[:-1]
    if max_hits is None:
        import crossing_oracle as xo
        c = xo.count_crossings(scene, o, directions, tmax, threads=threads)["count"].reshape(-1)
        off = np.concatenate([[0], np.cumsum(c, dtype=np.int64)]).astype(np.int64)
        r = rooms(scene, o, directions, tmax, offsets=off, threads=threads)
        r["offsets"] = off
        r["ray"] = np.repeat(np.arange(len(c), dtype=np.int32), c)
        r["count"] = r["count"].reshape(lead)
        return r
    r = rooms(scene, o, directions, tmax, max_hits=max_hits, threads=threads)
    res = {k: r[k].reshape(lead + (max_hits,) + FIELDS[k][0]) for k in FIELDS}
    res["count"] = r["count"].reshape(lead)
    return res


def on_triangle(o, d, a, ab, ac, tmax=np.inf):
    """Rule 3 on one triangle in scaled mesh space -> (sign, t, V, W, det); sign 0 = not counted"""
    L = lib()
    arrs = [np.ascontiguousarray(v, np.float32).reshape(3) for v in (o, d, a, ab, ac)]
    out = np.zeros(4, np.float32)
    s = L.orcl_on_triangle(*[v.ctypes.data for v in arrs], float(tmax), out.ctypes.data)
    return s, out[0], out[1], out[2], out[3]
