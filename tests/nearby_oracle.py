"""ctypes bindings of tests/nearby_oracle.c: brute-force nearby-triangle lists over an oracle scene (the specification of
rt_nearby_offsets / rt_list_nearby).  TEST INFRASTRUCTURE ONLY.  Built like tests/point_oracle.py: compiled with the oracle's flags next
to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "nearby_oracle.c")
DEPS = (SRC, os.path.join(HERE, "point_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libnearby_oracle.so")
FIELDS = dict(distance=((), np.float32), instance=((), np.int32), triangle=((), np.int32), point=((3,), np.float32),
              normal=((3,), np.float32), barycentric=((2,), np.float32), uv=((2,), np.float32))
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
            L.orcn_count_nearby.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            L.orcn_count_nearby.restype = None
            L.orcn_list_nearby.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 8
            L.orcn_list_nearby.restype = None
            _lib = L
    return _lib


def _in(points, max_distance):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    md = None if max_distance is None else np.ascontiguousarray(max_distance, np.float32).reshape(len(p))
    return p, md


def count_nearby(scene, points, max_distance=None, threads=8):
    """The number of pairs of every point (int32, flat)"""
    L = lib()
    p, md = _in(points, max_distance)
    cnt = np.zeros(len(p), np.int32)

    def run(a, b):
        L.orcn_count_nearby(scene.h, b - a, p[a:].ctypes.data, None if md is None else md[a:].ctypes.data, cnt[a:].ctypes.data)
    _parallel(len(p), 16, run, threads)
    return cnt


def rooms(scene, points, max_distance=None, offsets=None, max_hits=None, slots=None, fill=None, threads=8):
    """The rule on every point, written into rooms (offsets int64 [n + 1], or max_hits K: point i at [i*K, i*K + K)) of flat per-slot
    arrays of `slots` entries (default offsets[n] or n*K), each first set to `fill` (dict field -> value; default 0) -> dict of the
    FIELDS, flat, plus count [n]."""
    L = lib()
    p, md = _in(points, max_distance)
    n = len(p)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64).reshape(n + 1)
    if slots is None:
        slots = int(off[n]) if off is not None else n * int(max_hits)
    fill = fill or {}
    out = {k: np.full((slots,) + tr, fill.get(k, 0), dt) for k, (tr, dt) in FIELDS.items()}
    cnt = np.zeros(n, np.int32)

    def run(a, b):
        L.orcn_list_nearby(scene.h, b - a, p[a:].ctypes.data, None if md is None else md[a:].ctypes.data,
                           None if off is None else off[a:].ctypes.data, 0 if max_hits is None else int(max_hits),
                           *[out[k].ctypes.data if off is not None else out[k][a * int(max_hits):].ctypes.data for k in FIELDS],
                           cnt[a:].ctypes.data)
    _parallel(n, 16, run, threads)
    out["count"] = cnt
    return out


def list_nearby(scene, points, max_distance=None, max_hits=None, threads=8):
    """Shaped like the product's Scene.list_nearby: CSR (max_hits None: offsets, flat fields, point_index, count) or fixed rooms of
    max_hits (fields [..., K(, 2|3)], count [...])."""
    p = np.ascontiguousarray(points, np.float32)
    lead = p.shape[:-1]
    if max_hits is None:
        c = count_nearby(scene, p, max_distance, threads=threads)
        off = np.concatenate([[0], np.cumsum(c, dtype=np.int64)]).astype(np.int64)
        r = rooms(scene, p, max_distance, offsets=off, threads=threads)
        assert np.array_equal(r["count"], c)
        r["offsets"] = off
        r["point_index"] = np.repeat(np.arange(len(c), dtype=np.int32), c)
        r["count"] = r["count"].reshape(lead)
        return r
    r = rooms(scene, p, max_distance, max_hits=max_hits, threads=threads)
    res = {k: r[k].reshape(lead + (max_hits,) + FIELDS[k][0]) for k in FIELDS}
    res["count"] = r["count"].reshape(lead)
    return res
