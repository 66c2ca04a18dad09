"""ctypes bindings of tests/tri_intersect_oracle.c: brute-force triangle intersection queries over an oracle scene (the specification of
rt_count_intersecting / rt_intersecting_offsets / rt_list_intersecting).  TEST INFRASTRUCTURE ONLY.  Built like tests/nearby_oracle.py:
compiled with the oracle's flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "tri_intersect_oracle.c")
DEPS = (SRC, os.path.join(HERE, "crossing_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libtri_intersect_oracle.so")
FIELDS = dict(instance=((), np.int32), triangle=((), np.int32), normal=((3,), np.float32), segment=((2, 3), np.float32))
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
            L.orct_pair.argtypes = [C.c_void_p] * 3
            L.orct_pair.restype = C.c_int
            L.orct_segment.argtypes = [C.c_void_p] * 6
            L.orct_segment.restype = C.c_int
            L.orct_count_intersecting.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
            L.orct_count_intersecting.restype = None
            L.orct_list_intersecting.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 5
            L.orct_list_intersecting.restype = None
            _lib = L
    return _lib


def pair(q, t):
    """rule 10 on one pair given in scaled mesh space: q, t [3, 3] -> (hit, segment [2, 3])"""
    qa, ta = (np.ascontiguousarray(a, np.float32).reshape(9) for a in (q, t))
    seg = np.zeros((2, 3), np.float32)
    hit = lib().orct_pair(qa.ctypes.data, ta.ctypes.data, seg.ctypes.data)
    return bool(hit), seg


def segment(x, y, tri):
    """one segment test of rule 10 step 4: x -> y against tri [3, 3] -> (counted, t)"""
    v = [np.ascontiguousarray(a, np.float32).reshape(3) for a in (x, y, *np.asarray(tri, np.float32))]
    t = np.zeros(1, np.float32)
    hit = lib().orct_segment(*[a.ctypes.data for a in v], t.ctypes.data)
    return bool(hit), float(t[0])


def _in(tris, skip):
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    s = None if skip is None else np.ascontiguousarray(skip, np.int32).reshape(len(t))
    return t, s


def count_intersecting(scene, tris, skip=None, threads=8):
    """The number of pairs of every query triangle (int32, flat)"""
    L = lib()
    t, s = _in(tris, skip)
    cnt = np.zeros(len(t), np.int32)

    def run(a, b):
        L.orct_count_intersecting(scene.h, b - a, t[a:].ctypes.data, None if s is None else s[a:].ctypes.data, cnt[a:].ctypes.data)
    _parallel(len(t), 16, run, threads)
    return cnt


def rooms(scene, tris, skip=None, offsets=None, max_hits=None, slots=None, fill=None, threads=8):
    """The rule on every query, written into rooms (offsets int64 [n + 1], or max_hits K: query i at [i*K, i*K + K)) of flat per-slot
    arrays of `slots` entries (default offsets[n] or n*K), each first set to `fill` (dict field -> value; default 0) -> dict of the
    FIELDS, flat, plus count [n]."""
    L = lib()
    t, s = _in(tris, skip)
    n = len(t)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64).reshape(n + 1)
    if slots is None:
        slots = int(off[n]) if off is not None else n * int(max_hits)
    fill = fill or {}
    out = {k: np.full((slots,) + tr, fill.get(k, 0), dt) for k, (tr, dt) in FIELDS.items()}
    cnt = np.zeros(n, np.int32)

    def run(a, b):
        L.orct_list_intersecting(scene.h, b - a, t[a:].ctypes.data, None if s is None else s[a:].ctypes.data,
                                 None if off is None else off[a:].ctypes.data, 0 if max_hits is None else int(max_hits),
                                 *[out[k].ctypes.data if off is not None else out[k][a * int(max_hits):].ctypes.data for k in FIELDS],
                                 cnt[a:].ctypes.data)
    _parallel(n, 16, run, threads)
    out["count"] = cnt
    return out


def list_intersecting(scene, tris, skip=None, max_hits=None, threads=8):
    """Shaped like the product's Scene.list_intersecting: CSR (max_hits None: offsets, flat fields, query_index, count) or fixed rooms
    of max_hits (fields [..., K(, 3 | 2, 3)], count [...])."""
    t = np.ascontiguousarray(tris, np.float32)
    lead = t.shape[:-2]
    if max_hits is None:
        c = count_intersecting(scene, t, skip, threads=threads)
        off = np.concatenate([[0], np.cumsum(c, dtype=np.int64)]).astype(np.int64)
        r = rooms(scene, t, skip, offsets=off, threads=threads)
        assert np.array_equal(r["count"], c)
        r["offsets"] = off
        r["query_index"] = np.repeat(np.arange(len(c), dtype=np.int32), c)
        r["count"] = r["count"].reshape(lead)
        return r
    r = rooms(scene, t, skip, max_hits=max_hits, threads=threads)
    res = {k: r[k].reshape(lead + (max_hits,) + FIELDS[k][0]) for k in FIELDS}
    res["count"] = r["count"].reshape(lead)
    return res
