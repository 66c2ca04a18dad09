"""ctypes bindings of tests/section_oracle.c: brute-force plane sections over an oracle scene (the specification of rt_count_sections /
rt_section_offsets / rt_list_sections).  TEST INFRASTRUCTURE ONLY.  Built like tests/box_oracle.py: compiled with the oracle's flags
next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "section_oracle.c")
DEPS = (SRC, os.path.join(HERE, "crossing_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libsection_oracle.so")
FIELDS = dict(instance=((), np.int32), triangle=((), np.int32), segment=((2, 3), np.float32), normal=((3,), np.float32))
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
            L.orcs_pair.argtypes = [C.c_void_p] * 6
            L.orcs_pair.restype = C.c_int
            L.orcs_count_sections.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            L.orcs_count_sections.restype = None
            L.orcs_list_sections.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
            L.orcs_list_sections.restype = None
            _lib = L
    return _lib


def pair(plane, tri, pose=(0.0,) * 6):
    """rule 12 on one pair: plane [2, 3] world (point, normal), pose [6] the instance's world -> mesh map, tri [3, 3] in scaled mesh
    space -> (pair, segment [2, 3] in MESH space (0 when no pair), heights [3], mapped [2, 3] = p' and n')"""
    b, p, t = (np.ascontiguousarray(a, np.float32).reshape(k) for a, k in ((plane, 6), (pose, 6), (tri, 9)))
    seg, h, mapped = np.zeros((2, 3), np.float32), np.zeros(3, np.float32), np.zeros((2, 3), np.float32)
    hit = lib().orcs_pair(b.ctypes.data, p.ctypes.data, t.ctypes.data, seg.ctypes.data, h.ctypes.data, mapped.ctypes.data)
    return bool(hit), seg, h, mapped


def _in(planes):
    return np.ascontiguousarray(planes, np.float32).reshape(-1, 2, 3)


def count_sections(scene, planes, threads=8):
    """The number of pairs of every plane (int32, flat)"""
    L = lib()
    b = _in(planes)
    cnt = np.zeros(len(b), np.int32)

    def run(a, e):
        L.orcs_count_sections(scene.h, e - a, b[a:].ctypes.data, cnt[a:].ctypes.data)
    _parallel(len(b), 16, run, threads)
    return cnt


def rooms(scene, planes, offsets=None, max_hits=None, slots=None, fill=None, threads=8):
    """The rule on every plane, written into rooms (offsets int64 [n + 1], or max_hits K: plane i at [i*K, i*K + K)) of flat per-slot
    arrays of `slots` entries (default offsets[n] or n*K), each first set to `fill` (dict field -> value; default 0) -> dict of the
    FIELDS, flat, plus count [n]."""
    L = lib()
    b = _in(planes)
    n = len(b)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64).reshape(n + 1)
    if slots is None:
        slots = int(off[n]) if off is not None else n * int(max_hits)
    fill = fill or {}
    out = {k: np.full((slots,) + tr, fill.get(k, 0), dt) for k, (tr, dt) in FIELDS.items()}
    cnt = np.zeros(n, np.int32)

    def run(a, e):
        L.orcs_list_sections(scene.h, e - a, b[a:].ctypes.data, None if off is None else off[a:].ctypes.data,
                             0 if max_hits is None else int(max_hits),
                             *[out[k].ctypes.data if off is not None else out[k][a * int(max_hits):].ctypes.data for k in FIELDS],
                             cnt[a:].ctypes.data)
    _parallel(n, 16, run, threads)
    out["count"] = cnt
    return out


def list_sections(scene, planes, max_hits=None, threads=8):
    """Shaped like the product's Scene.list_sections: CSR (max_hits None: offsets, flat fields, query_index, count) or fixed rooms of
    max_hits (fields [..., K(, 2, 3 | 3)], count [...])."""
    b = np.ascontiguousarray(planes, np.float32)
    lead = b.shape[:-2]
    if max_hits is None:
        c = count_sections(scene, b, threads=threads)
        off = np.concatenate([[0], np.cumsum(c, dtype=np.int64)]).astype(np.int64)
        r = rooms(scene, b, offsets=off, threads=threads)
        assert np.array_equal(r["count"], c)
        r["offsets"] = off
        r["query_index"] = np.repeat(np.arange(len(c), dtype=np.int32), c)
        r["count"] = r["count"].reshape(lead)
        return r
    r = rooms(scene, b, max_hits=max_hits, threads=threads)
    res = {k: r[k].reshape(lead + (max_hits,) + FIELDS[k][0]) for k in FIELDS}
    res["count"] = r["count"].reshape(lead)
    return res
