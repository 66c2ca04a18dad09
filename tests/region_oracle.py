"""ctypes bindings of tests/region_oracle.c: brute-force region queries over an oracle scene (the specification of
rt_count_in_regions / rt_region_offsets / rt_list_in_regions, include/rt_hip.h rule 15).  TEST INFRASTRUCTURE ONLY.  Built like
tests/section_oracle.py: compiled with the oracle's flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "region_oracle.c")
DEPS = (SRC, os.path.join(HERE, "crossing_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libregion_oracle.so")
FIELDS = dict(instance=((), np.int32), triangle=((), np.int32), inside=((), np.uint8), normal=((3,), np.float32))
MAX_PLANES, MAX_VERTS = 8, 11
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
            L.orcr_pair.argtypes = [C.c_int] + [C.c_void_p] * 7
            L.orcr_pair.restype = C.c_int
            L.orcr_count_in_regions.argtypes = [C.c_void_p, C.c_int64, C.c_int] + [C.c_void_p] * 3
            L.orcr_count_in_regions.restype = None
            L.orcr_list_in_regions.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 5
            L.orcr_list_in_regions.restype = None
            _lib = L
    return _lib


def pair(region, tri, pose=(0.0,) * 6):
    """rule 15 on one pair: region [K, 2, 3] world (point, inward normal per plane), pose [6] the instance's world -> mesh map, tri
    [3, 3] in scaled mesh space -> (pair, inside, heights [K, 3], polygon [m, 3] in MESH space (the triangle when inside, empty when
    no pair), mapped [K, 2, 3] = p' and n')"""
    r = np.ascontiguousarray(region, np.float32)
    K = r.shape[0]
    assert r.shape == (K, 2, 3)
    p, t = (np.ascontiguousarray(a, np.float32).reshape(k) for a, k in ((pose, 6), (tri, 9)))
    h, poly, mapped = np.zeros((max(K, 1), 3), np.float32), np.zeros((MAX_VERTS, 3), np.float32), np.zeros((max(K, 1), 2, 3), np.float32)
    m = C.c_int32(0)
    res = lib().orcr_pair(K, r.ctypes.data, p.ctypes.data, t.ctypes.data, h.ctypes.data, poly.ctypes.data, C.addressof(m), mapped.ctypes.data)
    return res > 0, res == 2, h[:K], poly[:m.value].copy(), mapped[:K]


def _in(regions):
    b = np.ascontiguousarray(regions, np.float32)
    K = b.shape[-3]
    assert b.shape[-2:] == (2, 3) and 1 <= K <= MAX_PLANES, b.shape
    return b.reshape(-1, K, 2, 3), K


def count_in_regions(scene, regions, threads=8):
    """dict of count and inside (the number of wholly-inside pairs) of every region (int32, flat)"""
    L = lib()
    b, K = _in(regions)
    cnt, ins = np.zeros(len(b), np.int32), np.zeros(len(b), np.int32)

    def run(a, e):
        L.orcr_count_in_regions(scene.h, e - a, K, b[a:].ctypes.data, cnt[a:].ctypes.data, ins[a:].ctypes.data)
    _parallel(len(b), 16, run, threads)
    return dict(count=cnt, inside=ins)


def rooms(scene, regions, offsets=None, max_hits=None, slots=None, fill=None, threads=8):
    """The rule on every region, written into rooms (offsets int64 [n + 1], or max_hits: region i at [i*M, i*M + M)) of flat per-slot
    arrays of `slots` entries (default offsets[n] or n*M), each first set to `fill` (dict field -> value; default 0) -> dict of the
    FIELDS, flat, plus count [n]."""
    L = lib()
    b, K = _in(regions)
    n = len(b)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64).reshape(n + 1)
    if slots is None:
        slots = int(off[n]) if off is not None else n * int(max_hits)
    fill = fill or {}
    out = {k: np.full((slots,) + tr, fill.get(k, 0), dt) for k, (tr, dt) in FIELDS.items()}
    cnt = np.zeros(n, np.int32)

    def run(a, e):
        L.orcr_list_in_regions(scene.h, e - a, K, b[a:].ctypes.data, None if off is None else off[a:].ctypes.data,
                               0 if max_hits is None else int(max_hits),
                               *[out[k].ctypes.data if off is not None else out[k][a * int(max_hits):].ctypes.data for k in FIELDS],
                               cnt[a:].ctypes.data)
    _parallel(n, 16, run, threads)
    out["count"] = cnt
    return out


def list_in_regions(scene, regions, max_hits=None, threads=8):
    """Shaped like the product's Scene.list_in_regions: CSR (max_hits None: offsets, flat fields, query_index, count) or fixed rooms
    of max_hits (fields [..., M(, 3)], count [...])."""
    b = np.ascontiguousarray(regions, np.float32)
    lead = b.shape[:-3]
    if max_hits is None:
        c = count_in_regions(scene, b, threads=threads)["count"]
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
