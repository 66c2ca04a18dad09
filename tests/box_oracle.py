"""ctypes bindings of tests/box_oracle.c: brute-force box queries over an oracle scene (the specification of rt_count_in_boxes /
rt_box_offsets / rt_list_in_boxes / rt_occupancy_grid).  TEST INFRASTRUCTURE ONLY.  Built like tests/tri_intersect_oracle.py: compiled
with the oracle's flags next to this file when it is missing or older than its sources."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

from ray_oracle import FLAGS, _parallel

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "box_oracle.c")
DEPS = (SRC, os.path.join(HERE, "crossing_oracle.c"), os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libbox_oracle.so")
FIELDS = ("instance", "triangle")
AXES = ("Ex", "Ey", "Ez", "N") + tuple("E%sxF%d" % (m, n) for m in "xyz" for n in range(3))
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
            L.orcb_pair.argtypes = [C.c_void_p] * 4
            L.orcb_pair.restype = C.c_int
            L.orcb_corners.argtypes = [C.c_void_p] * 3
            L.orcb_corners.restype = None
            L.orcb_count_in_boxes.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
            L.orcb_count_in_boxes.restype = None
            L.orcb_list_in_boxes.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 3
            L.orcb_list_in_boxes.restype = None
            _lib = L
    return _lib


def pair(box, tri, pose=(0.0,) * 6):
    """rule 11 on one pair: box [2, 3] world (lo, hi), pose [6] the instance's world -> mesh map, tri [3, 3] in scaled mesh space ->
    (pair, why): why is "pair", "invalid" (step 1), "boxes" (step 4) or the name of the first separating axis (AXES)"""
    b, p, t = (np.ascontiguousarray(a, np.float32).reshape(k) for a, k in ((box, 6), (pose, 6), (tri, 9)))
    which = C.c_int(0)
    hit = lib().orcb_pair(b.ctypes.data, p.ctypes.data, t.ctypes.data, C.addressof(which))
    w = which.value
    return bool(hit), "invalid" if w < 0 else "pair" if w == 0 else "boxes" if w == 1 else AXES[w - 2]


def corners(box, pose=(0.0,) * 6):
    """rule 11 step 2's mapped corners C0..C7 [8, 3] of one box under one pose"""
    b, p = (np.ascontiguousarray(a, np.float32).reshape(6) for a in (box, pose))
    out = np.zeros((8, 3), np.float32)
    lib().orcb_corners(b.ctypes.data, p.ctypes.data, out.ctypes.data)
    return out


def _in(boxes):
    return np.ascontiguousarray(boxes, np.float32).reshape(-1, 2, 3)


def count_in_boxes(scene, boxes, threads=8):
    """The number of pairs of every box (int32, flat)"""
    L = lib()
    b = _in(boxes)
    cnt = np.zeros(len(b), np.int32)

    def run(a, e):
        L.orcb_count_in_boxes(scene.h, e - a, b[a:].ctypes.data, cnt[a:].ctypes.data)
    _parallel(len(b), 16, run, threads)
    return cnt


def rooms(scene, boxes, offsets=None, max_hits=None, slots=None, fill=0, threads=8):
    """The rule on every box, written into rooms (offsets int64 [n + 1], or max_hits K: box i at [i*K, i*K + K)) of flat per-slot arrays
    of `slots` entries (default offsets[n] or n*K), each first set to `fill` -> dict of instance, triangle (flat) and count [n]."""
    L = lib()
    b = _in(boxes)
    n = len(b)
    off = None if offsets is None else np.ascontiguousarray(offsets, np.int64).reshape(n + 1)
    if slots is None:
        slots = int(off[n]) if off is not None else n * int(max_hits)
    out = {k: np.full(slots, fill, np.int32) for k in FIELDS}
    cnt = np.zeros(n, np.int32)

    def run(a, e):
        L.orcb_list_in_boxes(scene.h, e - a, b[a:].ctypes.data, None if off is None else off[a:].ctypes.data,
                             0 if max_hits is None else int(max_hits),
                             *[out[k].ctypes.data if off is not None else out[k][a * int(max_hits):].ctypes.data for k in FIELDS],
                             cnt[a:].ctypes.data)
    _parallel(n, 16, run, threads)
    out["count"] = cnt
    return out


def list_in_boxes(scene, boxes, max_hits=None, threads=8):
    """Shaped like the product's Scene.list_in_boxes: CSR (max_hits None: offsets, flat fields, query_index, count) or fixed rooms of
    max_hits (fields [..., K], count [...])."""
    b = np.ascontiguousarray(boxes, np.float32)
    lead = b.shape[:-2]
    if max_hits is None:
        c = count_in_boxes(scene, b, threads=threads)
        off = np.concatenate([[0], np.cumsum(c, dtype=np.int64)]).astype(np.int64)
        r = rooms(scene, b, offsets=off, threads=threads)
        assert np.array_equal(r["count"], c)
        r["offsets"] = off
        r["query_index"] = np.repeat(np.arange(len(c), dtype=np.int32), c)
        r["count"] = r["count"].reshape(lead)
        return r
    r = rooms(scene, b, max_hits=max_hits, threads=threads)
    res = {k: r[k].reshape(lead + (max_hits,)) for k in FIELDS}
    res["count"] = r["count"].reshape(lead)
    return res


def grid_boxes(origin, spacing, dims):
    """The cells of rt_occupancy_grid as boxes [nz, ny, nx, 2, 3]: origin + float32(i) * spacing, the product rounded, then the sum"""
    o, s = np.asarray(origin, np.float32), np.asarray(spacing, np.float32)
    nx, ny, nz = (int(d) for d in dims)
    edge = [(o[a] + np.arange(n + 1, dtype=np.float32) * s[a]).astype(np.float32) for a, n in enumerate((nx, ny, nz))]
    b = np.zeros((nz, ny, nx, 2, 3), np.float32)
    for a, n in enumerate((nx, ny, nz)):
        shape = [1, 1, 1]
        shape[2 - a] = n
        b[..., 0, a] = edge[a][:-1].reshape(shape)
        b[..., 1, a] = edge[a][1:].reshape(shape)
    return b


def grid_cells(origin, spacing, dims, cells):
    """grid_boxes' boxes [m, 2, 3] of the cells with flat indices `cells` ((iz * ny + iy) * nx + ix) alone, by the same formula: for
    grids too large to make whole"""
    o, s = np.asarray(origin, np.float32), np.asarray(spacing, np.float32)
    nx, ny, nz = (int(d) for d in dims)
    c = np.asarray(cells, np.int64).reshape(-1)
    assert c.size == 0 or (0 <= c.min() and c.max() < nx * ny * nz)
    b = np.zeros((len(c), 2, 3), np.float32)
    for a, i in enumerate((c % nx, c // nx % ny, c // (nx * ny))):
        b[:, 0, a] = o[a] + i.astype(np.float32) * s[a]
        b[:, 1, a] = o[a] + (i + 1).astype(np.float32) * s[a]
    return b
