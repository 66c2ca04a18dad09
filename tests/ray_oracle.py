"""ctypes bindings of tests/ray_oracle.c: the CPU oracle's cast_ray_lp and camera_ray on arbitrary rays (the specification of
rt_trace_rays / rt_occluded / rt_camera_rays).  TEST INFRASTRUCTURE ONLY.  The library is compiled with the oracle's flags
(oracle/Makefile) next to this file when it is missing or older than its sources, as orc.build_oracle() does for the oracle."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "ray_oracle.c")
DEPS = (SRC, os.path.join(ROOT, "oracle", "rt_oracle.c"))
SO = os.path.join(HERE, "libray_oracle.so")
FLAGS = ["-O2", "-std=gnu99", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-shared"]
OUTPUTS = ("t", "instance", "triangle", "location", "normal", "uv", "pops")
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
            L.orcx_cast_rays.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_void_p] * 7
            L.orcx_cast_rays.restype = None
            L.orcx_camera_rays.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            L.orcx_camera_rays.restype = None
            _lib = L
    return _lib


def _parallel(n, step, fn, threads):
    spans = [(a, min(a + step, n)) for a in range(0, n, step)]
    if threads <= 1 or len(spans) <= 1:
        for a, b in spans:
            fn(a, b)
        return
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(lambda ab: fn(*ab), spans))


def camera_rays(width, height, K, D, pose, threads=8):
    """(origins, directions) float32 [height, width, 3] of every pixel's primary ray (the oracle's camera_ray)."""
    L = lib()
    org = np.zeros((height, width, 3), np.float32)
    dirs = np.zeros((height, width, 3), np.float32)
    Kf, Df, Pf = (np.ascontiguousarray(v, np.float32) for v in (K, D, pose))
    _parallel(height, 8, lambda a, b: L.orcx_camera_rays(width, height, Kf.ctypes.data, Df.ctypes.data, Pf.ctypes.data, a, b,
                                                          org.ctypes.data, dirs.ctypes.data), threads)
    return org, dirs


def cast_rays(scene, origins, directions, lighting_pass=0, tmax=None, threads=8):
    """The oracle's cast_ray_lp on every ray of origins / directions [..., 3] (scene: an orc.OracleScene) -> dict of OUTPUTS
    shaped like the product's Scene.trace_rays; with lighting_pass, also `occluded` (uint8: an accepted hit below tmax)."""
    L = lib()
    o = np.ascontiguousarray(origins, np.float32)
    d = np.ascontiguousarray(directions, np.float32)
    lead = o.shape[:-1]
    n = int(np.prod(lead, dtype=np.int64))
    o, d = o.reshape(n, 3), d.reshape(n, 3)
    tm = None if tmax is None else np.ascontiguousarray(tmax, np.float32).reshape(n)
    out = dict(t=np.zeros(n, np.float32), instance=np.zeros(n, np.int32), triangle=np.zeros(n, np.int32),
               location=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), uv=np.zeros((n, 2), np.float32),
               pops=np.zeros(n, np.int32))

    def run(a, b):
        L.orcx_cast_rays(scene.h, b - a, o[a:].ctypes.data, d[a:].ctypes.data, lighting_pass, None if tm is None else tm[a:].ctypes.data,
                         *[out[k][a:].ctypes.data for k in OUTPUTS])
    _parallel(n, 4096, run, threads)
    if lighting_pass:
        bound = np.full(n, np.finfo(np.float32).max, np.float32) if tm is None else tm
        out["occluded"] = ((out["instance"] >= 0) & (out["t"] < bound)).astype(np.uint8)
    return {k: v.reshape(lead + v.shape[1:]) for k, v in out.items()}
