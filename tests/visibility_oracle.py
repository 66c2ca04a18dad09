"""The CPU oracle of visibility masks (rt_visibility / Scene.visibility; the rule is in include/rt_hip.h, "visibility masks"): the
rule in numpy float32, every sum left to right, around ONE call of ray_oracle.cast_rays(..., lighting_pass=1, tmax=...) -- the
specification of rt_occluded.  TEST INFRASTRUCTURE ONLY: no shim of its own."""
import numpy as np

import ray_oracle

F = np.float32


def points_of(points, n):
    """[K, 3] or [n, K, 3] -> float32 [n, K, 3]"""
    P = np.asarray(points, F)
    assert P.ndim in (2, 3) and P.shape[-1] == 3 and 1 <= P.shape[-2] <= 32 and (P.ndim == 2 or P.shape[0] == n), P.shape
    return np.ascontiguousarray(np.broadcast_to(P, (n,) + P.shape[-2:]))


def rays(location, points, bias):
    """(L, v, tmax) of rules 1-4 for every (pixel, point): location [n, h, w, 3], points [n, K, 3] -> [n, h, w, K, 3] twice and
    [n, h, w, K]"""
    X = np.asarray(location, F)[:, :, :, None, :]
    L = np.ascontiguousarray(np.broadcast_to(np.asarray(points, F)[:, None, None, :, :], X.shape[:3] + points.shape[1:]))
    with np.errstate(all="ignore"):
        v = (X - L).astype(F)                                           # 1
        d = np.sqrt(((v[..., 0] * v[..., 0]).astype(F) + (v[..., 1] * v[..., 1]).astype(F)).astype(F) + (v[..., 2] * v[..., 2]).astype(F))    # 2
        s = F(1.0) - F(bias)                                            # 3
        tmax = (d.astype(F) * s).astype(F)                              # 4
    return L, np.ascontiguousarray(v), np.ascontiguousarray(tmax)


def pack(bits):
    """bool [..., K] -> int32 [...]: bit k from bits[..., k]"""
    K = bits.shape[-1]
    word = np.zeros(bits.shape[:-1], np.uint32)
    for k in range(K):
        word |= bits[..., k].astype(np.uint32) << np.uint32(k)
    return word.view(np.int32)


def occluded(scene, location, points, bias, threads=8):
    """uint8 [n, h, w, K]: the oracle's rt_occluded for every (pixel, point) ray of the rule, hit or not"""
    L, v, tmax = rays(location, points, bias)
    return ray_oracle.cast_rays(scene, L, v, lighting_pass=1, tmax=tmax, threads=threads)["occluded"]


def masks(scene, instance, location, normal, points, bias=2.0 ** -10, threads=8):
    """dict(visible, facing) int32 [n, h, w] (facing only with a normal plane); points [K, 3] or [n, K, 3]"""
    instance = np.asarray(instance, np.int32)
    n = instance.shape[0]
    P = points_of(points, n)
    hit = (instance >= 0)[..., None]
    out = dict(visible=pack((occluded(scene, location, P, bias, threads) == 0) & hit))      # 5, 8, 9
    if normal is not None:
        X = np.asarray(location, F)[:, :, :, None, :]
        N = np.asarray(normal, F)[:, :, :, None, :]
        with np.errstate(all="ignore"):
            w = (P[:, None, None, :, :] - X).astype(F)                  # 6
            dot = ((N[..., 0] * w[..., 0]).astype(F) + (N[..., 1] * w[..., 1]).astype(F)).astype(F) + (N[..., 2] * w[..., 2]).astype(F)
        out["facing"] = pack((dot.astype(F) > 0) & hit)                 # 7, 8, 9
    return out
