"""Query-triangle families for the triangle-distance tests (tests/test_gpu_triangle_distance.py): drawn on the host from one seed, with
the test oracle's ray casts supplying surface points, as tests/query_segments.py draws segments.  Every triangle returned here is
finite; the contract leaves non-finite triangles' results unspecified."""
import numpy as np

import query_points as qp
import ray_oracle

F32 = np.float32


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _join(p0, p1, p2):
    return np.ascontiguousarray(np.stack([np.asarray(p0, F32), np.asarray(p1, F32), np.asarray(p2, F32)], axis=1), F32)


def _tangent(nn, rng):
    """a unit vector perpendicular to each unit nn"""
    t = np.cross(nn, _unit(rng, len(nn)))
    ln = np.linalg.norm(t, axis=1, keepdims=True)
    return np.where(ln > 1e-6, t / np.where(ln > 1e-6, ln, 1.0), np.cross(nn, np.array([1.0, 0.0, 0.0])))


def families(rng, o, desc, so, cam, n=300):
    """-> (list of (name, triangles [m, 3, 3] float32), scene diagonal).  o: orc.oracle(); desc: the SceneDesc after desc.build_oracle
    (so: its OracleScene); cam: (origins, directions) of a camera's primary rays.  About n triangles in all."""
    meshes = desc.oracle_meshes
    lo, hi = qp.scene_box(o, desc, meshes)
    diag = float(max(np.linalg.norm((hi - lo).astype(np.float64)), 1e-3))
    k = max(n // 16, 8)
    org, dirs = (np.ascontiguousarray(a.reshape(-1, 3)) for a in cam)
    pick = rng.choice(len(org), min(len(org), 4 * k), replace=False)
    hit = ray_oracle.cast_rays(so, org[pick], dirs[pick], threads=8)
    ok = (hit["instance"] >= 0) & np.isfinite(hit["location"]).all(axis=1) & np.isfinite(hit["normal"]).all(axis=1)
    loc, nrm = hit["location"][ok].astype(np.float64), hit["normal"][ok].astype(np.float64)
    fams = []
    if len(loc):
        # small triangles at surface points, offset along the normal
        off = (loc + nrm * (diag * 1e-3))[:, None] + rng.normal(size=(len(loc), 3, 3)) * (diag * 1e-3 * 0.5)
        fams.append(("surface_small", off.astype(F32)[:max(k, n // 8)]))
    tris = []
    for mesh, _mat, pose, scale in desc.instances:
        t = o.mesh_dump(meshes[mesh])["tris"][:, :9].reshape(-1, 3, 3)
        t = t[np.isfinite(t).all(axis=(1, 2))]
        if len(t):
            t = t[rng.choice(len(t), min(len(t), k), replace=False)]
            w = qp._world(o, pose, scale, t.reshape(-1, 3)).reshape(-1, 3, 3)
            tris.append(w[np.isfinite(w).all(axis=(1, 2))])
    tris = np.concatenate(tris).astype(np.float64) if tris else np.zeros((0, 3, 3))
    tris = tris[np.abs(tris).max(axis=(1, 2)) < 1e15] if len(tris) else tris
    if len(tris):
        tris = tris[rng.permutation(len(tris))[:k]]
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        nn = np.cross(b - a, c - a)
        ln = np.linalg.norm(nn, axis=1, keepdims=True)
        nn = np.where(ln > 0, nn / np.where(ln > 0, ln, 1.0), _unit(rng, len(tris)))
        size = np.maximum(np.linalg.norm(b - a, axis=1, keepdims=True), 1e-6 * diag)
        cen, mid = (a + b + c) / 3.0, (a + b) * 0.5
        tg = _tangent(nn, rng)
        out = np.cross(b - a, nn)                               # in the face's plane, away from it across the edge AB, |AB| long
        # above a face's interior, one vertex nearest: an (a) candidate
        top = cen + nn * size * 0.5
        fams.append(("vertex_nearest", _join(cen + nn * size * 0.05, top + tg * size * 0.2, top - tg * size * 0.2)))
        # an edge across a scene edge: over it in an X, and passing beside it along the normal ((c) candidates inside both edges)
        fams.append(("edge_across", np.concatenate([
            _join(mid - out * 0.3 + nn * size * 0.05, mid + out * 0.3 + nn * size * 0.05, mid + nn * size * 0.6),
            _join(mid - nn * size * 0.2 + out * 0.05, mid + nn * size * 0.3 + out * 0.05, mid + out * 0.6 + (b - a) * 0.1)])))
        # the interior hovering over a scene vertex, tilted away from the face, on either side of it (the winding does not say which
        # side is outside): a (b) candidate
        hover = []
        for side in (1.0, -1.0):
            away = a - cen
            away = away / np.maximum(np.linalg.norm(away, axis=1, keepdims=True), 1e-30) * 0.3 + nn * side
            away = away / np.maximum(np.linalg.norm(away, axis=1, keepdims=True), 1e-30)
            t1 = _tangent(away, rng)
            t2 = np.cross(away, t1)
            h = a + away * size * 0.1
            hover.append(_join(h + t1 * size * 0.2, h - t1 * size * 0.12 + t2 * size * 0.16, h - t1 * size * 0.12 - t2 * size * 0.16))
        fams.append(("hover_vertex", np.concatenate(hover)))
        # through a face; in a face's plane, overlapping it
        reach = size * rng.uniform(0.05, 0.5, (len(tris), 1))
        fams.append(("piercing", _join(cen - nn * reach, cen + nn * reach + tg * size * 0.1, cen + nn * reach - tg * size * 0.1)))
        shift = (b - a) * rng.uniform(-0.4, 0.4, (len(tris), 1))
        fams.append(("coplanar", _join(*((tris[:, j] - cen) * 0.6 + cen + shift for j in range(3)))))
    span = np.maximum((hi - lo).astype(np.float64), 1e-3)
    inside = lo + span * rng.uniform(-0.05, 1.05, (5 * k, 3))
    fams.append(("all_equal", _join(inside[:k], inside[:k], inside[:k])))
    p = inside[k:2 * k]
    q = p + _unit(rng, len(p)) * (diag * 0.05)
    fams.append(("two_equal", np.concatenate([_join(p, p, q), _join(p, q, q), _join(q, p, q)])[rng.permutation(3 * len(p))[:k]]))
    for j, (name, f) in enumerate((("size_1e-3", 1e-3), ("size_1e-1", 1e-1), ("size_2", 2.0))):
        p = inside[(j + 2) * k:(j + 3) * k]
        fams.append((name, _join(p, p + _unit(rng, len(p)) * (diag * f), p + _unit(rng, len(p)) * (diag * f))))
    far = (lo + hi) * 0.5 + _unit(rng, k) * (diag * 10.0 ** rng.uniform(0.5, 3, (k, 1)))
    fams.append(("outside", _join(far, far + _unit(rng, k) * (diag * rng.uniform(0.01, 1.0, (k, 1))),
                                  far + _unit(rng, k) * (diag * rng.uniform(0.01, 1.0, (k, 1))))))
    allt = np.concatenate([f[1] for f in fams]).astype(np.float64)
    some = allt[rng.integers(0, len(allt), k)]
    fams.append(("scaled_1e-10", (some * 1e-10).astype(F32)))
    fams.append(("scaled_1e10", (some * 1e10).astype(F32)))
    fams = [(name, np.ascontiguousarray(s, F32)) for name, s in fams if len(s)]
    return [(name, s[np.isfinite(s).all(axis=(1, 2))]) for name, s in fams], F32(diag)


def flatten(fams):
    return np.ascontiguousarray(np.concatenate([f[1] for f in fams]), F32)
