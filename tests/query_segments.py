"""Segment families for the segment-query tests (tests/test_gpu_segments.py): drawn on the host from one seed, with the test oracle's
ray casts supplying surface points.  Every segment returned here is finite; the contract leaves non-finite segments' results
unspecified."""
import numpy as np

import query_points as qp
import ray_oracle

F32 = np.float32


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _join(p0, p1):
    return np.ascontiguousarray(np.stack([np.asarray(p0, F32), np.asarray(p1, F32)], axis=1), F32)


def families(rng, o, desc, so, cam, n=300):
    """-> (list of (name, segments [m, 2, 3] float32), scene diagonal).  o: orc.oracle(); desc: the SceneDesc after desc.build_oracle
    (so: its OracleScene); cam: (origins, directions) of a camera's primary rays.  About n segments in all."""
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
    if len(loc) >= 2:
        # surface points offset along the normal, each joined to its neighbour's
        off = loc + nrm * (diag * 1e-3)
        fams.append(("surface_joined", _join(off[:-1], off[1:])[:k]))
        fams.append(("surface_short", _join(off, off + _unit(rng, len(off)) * (diag * 1e-3))[:max(k, n // 8)]))
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
        mid = (a + b) * 0.5
        fams.append(("along_edges", np.concatenate([_join(a, b), _join(a + (b - a) * 0.25 + nn * size * 0.01, a + (b - a) * 1.5 + nn * size * 0.01)])))
        out = np.cross(b - a, nn)
        fams.append(("across_edges", np.concatenate([_join(mid - out * 0.3 + nn * size * 0.05, mid + out * 0.3 + nn * size * 0.05),
                                                     _join(mid - nn * size * 0.2 + out * 0.05, mid + nn * size * 0.3 + out * 0.05)])))
        v = tris.reshape(-1, 3)
        fams.append(("vertex_pairs", _join(v[rng.integers(0, len(v), k)], v[rng.integers(0, len(v), k)])))
        cen = (a + b + c) / 3.0
        reach = size * rng.uniform(0.05, 0.5, (len(tris), 1))
        fams.append(("piercing", _join(cen - nn * reach, cen + nn * reach * rng.uniform(0.5, 2.0, (len(tris), 1)))))
    span = np.maximum((hi - lo).astype(np.float64), 1e-3)
    inside = lo + span * rng.uniform(-0.05, 1.05, (4 * k, 3))
    fams.append(("zero_length", _join(inside[:k], inside[:k])))
    for j, (name, f) in enumerate((("len_1e-3", 1e-3), ("len_1e-1", 1e-1), ("len_2", 2.0))):
        p = inside[(j + 1) * k:(j + 2) * k]
        fams.append((name, _join(p, p + _unit(rng, len(p)) * (diag * f))))
    far = (lo + hi) * 0.5 + _unit(rng, k) * (diag * 10.0 ** rng.uniform(0.5, 3, (k, 1)))
    fams.append(("outside", _join(far, far + _unit(rng, k) * (diag * rng.uniform(0.01, 1.0, (k, 1))))))
    allp = np.concatenate([f[1] for f in fams]).astype(np.float64)
    some = allp[rng.integers(0, len(allp), k)]
    fams.append(("scaled_1e-10", (some * 1e-10).astype(F32)))
    fams.append(("scaled_1e10", (some * 1e10).astype(F32)))
    fams = [(name, np.ascontiguousarray(s, F32)) for name, s in fams if len(s)]
    return [(name, s[np.isfinite(s).all(axis=(1, 2))]) for name, s in fams], F32(diag)


def flatten(fams):
    return np.ascontiguousarray(np.concatenate([f[1] for f in fams]), F32)

