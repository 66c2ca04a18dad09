"""Sweep families for the sphere-sweep tests (tests/test_gpu_sweeps.py, tests/test_sweep_host.py): drawn on the host from one seed, with
the test oracle's ray casts supplying surface points.  Every segment returned here is finite (the contract leaves non-finite sweeps'
results unspecified); the radii include 0, +inf, NaN and negative values, which the rule defines."""
import numpy as np

import query_points as qp
import ray_oracle
from query_segments import _join, _unit

F32 = np.float32
OFFSETS = (0.5, 1.0, 1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, 2.0, 10.0)      # the start's height over the surface, in radii


def _boundary_first(rng, t, limit):
    """`limit` of the mesh triangles t [m, 3, 3], in random order but those with an edge no other triangle shares first, rotated so
    that this edge is AB: an open edge is where a sphere can touch an edge or a vertex before any face"""
    t = t[rng.permutation(len(t))]
    ends = np.stack([t, np.roll(t, -1, axis=1)], axis=2).reshape(-1, 2, 3)                  # edge j of triangle i at 3 i + j
    swap = (ends[:, 0].view(np.uint32).astype(np.int64) * np.array([1, 3, 7])).sum(1) > \
           (ends[:, 1].view(np.uint32).astype(np.int64) * np.array([1, 3, 7])).sum(1)
    ends[swap] = ends[swap][:, ::-1]
    keys = np.ascontiguousarray(ends.reshape(-1, 6)).view(np.dtype((np.void, 24))).ravel()
    _u, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    open_ = (cnt[inv] == 1).reshape(-1, 3)
    has = open_.any(axis=1)
    first = open_.argmax(axis=1)
    rot = np.stack([np.roll(t[i], -first[i], axis=0) for i in np.flatnonzero(has)[:limit]]) if has.any() else t[:0]
    return np.concatenate([rot[:limit // 2], t[~has][:limit], t[has][:limit]])[:limit]


def _aimed(rng, tris, diag, vertex):
    """one sweep per world triangle onto its edge AB (or its vertex A) from just outside the triangle's prism -> (segments, radius)"""
    a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
    nn = np.cross(b - a, c - a)
    ln = np.linalg.norm(nn, axis=1, keepdims=True)
    nn = np.where(ln > 0, nn / np.where(ln > 0, ln, 1.0), _unit(rng, len(tris)))
    size = np.maximum(np.linalg.norm(b - a, axis=1, keepdims=True), 1e-6 * diag)
    r = size * 10.0 ** rng.uniform(-1.5, -0.5, (len(tris), 1))
    e = (b - a) / size
    out = np.cross(e, nn)                                       # in the triangle's plane, away from it across the edge AB
    side = np.where(rng.random((len(tris), 1)) < 0.5, 1.0, -1.0)
    tilt = 10.0 ** rng.uniform(-3, 0.5, (len(tris), 1))
    corner = a - (a + b + c) / 3.0
    corner = corner / np.maximum(np.linalg.norm(corner, axis=1, keepdims=True), 1e-30)
    at, d = (a, nn * side + corner * tilt) if vertex else ((a + b) * 0.5, nn * side + out * tilt)
    return _join(at + d * (r * 5), at - d * r), np.ascontiguousarray(r[:, 0], F32)


def _features(rng, so, tris, diag, k):
    """Sweeps onto an edge and onto a vertex of the world triangles `tris`.  The feature is touched first only on an open edge, a
    convex crease or a corner (elsewhere a neighbour's face is), and a scene may have few of those, so many sweeps are drawn and the
    shim says which to keep: up to k whose winner is an edge, up to k whose winner is a vertex, and k of the others.  Where a first
    round finds too few, a second varies radius and direction on the triangles that gave one."""
    import sweep_oracle
    res = []
    for name, vertex, kinds in (("at_edge", False, (2, 3, 4)), ("at_vertex", True, (5, 6, 7))):
        found, others, pool = [], [], tris
        for _round in range(2):
            segs, rad = _aimed(rng, pool, diag, vertex)
            keep = np.isfinite(segs).all(axis=(1, 2))
            which = np.where(keep, sweep_oracle.sweep_spheres(so, segs, rad)["which"], -2)
            won = np.isin(which, kinds)
            found.append((segs[won], rad[won]))
            others.append((segs[keep & ~won], rad[keep & ~won]))
            if sum(len(f[0]) for f in found) >= k or not won.any():
                break
            pool = np.repeat(pool[won], 4 * k, axis=0)[:24 * k]
        for sub, parts in ((name, found), (name + "_others", others)):
            segs, rad = np.concatenate([q[0] for q in parts])[:k], np.concatenate([q[1] for q in parts])[:k]
            if len(segs):
                res.append((sub, np.ascontiguousarray(segs), np.ascontiguousarray(rad)))
    return res


def families(rng, o, desc, so, cam, n=300):
    """-> (list of (name, segments [m, 2, 3] float32, radius [m] float32), scene diagonal).  o: orc.oracle(); desc: the SceneDesc
    after desc.build_oracle (so: its OracleScene); cam: (origins, directions) of a camera's primary rays.  About n sweeps in all."""
    meshes = desc.oracle_meshes
    lo, hi = qp.scene_box(o, desc, meshes)
    diag = float(max(np.linalg.norm((hi - lo).astype(np.float64)), 1e-3))
    k = max(n // 20, 8)
    r0 = diag * 1e-2
    org, dirs = (np.ascontiguousarray(a.reshape(-1, 3)) for a in cam)
    pick = rng.choice(len(org), min(len(org), 6 * k), replace=False)
    hit = ray_oracle.cast_rays(so, org[pick], dirs[pick], threads=8)
    ok = (hit["instance"] >= 0) & np.isfinite(hit["location"]).all(axis=1) & np.isfinite(hit["normal"]).all(axis=1)
    loc, nrm = hit["location"][ok].astype(np.float64), hit["normal"][ok].astype(np.float64)
    fams = []

    def add(name, p0, p1, r):
        r = np.broadcast_to(np.asarray(r, np.float64), (len(p0),))
        fams.append((name, _join(p0, p1), np.ascontiguousarray(r, F32)))
    if len(loc) >= 2:
        loc, nrm = loc[:2 * k], nrm[:2 * k]
        h = np.array(OFFSETS)[rng.integers(0, len(OFFSETS), len(loc))][:, None]
        r = r0 * 10.0 ** rng.uniform(-1, 0.5, len(loc))
        start = loc + nrm * (h * r[:, None])
        add("surface_towards", start, loc - nrm * r[:, None], r)
        add("surface_away", start, start + nrm * (5.0 * r[:, None]) + _unit(rng, len(loc)) * r[:, None], r)
        add("surface_short", start[:k], start[:k] + _unit(rng, k)[:len(start[:k])] * (diag * 1e-3), np.full(len(start[:k]), diag * 1e-3))
    tris = []
    for mesh, _mat, pose, scale in desc.instances:
        t = o.mesh_dump(meshes[mesh])["tris"][:, :9].reshape(-1, 3, 3)
        t = t[np.isfinite(t).all(axis=(1, 2))]
        if len(t):
            t = _boundary_first(rng, t, 12 * k)
            w = qp._world(o, pose, scale, t.reshape(-1, 3)).reshape(-1, 3, 3)
            tris.append(w[np.isfinite(w).all(axis=(1, 2))])
    tris = np.concatenate(tris).astype(np.float64) if tris else np.zeros((0, 3, 3))
    tris = tris[np.abs(tris).max(axis=(1, 2)) < 1e15] if len(tris) else tris
    if len(tris):
        fams.extend(_features(rng, so, tris[:36 * k], diag, k))
        tris = tris[rng.permutation(len(tris))][:2 * k]
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        nn = np.cross(b - a, c - a)
        ln = np.linalg.norm(nn, axis=1, keepdims=True)
        nn = np.where(ln > 0, nn / np.where(ln > 0, ln, 1.0), _unit(rng, len(tris)))
        size = np.maximum(np.linalg.norm(b - a, axis=1, keepdims=True), 1e-6 * diag)
        r = (size * 10.0 ** rng.uniform(-1.5, -0.5, (len(tris), 1)))
        cen, mid = (a + b + c) / 3.0, (a + b) * 0.5
        e = (b - a) / size
        out = np.cross(e, nn)                                   # in the triangle's plane, away from it across the edge AB
        side = np.where(rng.random((len(tris), 1)) < 0.5, 1.0, -1.0)
        add("at_face", cen + nn * side * (r * 4 + size * 0.2), cen - nn * side * r, r[:, 0])
        hgt = np.stack([r[:, 0], np.nextafter(r[:, 0].astype(F32), F32(0)).astype(np.float64),
                        np.nextafter(r[:, 0].astype(F32), F32(np.inf)).astype(np.float64)])[rng.integers(0, 3, len(tris)), np.arange(len(tris))]
        add("grazing_face", cen + nn * hgt[:, None] - e * size * 2, cen + nn * hgt[:, None] + e * size * 2, r[:, 0])
        f = np.array([0.5, 1.0, 2.0])[rng.integers(0, 3, len(tris))][:, None]
        shift = (out * 0.8 + nn * 0.6) * (r * f)
        add("parallel_to_edge", a - e * size * 0.5 + shift, b + e * size * 0.5 + shift, r[:, 0])
    span = np.maximum((hi - lo).astype(np.float64), 1e-3)
    inside = lo + span * rng.uniform(-0.05, 1.05, (4 * k, 3))
    add("zero_length", inside[:k], inside[:k], r0 * 10.0 ** rng.uniform(-1, 1.5, k))
    for j, (name, f) in enumerate((("len_1e-3", 1e-3), ("len_1e-1", 1e-1), ("len_2", 2.0))):
        p = inside[(j + 1) * k:(j + 2) * k]
        add(name, p, p + _unit(rng, len(p)) * (diag * f), r0 * 10.0 ** rng.uniform(-1, 0.5, len(p)))
    far = (lo + hi) * 0.5 + _unit(rng, k) * (diag * 10.0 ** rng.uniform(0.5, 3, (k, 1)))
    add("outside", far, far + _unit(rng, k) * (diag * rng.uniform(0.01, 1.0, (k, 1))), r0)
    allp = np.concatenate([f[1] for f in fams]).astype(np.float64)
    allr = np.concatenate([f[2] for f in fams]).astype(np.float64)
    some = rng.integers(0, len(allp), k)
    fams.append(("scaled_1e-10", (allp[some] * 1e-10).astype(F32), (allr[some] * 1e-10).astype(F32)))
    fams.append(("scaled_1e10", (allp[some] * 1e10).astype(F32), (allr[some] * 1e10).astype(F32)))
    some = rng.integers(0, len(allp), 2 * k)
    special = np.array([0.0, 1e-30, diag * 1e-7, diag, np.inf, np.nan, -1.0, -0.0], F32)
    fams.append(("special_radii", allp[some].astype(F32), special[np.arange(2 * k) % len(special)]))
    out_ = []
    for name, s, r in fams:
        s = np.ascontiguousarray(s, F32)
        keep = np.isfinite(s).all(axis=(1, 2))
        if keep.any():
            out_.append((name, np.ascontiguousarray(s[keep]), np.ascontiguousarray(np.asarray(r, F32)[keep])))
    return out_, F32(diag)


def flatten(fams):
    """-> (segments [m, 2, 3], radius [m]) of all families"""
    return (np.ascontiguousarray(np.concatenate([f[1] for f in fams]), F32), np.ascontiguousarray(np.concatenate([f[2] for f in fams]), F32))
