"""Point families for the closest-point tests (tests/test_gpu_point_query.py): drawn on the host from one seed, with the test oracle's
ray casts (tests/ray_oracle.c) supplying surface points.  Every point returned here is finite; the contract leaves non-finite points'
results unspecified."""
import numpy as np

import ray_oracle

F32 = np.float32


def _world(o, pose, scale, v):
    """mesh-space vertices v [k, 3] of an instance -> world (apply_lre(inv_pose, v * scale), the oracle's fp32 functions)"""
    inv = o.invert_lre(np.asarray(pose, F32))
    s = np.asarray(scale, F32)
    return np.stack([o.apply_lre(inv, (x * s).astype(F32)) for x in v]).astype(F32) if len(v) else np.zeros((0, 3), F32)


def ulp_steps(x, k):
    """x moved k float steps (k may be negative), elementwise"""
    x = np.asarray(x, F32).copy()
    for _ in range(abs(int(k))):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf)).astype(F32)
    return x


def scene_box(o, desc, so_meshes):
    """(lo, hi) of the scene's finite world vertices"""
    pts = []
    for mesh, _mat, pose, scale in desc.instances:
        t = o.mesh_dump(so_meshes[mesh])["tris"][:, :9].reshape(-1, 3)
        t = t[np.isfinite(t).all(axis=1)]
        if len(t):
            pts.append(_world(o, pose, scale, t[np.linspace(0, len(t) - 1, min(len(t), 300)).astype(int)]))
    p = np.concatenate(pts) if pts else np.zeros((1, 3), F32)
    return p.min(axis=0), p.max(axis=0)


def families(rng, o, desc, so, cam, n=600):
    """-> list of (name, points [m, 3] float32).  o: orc.oracle(); desc: the SceneDesc, after desc.build_oracle (so: its OracleScene);
    cam: (origins, directions) of a camera's primary rays."""
    meshes = desc.oracle_meshes
    lo, hi = scene_box(o, desc, meshes)
    diag = F32(max(float(np.linalg.norm((hi - lo).astype(np.float64))), 1e-3))
    org, dirs = (np.ascontiguousarray(a.reshape(-1, 3)) for a in cam)
    pick = rng.choice(len(org), min(len(org), n), replace=False)
    hit = ray_oracle.cast_rays(so, org[pick], dirs[pick], threads=8)
    ok = (hit["instance"] >= 0) & np.isfinite(hit["location"]).all(axis=1) & np.isfinite(hit["normal"]).all(axis=1)
    loc, nrm = hit["location"][ok], hit["normal"][ok]
    fams = []
    if len(loc):
        fams.append(("surface", loc))
        mag = np.maximum(np.abs(loc).max(axis=1, keepdims=True), F32(1e-30))
        u = (np.nextafter(mag, F32(np.inf)) - mag).astype(F32)
        fams.append(("surface_ulps", (loc + nrm * (u * F32(rng.choice([-3, -1, 1, 3])))).astype(F32)))
        fams.append(("surface_offset", (loc + nrm * (diag * F32(1e-3))).astype(F32)))
        fams.append(("surface_below", (loc - nrm * (diag * F32(1e-3))).astype(F32)))
    verts, mids, faces = [], [], []
    for mesh, _mat, pose, scale in desc.instances:
        d = o.mesh_dump(meshes[mesh])
        t = d["tris"][:, :9].reshape(-1, 3, 3)
        t = t[np.isfinite(t).all(axis=(1, 2))]
        if len(t):
            t = t[rng.choice(len(t), min(len(t), 40), replace=False)]
            verts.append(_world(o, pose, scale, t.reshape(-1, 3)))
            mids.append(_world(o, pose, scale, ((t[:, 0] + t[:, 1]) * F32(0.5)).astype(F32)))
        b = d["boxes"][1:]
        b = b[np.isfinite(b).all(axis=1) & (b[:, :3] <= b[:, 3:]).all(axis=1)]
        if len(b):
            b = b[rng.choice(len(b), min(len(b), 40), replace=False)]
            # a point on one face of the box (the others' coordinates inside it), then a few float steps either side
            p = (b[:, :3] + (b[:, 3:] - b[:, :3]) * rng.uniform(0, 1, (len(b), 3)).astype(F32)).astype(F32)
            ax = rng.integers(0, 3, len(b))
            side = rng.integers(0, 2, len(b))
            p[np.arange(len(b)), ax] = b[np.arange(len(b)), ax + 3 * side]
            w = _world(o, pose, scale, p)
            faces += [w, ulp_steps(w, 2), ulp_steps(w, -2), ulp_steps(w, 8), ulp_steps(w, -8)]
    if verts:
        fams.append(("vertices", np.concatenate(verts)))
        fams.append(("edge_midpoints", np.concatenate(mids)))
    if faces:
        fams.append(("box_faces", np.concatenate(faces)))
    span = np.maximum(hi - lo, F32(1e-3))
    fams.append(("in_box", (lo + span * rng.uniform(-0.1, 1.1, (n, 3))).astype(F32)))
    far = rng.normal(size=(n // 4, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * (float(diag) * 10.0 ** rng.uniform(0, 4, (n // 4, 1)))
    fams.append(("far", ((lo + hi) * F32(0.5) + far).astype(F32)))
    allp = np.concatenate([f[1] for f in fams])
    dup = allp[rng.integers(0, len(allp), n // 4)]
    fams.append(("duplicates", np.concatenate([dup, dup])))
    # 64-point blocks that are one point, or alternate between two far-apart points (the caller's wave = 64 consecutive points)
    blocks = []
    for k in range(4):
        a = allp[rng.integers(len(allp))]
        b = fams[-2][1][rng.integers(len(fams[-2][1]))]
        blocks.append(np.repeat(a[None], 64, axis=0) if k % 2 == 0 else np.where((np.arange(64) % 2 == 0)[:, None], a, b))
    fams.append(("blocks", np.concatenate(blocks).astype(F32)))
    return [(name, np.ascontiguousarray(p, F32)) for name, p in fams if len(p)]


def flatten(fams):
    """the families' points in one array whose last family (blocks) starts at a multiple of 64: its blocks are whole waves"""
    head = np.concatenate([f[1] for f in fams[:-1]])
    pad = (-len(head)) % 64
    return np.ascontiguousarray(np.concatenate([head, head[:pad], fams[-1][1]]), F32)


def special_bounds(rng, dist):
    """max_distance per point: +inf, 0, the exact distance and its float neighbours, NaN, negative, and random fractions"""
    n = len(dist)
    d = np.where(dist < np.finfo(F32).max, dist, F32(1.0)).astype(F32)
    kinds = rng.integers(0, 8, n)
    out = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3, kinds == 4, kinds == 5, kinds == 6],
                    [F32(np.inf), F32(0.0), d, np.nextafter(d, F32(0)), np.nextafter(d, F32(np.inf)), F32(np.nan), F32(-1.0)],
                    (d * rng.uniform(0.2, 2.0, n)).astype(F32))
    return np.ascontiguousarray(out, F32)
