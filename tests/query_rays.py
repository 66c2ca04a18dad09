"""Ray families for the ray-query fuzz (tests/test_gpu_ray_query_fuzz.py) and their CPU pins (tests/test_ray_query_host.py): the rays,
bounds and scenes are drawn on the host from one seed, with the test oracle's cast (tests/ray_oracle.c) supplying the hit locations
that later families aim at.  Every ray returned here has finite components: the contract leaves non-finite rays' results unspecified."""
import numpy as np

import ray_oracle
import scene_defs as sd

F32 = np.float32
FLT_MAX = np.finfo(F32).max
TINY = np.float32(np.finfo(F32).smallest_subnormal)


def _finite(o, d):
    keep = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
    return np.ascontiguousarray(o[keep], F32), np.ascontiguousarray(d[keep], F32)


def _units(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def octant_blocks(rng, o, d, blocks):
    """`blocks` blocks of 64 consecutive rays taken from (o, d), whose directions have no zero component: even blocks all in one world
    sign octant (the signs of the direction are set to it), odd blocks with the octant changing from lane to lane.  families() puts the
    first block at a multiple of 64, so in an unbinned call each block is one wave: an even block can take the hand-written loop on
    identity and translated instances (trace_instance: a usable, shared octant in mesh space), an odd one always falls back to the
    compiler's loop."""
    idx = rng.integers(0, len(o), blocks * 64)
    bo, bd = o[idx].copy(), np.abs(d[idx])
    lane = np.arange(blocks * 64)
    oct_ = np.where((lane // 64) % 2 == 0, np.repeat(rng.integers(0, 8, blocks), 64), lane % 8)
    for k in range(3):
        bd[:, k] = np.where((oct_ >> k) & 1, -bd[:, k], bd[:, k])
    return bo, bd.astype(F32)


def families(rng, so, cam_rays, n=4000):
    """-> list of (name, origins, directions), each float32 [m, 3] and finite.  so: the scene's orc.OracleScene; cam_rays: the camera's
    (origins, directions) [..., 3].  n scales every family (about 8 n rays in all, plus the camera's).  The flattened rays are a
    multiple of 64 long and the octant blocks come last, so that they are whole waves in one call and in repeated copies of it."""
    co, cd = _finite(cam_rays[0].reshape(-1, 3), cam_rays[1].reshape(-1, 3))
    out = [("camera", co, cd)]
    ref = ray_oracle.cast_rays(so, co, cd, threads=16)
    hit = ref["instance"] >= 0
    locs, norms = ref["location"][hit], ref["normal"][hit]
    ok = np.isfinite(locs).all(axis=1)
    locs, norms = locs[ok], norms[ok]
    if len(locs) == 0:
        locs = rng.uniform(-1, 1, (16, 3)).astype(F32)
        norms = _units(rng, 16)
    lo, hi = np.percentile(locs, 2, axis=0), np.percentile(locs, 98, axis=0)
    mid, half = (lo + hi) / 2, np.maximum((hi - lo) * 0.6, 1e-3 * max(1.0, float(np.abs(locs).max())))
    box = lambda m: (mid + rng.uniform(-1, 1, (m, 3)) * half).astype(F32)
    # origins in the box around the hits, aimed at earlier hit locations: the direction is the difference itself (not normalised)
    o = box(n)
    d = (locs[rng.integers(0, len(locs), n)] - o).astype(F32)
    out.append(("aimed", *_finite(o, d)))
    # the same with lengths 10^k, k in [-20, 18] (t stays the Euclidean world distance)
    o = box(n)
    with np.errstate(over="ignore"):
        d = (locs[rng.integers(0, len(locs), n)] - o).astype(F32) * np.power(10.0, rng.integers(-20, 19, (n, 1))).astype(F32)
    out.append(("scaled", *_finite(o, d)))
    # unit directions with +-0 components (one, two or all three of them zero)
    o = box(n // 2)
    d = _units(rng, n // 2)
    zero = rng.random((n // 2, 3)) < np.array([0.3, 0.3, 0.3])
    d = np.where(zero, np.where(rng.random((n // 2, 3)) < 0.5, F32(0.0), F32(-0.0)), d).astype(F32)
    d[:8] = np.where(rng.random((8, 3)) < 0.5, F32(0.0), F32(-0.0))     # all-zero directions: ordinary input (rt_hip.h)
    out.append(("signed_zero", o, d))
    # secondary rays from exactly the hit locations (no epsilon): back at the triangle, along its plane, away from it
    m = n // 3
    k = rng.integers(0, len(locs), 3 * m)
    side = np.cross(norms[k[m:2 * m]], rng.normal(size=(m, 3))).astype(F32)
    d = np.concatenate([-norms[k[:m]], side, norms[k[2 * m:]]]).astype(F32)
    out.append(("secondary", *_finite(locs[k].astype(F32), d)))
    # lattice origins and integer directions: rays along lattice edges, through lattice vertices, in lattice planes
    step = F32(rng.choice([0.25, 0.5, 1.0]))
    o = (rng.integers(-12, 13, (n // 2, 3)).astype(F32) * step).astype(F32)
    d = rng.integers(-2, 3, (n // 2, 3)).astype(F32)
    d[np.abs(d).sum(axis=1) == 0, 1] = 1.0
    extra = (sum(len(f[1]) for f in out) + len(o)) % 64       # (the lattice family ends at a multiple of 64)
    out.append(("lattice", o[:len(o) - extra], d[:len(d) - extra]))
    # blocks of 64 rays in one world octant, and blocks whose octant changes every lane (from the aimed rays: no zero component)
    nz = (out[1][2] != 0).all(axis=1)
    out.append(("octant_blocks", *octant_blocks(rng, out[1][1][nz], out[1][2][nz], max(2, n // 64))))
    return out


def flatten(fams):
    return np.concatenate([f[1] for f in fams]), np.concatenate([f[2] for f in fams])


def special_tmax(rng, n):
    """-1, -0.0, +0.0, the smallest subnormal, NaN, FLT_MAX, +inf and random values in [0, 3], cycled over n rays"""
    s = np.array([-1.0, -0.0, 0.0, TINY, np.nan, FLT_MAX, np.inf], F32)
    t = rng.uniform(0.0, 3.0, n).astype(F32)
    pick = rng.integers(0, len(s) + 3, n)
    return np.where(pick < len(s), s[np.minimum(pick, len(s) - 1)], t).astype(F32)


def around(t):
    """t, nextafter(t, -inf), nextafter(t, +inf) (float32)"""
    t = np.asarray(t, F32)
    with np.errstate(over="ignore"):
        return [t, np.nextafter(t, F32(-np.inf)), np.nextafter(t, F32(np.inf))]


def single_instance_distances(orc, desc, o, d):
    """Each instance's own closest-hit distance along every ray: the same rays cast on a copy of the scene that holds that instance
    alone (oracle).  -> list of float32 [m] (FLT_MAX where the instance is missed)."""
    out = []
    for inst in desc.instances:
        so = sd.SceneDesc(desc.materials, desc.meshes, [inst]).build_oracle(orc)
        try:
            out.append(ray_oracle.cast_rays(so, o, d, threads=16)["t"])
        finally:
            so.close()
    return out


def tmax_families(rng, orc, desc, o, d, closest_t):
    """-> list of (name, tmax float32 [m]): the closest hit and its neighbours, every instance's own closest hit and its neighbours
    (distances the full cast accepts: lanes reach their bound inside the loop with entries left on the stack), specials."""
    fams = [("closest%s" % s, t) for s, t in zip(("", "-", "+"), around(closest_t))]
    for k, tk in enumerate(single_instance_distances(orc, desc, o, d)):
        fams += [("instance%d%s" % (k, s), t) for s, t in zip(("", "-", "+"), around(tk))]
    fams.append(("special", special_tmax(rng, len(o))))
    return fams


def query_scene(scenes, seed):
    """The fuzz scene of test_fuzz_adversarial_queries[seed] -> (SceneDesc, W, H, K, camera pose, description)"""
    desc, W, H, K, cam_pose, info = sd.adversarial_scene(scenes, np.random.default_rng(83000 + seed))
    if seed % 6 == 5:                                           # (stacks that outgrow the LDS part, with per-lane origins)
        desc, W, H, K, cam_pose = sd.deep_stack_scene(28), 96, 64, scenes.scaled_K(96), (0.0, -1.0, 0.0, 0.0, 0.0, 0.0)
        info = "deep_stack_scene(28)"
    if seed % 4 == 3:
        tris = sd.random_triangles(50, seed=5, spread=0.6, size=0.5)
        tris[::3, 12] = 3.0e38                                  # (uv values past what the interpolation keeps: an exact-uv mesh)
        tris[1::7, 14] = FLT_MAX
        desc = sd.SceneDesc(desc.materials, desc.meshes + [("tris", tris)], desc.instances + [(len(desc.meshes), 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
        info += " + exact-uv mesh"
    return desc, W, H, K, cam_pose, info
