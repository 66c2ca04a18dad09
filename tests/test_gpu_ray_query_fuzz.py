"""Differential fuzzing of the ray queries (Scene.trace_rays / Scene.occluded / Camera.rays) against the test oracle's cast_ray_lp /
camera_ray (tests/ray_oracle.c), where the kernel is least comfortable: the awkward meshes and instance forms of the adversarial render
fuzz (mirrored, quarter-turn, signed-zero, 1e+-3 scales; lattices, piles, 1e18 / 1e-20 coordinates, slivers, non-finite vertices),
directions far from unit length or zero, per-lane bounds that equal distances the cast accepts, non-finite rays beside finite ones,
scene updates, and the shapes of a call.  Ray families and bounds: tests/query_rays.py."""
import contextlib
import os

import numpy as np
import pytest

import query_rays as qr
import ray_oracle
import scene_defs as sd

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
ALL = ("t", "instance", "triangle", "location", "normal", "uv", "pops")


def differing_rows(got, want):
    """Rows (first axis) where `got` and `want` differ bit for bit -- with one relaxation: any NaN equals any NaN, whatever its sign and
    payload (the GPU and x86 spell the default NaN differently, see test_gpu_ray_query._same_rays).  +0.0 and -0.0 stay distinct.
    -> int64 indices."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == F32:
        gn, wn = np.isnan(got), np.isnan(want)
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(gn & wn)
    else:
        bad = got != want
    return np.flatnonzero(bad.reshape(len(got), -1).any(axis=1)) if got.ndim else np.flatnonzero([bad])


def _numpy(v):
    return v.cpu().numpy() if hasattr(v, "cpu") else v


def _check(got, want, keys, where, rows=None, names=None):
    """every key of `got` equals `want` (differing_rows); rows: compare only these; names: a label per ray, for the message"""
    for k in keys:
        g, w = _numpy(got[k]), want[k]
        if rows is not None:
            g, w = g[rows], w[rows]
        bad = differing_rows(g, w)
        if bad.size:
            lab = "" if names is None else " families %s" % sorted(set(np.asarray(names if rows is None else names[rows])[bad[:200]]))
            raise AssertionError("%s %s: %d of %d rays differ%s, first %s: got %s want %s"
                                 % (where, k, bad.size, len(g), lab, bad[:3], g[bad[:3]], w[bad[:3]]))


@contextlib.contextmanager
def _scene(rt, orc, desc, gpu_build=False):
    """(oracle scene or None, uploaded product scene), both closed on the way out, also when the test fails"""
    so = desc.build_oracle(orc) if orc is not None else None
    sp = None
    try:
        sp = desc.build_product(rt, gpu_build=gpu_build)
        sp.upload_to_device()
        yield so, sp
    finally:
        if sp is not None:
            sp.close()
        if so is not None:
            so.close()


def _labels(fams):
    return np.concatenate([np.full(len(f[1]), f[0], dtype=object) for f in fams])


def _torch(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _check_occluded(sp, so, o, d, tfams, where, names):
    """occluded for every tmax family in one call (rays repeated per family) against the oracle: numpy unbinned, torch binned"""
    import torch
    O, D = np.tile(o, (len(tfams), 1)), np.tile(d, (len(tfams), 1))
    T = np.concatenate([t for _, t in tfams]).astype(F32)
    lab = np.concatenate([np.array(["%s/%s" % (tn, n) for n in names], dtype=object) for tn, _ in tfams])
    want = ray_oracle.cast_rays(so, O, D, lighting_pass=1, tmax=T, threads=16)["occluded"]
    got = sp.occluded(O, D, T, binning=False)
    _check({"occluded": got}, {"occluded": want}, ("occluded",), where + " occluded binning=False", names=lab)
    tO, tD, tT = _torch(O, D, T)
    got = sp.occluded(tO, tD, tT, binning=True)
    torch.cuda.synchronize()
    _check({"occluded": got}, {"occluded": want}, ("occluded",), where + " occluded binning=True (torch)", names=lab)


def _queries_against_oracle(orc, desc, so, sp, rng, fams, where):
    """all seven trace_rays outputs (binning off and on) and occluded over every tmax family, against the oracle"""
    o, d = qr.flatten(fams)
    names = _labels(fams)
    ref = ray_oracle.cast_rays(so, o, d, threads=16)
    for binning in (False, True):
        _check(sp.trace_rays(o, d, outputs=ALL, binning=binning), ref, ALL, "%s binning=%s" % (where, binning), names=names)
    _check_occluded(sp, so, o, d, qr.tmax_families(rng, orc, desc, o, d, ref["t"]), where, names)
    return ref


# RT_FUZZ_QUERY_SEEDS=n / RT_FUZZ_QUERY_FIRST=k: a campaign of the query fuzz below (the suite runs 12 seeds; tools/fuzz_adversarial_campaign.py)
_Q_FIRST = int(os.environ.get("RT_FUZZ_QUERY_FIRST", 0))
_RAYS = 5000                                                    # (query_rays.families: about 8x this many rays per scene, plus the camera's)


@pytest.mark.parametrize("seed", range(_Q_FIRST, _Q_FIRST + int(os.environ.get("RT_FUZZ_QUERY_SEEDS", 12))))
def test_fuzz_adversarial_queries(rt, orc, scenes, seed):
    """The adversarial scenes (numpy default_rng(83000 + seed); every fourth seed with an exact-uv mesh added, every sixth the deep-stack
    chain instead; trees from the GPU builder when seed % 3 == 2) queried with the families of query_rays (rays: default_rng(89000 + seed)):
    camera rays; random origins aimed at hit locations, not normalised, also scaled by 1e-20..1e18; unit directions with +-0 components
    and all-zero directions; secondary rays from exactly the hit points (into, along and away from the triangle); lattice origins with
    integer directions; blocks of 64 rays in one world octant beside blocks that change octant every lane.  All seven outputs binned and
    unbinned; occluded with tmax = the closest hit, every instance's own closest hit (a bound the cast meets inside its loop, with entries
    left on the stack) and their float neighbours, and -1 / -0 / +0 / subnormal / NaN / FLT_MAX / +inf / random."""
    desc, W, H, K, cam_pose, info = qr.query_scene(scenes, seed)
    print("seed", seed, info)
    rng = np.random.default_rng(89000 + seed)
    with _scene(rt, orc, desc, gpu_build=seed % 3 == 2) as (so, sp):
        fams = qr.families(rng, so, ray_oracle.camera_rays(W, H, K, scenes.D_REF, cam_pose), n=_RAYS)
        print("rays", {f[0]: len(f[1]) for f in fams})
        _queries_against_oracle(orc, desc, so, sp, rng, fams, "seed %d" % seed)


def _boundary_scenes(scenes, blob5k):
    tris = sd.random_triangles(300, seed=11, spread=0.8, size=0.3)
    overlap = sd.SceneDesc([((0.9, 0.5, 0.2), None)], [("obj", blob5k), ("tris", tris)],
                           [(0, 0, (0.1, 0.0, 0.05, 0.3, 0.2, -0.1), (1.0, 1.0, 1.0)),
                            (0, 0, (-0.1, 0.05, 0.0, -0.2, 0.4, 0.1), (0.9, 1.1, 1.0)),
                            (1, 0, (0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    half_pi = float(np.float32(np.pi / 2))
    mirrored = sd.SceneDesc([((0.9, 0.5, 0.2), None)], [("obj", blob5k), ("tris", tris)],
                            [(0, 0, (0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (-1.0, 1.0, 1.0)),
                             (1, 0, (0.3, -0.2, 0.1, 0.0, half_pi, 0.0), (1.0, -0.8, 1.2))])
    return [("overlapping posed instances", overlap), ("mirrored instance", mirrored)]


def test_occlusion_boundary(rt, scenes, blob5k):
    """No oracle: for every ray whose closest hit the GPU reports at t, occluded(tmax = t) is 0 (the bound is exclusive: a hit AT the
    bound does not occlude) and occluded(tmax = nextafter(t, +inf)) is 1; a miss is 0 for any tmax (+inf included).  Coherent waves
    (camera rays, also binned) and incoherent ones (random rays, unbinned and binned), on two overlapping posed instances and on a mirrored
    one.  (An inclusive bound, `hit.min <= tmax` in any_hit_done, reports 1 at tmax = t.)"""
    rng = np.random.default_rng(83500)
    for name, desc in _boundary_scenes(scenes, blob5k):
        with _scene(rt, None, desc) as (_, sp):
            cam = rt.Camera(320, 180, scenes.scaled_K(320), scenes.D_REF)
            cam.set_pose((0.0, -2.6, 0.2, 0.0, 0.0, 0.0))
            co, cd = (a.reshape(-1, 3).copy() for a in cam.rays(as_numpy=True))
            keep = np.isfinite(cd).all(axis=1)
            co, cd = co[keep], cd[keep]
            ro = rng.uniform(-1.5, 1.5, (60000, 3)).astype(F32)
            rd = rng.normal(size=(60000, 3)).astype(F32)
            for waves, o, d, binnings in (("camera", co, cd, (False, True)), ("random", ro, rd, (False, True))):
                for binning in binnings:
                    where = "%s, %s rays, binning=%s" % (name, waves, binning)
                    hits = sp.trace_rays(o, d, outputs=("t", "instance"), binning=binning)
                    t, hit = hits["t"], hits["instance"] >= 0
                    assert 0 < hit.sum() < len(hit), where
                    at = sp.occluded(o, d, t, binning=binning)
                    above = sp.occluded(o, d, qr.around(t)[2], binning=binning)
                    bad = np.flatnonzero(hit & (at != 0))
                    assert bad.size == 0, "%s: occluded(tmax = t) is 1 on %d hits, first %s t %s" % (where, bad.size, bad[:3], t[bad[:3]])
                    bad = np.flatnonzero(hit & (above != 1))
                    assert bad.size == 0, "%s: occluded(tmax = nextafter(t)) is 0 on %d hits, first %s t %s" % (where, bad.size, bad[:3], t[bad[:3]])
                    anyt = qr.special_tmax(rng, len(o))
                    anyt[::5] = np.inf
                    anyt[1::5] = FLT_MAX
                    assert not (above[~hit].any() or sp.occluded(o, d, anyt, binning=binning)[~hit].any()), where


def _poison(rng, o, d):
    """one ray with a NaN or +-inf component in the middle of every 64-ray block -> (o', d', poisoned mask)"""
    o, d = o.copy(), d.copy()
    idx = np.arange(32, len(o), 64)
    comp = rng.integers(0, 6, len(idx))
    val = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), len(idx))
    o[idx[comp < 3], comp[comp < 3]] = val[comp < 3]
    d[idx[comp >= 3], comp[comp >= 3] - 3] = val[comp >= 3]
    bad = np.zeros(len(o), bool)
    bad[idx] = True
    return o, d, bad


def test_nonfinite_rays_leave_other_rays_alone(rt, orc, scenes, blob5k):
    """A ray with a NaN or +-inf component in the middle of every 64-ray block: both calls return OK, and every finite ray's outputs
    equal the oracle's and those of the same call without the poisoned rays (theirs are unspecified and not looked at).  Every poisoned
    wave runs the compiler's generic loop (trace_instance: the ballot over `usable` fails), so this also checks that the generic loop gives
    the hand-written loop's bits on rays that otherwise never leave it.
    Why no index can leave its array: a non-finite ray changes only arithmetic.  slab() returns its near distance or FLT_MAX and never
    NaN (a NaN product fails `dst_far >= dst_near`, and fminf / fmaxf drop single NaNs), so `dist < hit.min` merely chooses among the
    two child references the record holds; what is pushed, popped and fetched are those references, one push per interior node on the
    path, at most the tree's depth (kMaxStack); a leaf's triangle count comes from its reference.  hit.min stays FLT_MAX unless a
    candidate passes `dist < hit.min`, which a NaN distance does not, and hit.slot changes with hit.instance only, so the epilogue reads
    tri_id / tri_uv for accepted hits alone.  The output index comes from the lane's LDS column, not from the ray."""
    import torch
    rng = np.random.default_rng(83600)
    m = sd.MULTI_CAMERA
    cases = [("blob5k", sd.blob_scene(scenes, blob5k), 320, 180, scenes.C2_CAMERAS["mid"], 1.2),
             ("multi", sd.multi_instance_scene(scenes, blob5k), m["width"], m["height"], m["pose"], 2.0)]
    for name, desc, W, H, pose, box in cases:
        with _scene(rt, orc, desc) as (so, sp):
            co, cd = (a.reshape(-1, 3) for a in ray_oracle.camera_rays(W, H, scenes.scaled_K(W), scenes.D_REF, pose))
            ro = rng.uniform(-box, box, (40000, 3)).astype(F32)
            rd = rng.normal(size=(40000, 3)).astype(F32)
            for waves, o, d in (("camera", co, cd), ("random", ro, rd)):
                ok = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1)
                o, d = np.ascontiguousarray(o[ok]), np.ascontiguousarray(d[ok])
                po, pd, bad = _poison(rng, o, d)
                keep = ~bad
                ref = ray_oracle.cast_rays(so, o, d, threads=16)
                tmax = ref["t"].copy()
                tmax[1::3] = qr.around(tmax[1::3])[2]
                tmax[2::3] = qr.special_tmax(rng, len(tmax[2::3]))
                oref = ray_oracle.cast_rays(so, o, d, lighting_pass=1, tmax=tmax, threads=16)["occluded"]
                assert (ref["instance"][keep] >= 0).any() and oref[keep].any(), (name, waves)
                for binning in (False, True):
                    where = "%s %s rays binning=%s" % (name, waves, binning)
                    clean = sp.trace_rays(o, d, outputs=ALL, binning=binning)
                    if binning:
                        got = {k: v.cpu().numpy() for k, v in sp.trace_rays(*_torch(po, pd), outputs=ALL, binning=True).items()}
                    else:
                        got = sp.trace_rays(po, pd, outputs=ALL, binning=False)
                    _check(clean, ref, ALL, where + " unpoisoned vs oracle")
                    _check(got, ref, ALL, where + " poisoned vs oracle", rows=keep)
                    _check(got, clean, ALL, where + " poisoned vs unpoisoned", rows=keep)
                    oclean = sp.occluded(o, d, tmax, binning=binning)
                    ogot = sp.occluded(po, pd, tmax, binning=binning)
                    _check({"o": oclean}, {"o": oref}, ("o",), where + " occluded unpoisoned vs oracle")
                    _check({"o": ogot}, {"o": oref}, ("o",), where + " occluded poisoned vs oracle", rows=keep)
            torch.cuda.synchronize()


@pytest.mark.parametrize("seed", range(4))
def test_queries_follow_adversarial_updates(rt, orc, scenes, seed):
    """The sequence of test_fuzz_adversarial_refit_and_rebuild on fresh seeds (numpy default_rng(86000 + seed); other poses from
    default_rng(87000 + seed)): an awkward scene, its first mesh refitted to another awkward mesh of the same count, uploaded again,
    rebuilt on the device from a third, then every instance given another awkward pose and scale -- the oracle mirrors each step
    (orc_mesh_refit on the same tree, a fresh mesh for the rebuild).  After each step trace_rays (all outputs) and occluded on the ray
    families of test_fuzz_adversarial_queries, against the oracle."""
    import orc as orc_mod
    o = orc_mod.oracle()
    rng = np.random.default_rng(86000 + seed)
    desc, W, H, K, cam_pose, info = sd.adversarial_scene(scenes, rng)
    n0 = len(desc.meshes[0][1])
    kind_b, b = sd.adversarial_mesh(o, rng)
    b = b[np.arange(n0) % len(b)]
    b_kept = b.copy()                                           # (a refit keeps the mesh's texture coordinates, rt_hip.h)
    b_kept[:, 12:18] = desc.meshes[0][1][:, 12:18]
    kind_c, c = sd.adversarial_mesh(o, rng)
    c = c[:n0]
    print("seed", seed, info, "refit to", kind_b, "rebuild from", kind_c, len(c))
    rays_rng = np.random.default_rng(88000 + seed)
    cam = ray_oracle.camera_rays(W, H, K, scenes.D_REF, cam_pose)

    def check(sp, so, d, what):
        fams = qr.families(rays_rng, so, cam, n=1200)
        _queries_against_oracle(orc, d, so, sp, rays_rng, fams, "seed %d %s" % (seed, what))

    with _scene(rt, orc, desc, gpu_build=seed % 2 == 1) as (so, sp):
        check(sp, so, desc, "as uploaded")
        sp.refit_mesh(0, b)
        o.mesh_refit(desc.oracle_meshes[0], b_kept)
        desc_b = sd.SceneDesc(desc.materials, [("tris", b_kept)] + list(desc.meshes[1:]), desc.instances)
        check(sp, so, desc_b, "refitted")
        sp.upload_to_device()
        check(sp, so, desc_b, "uploaded again after the refit")
        sp.rebuild_mesh(0, c)
        desc_c = sd.SceneDesc(desc.materials, [("tris", c)] + list(desc.meshes[1:]), desc.instances)
        so_c = desc_c.build_oracle(orc)
        try:
            check(sp, so_c, desc_c, "rebuilt")
            other = sd.adversarial_scene(scenes, np.random.default_rng(87000 + seed))[0].instances
            insts = []
            for i, (mesh, mat, _, _) in enumerate(desc.instances):
                pose, scale = other[i % len(other)][2], other[i % len(other)][3]
                sp.update_mesh_instance(i, mesh, mat, pose, scale, stream=False if i % 2 == 0 else None)
                so_c.update_instance(i, mesh, mat, pose, scale)
                insts.append((mesh, mat, pose, scale))
            check(sp, so_c, sd.SceneDesc(desc.materials, desc_c.meshes, insts), "instances updated")
        finally:
            so_c.close()


def _shape_rays(rng, n, pattern):
    o = rng.uniform(-1.2, 1.2, (n, 3)).astype(F32)
    d = np.abs(rng.normal(size=(n, 3))).astype(F32)
    oct_ = np.full(n, 5) if pattern == "one octant" else np.arange(n) % 8
    for k in range(3):
        d[:, k] = np.where((oct_ >> k) & 1, -d[:, k], d[:, k])
    return o, d


def test_call_shape_invariance(rt, orc, scenes, blob5k):
    """n in {1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17}, with every ray in one octant (seven empty buckets for the binning) or the
    octant changing every lane: the whole call against the oracle; the same rays as torch views 1-3 rays into a buffer (a base that is not
    16-byte aligned); every output requested alone gives the bits of all outputs together; a call split at an odd index gives the whole
    call's results (trace and occluded, binned and unbinned)."""
    import torch
    rng = np.random.default_rng(83700)
    with _scene(rt, orc, sd.blob_scene(scenes, blob5k)) as (so, sp):
        for n in (1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17):
            for pattern in ("one octant", "alternating"):
                o, d = _shape_rays(rng, n, pattern)
                where = "n=%d %s" % (n, pattern)
                ref = ray_oracle.cast_rays(so, o, d, threads=16)
                tmax = ref["t"].copy()
                tmax[1::2] = qr.around(tmax[1::2])[2]
                oref = ray_oracle.cast_rays(so, o, d, lighting_pass=1, tmax=tmax, threads=16)["occluded"]
                off = 1 + n % 3
                buf = torch.zeros(((n + off) * 3 + 2,), dtype=torch.float32, device="cuda")
                tb = torch.zeros((n + off + 1,), dtype=torch.float32, device="cuda")
                vo = buf[off * 3:(off + n) * 3].view(n, 3)
                vd = torch.zeros(((n + off) * 3,), dtype=torch.float32, device="cuda")[off * 3:].view(n, 3)
                vt = tb[off:off + n]
                vo.copy_(torch.from_numpy(o))
                vd.copy_(torch.from_numpy(d))
                vt.copy_(torch.from_numpy(tmax))
                assert vo.data_ptr() % 16 != 0 and vd.data_ptr() % 16 != 0 and vo.is_contiguous()
                for binning in (False, True):
                    whole = sp.trace_rays(o, d, outputs=ALL, binning=binning)
                    _check(whole, ref, ALL, where + " binning=%s" % binning)
                    view = sp.trace_rays(vo, vd, outputs=ALL, binning=binning)
                    torch.cuda.synchronize()
                    _check(view, ref, ALL, where + " torch view binning=%s" % binning)
                    assert np.array_equal(sp.occluded(o, d, tmax, binning=binning), oref), where
                    ov = sp.occluded(vo, vd, vt, binning=binning)
                    torch.cuda.synchronize()
                    assert np.array_equal(ov.cpu().numpy(), oref), where + " torch view"
                for k in ALL:
                    alone = sp.trace_rays(vo, vd, outputs=(k,), binning=(n + len(k)) % 2 == 1)
                    torch.cuda.synchronize()
                    assert set(alone) == {k}
                    _check(alone, ref, (k,), where + " %s requested alone" % k)
                if n > 1:
                    s = (n // 2) | 1 if n > 2 else 1
                    for binning in (False, True):
                        a = sp.trace_rays(o[:s].copy(), d[:s].copy(), outputs=ALL, binning=binning)
                        b = sp.trace_rays(o[s:].copy(), d[s:].copy(), outputs=ALL, binning=binning)
                        _check({k: np.concatenate([a[k], b[k]]) for k in ALL}, ref, ALL, where + " split at %d binning=%s" % (s, binning))
                        oc = np.concatenate([sp.occluded(o[:s].copy(), d[:s].copy(), tmax[:s].copy(), binning=binning),
                                             sp.occluded(o[s:].copy(), d[s:].copy(), tmax[s:].copy(), binning=binning)])
                        assert np.array_equal(oc, oref), where + " occluded split"
                assert (ref["instance"] >= 0).any() or n < 64, where


def test_camera_rays_fuzz(rt, scenes):
    """Camera.rays() against the oracle's camera_ray (numpy and torch paths): 1x1, 1xn, nx1, prime sizes and pixel counts that are not a
    multiple of 256; random principal points, some on a pixel centre (where the reference's ray is 0 / 0); D zero, D_REF and scaled;
    poses with signed zeros and quarter turns."""
    import torch
    rng = np.random.default_rng(83800)
    half_pi = float(np.float32(np.pi / 2))
    sizes = [(1, 1), (1, 37), (53, 1), (97, 61), (127, 7), (333, 190), (251, 3), (2, 509)]
    D_REF = np.asarray(scenes.D_REF, np.float64)
    nan_seen = 0
    for i, (W, H) in enumerate(sizes):
        f = rng.uniform(0.3, 2.0, 2) * max(W, H)
        if i % 2 == 0:
            cx, cy = float(rng.integers(0, W)), float(rng.integers(0, H))          # a pixel centre
        else:
            cx, cy = rng.uniform(-0.5, 1.5) * W, rng.uniform(-0.5, 1.5) * H
        K = (float(f[0]), 0.0, cx, 0.0, float(f[1]), cy, 0.0, 0.0, 1.0)
        D = [np.zeros(4), D_REF, D_REF * float(rng.choice([-3.0, 0.5, 8.0]))][i % 3]
        rot = [tuple(float(np.float32(-0.0)) if rng.random() < 0.5 else 0.0 for _ in range(3)),
               tuple(half_pi * float(v) for v in rng.integers(-2, 3, 3)),
               tuple(rng.uniform(-3.1, 3.1, 3))][i % 3]
        pos = tuple(float(np.float32(-0.0)) if rng.random() < 0.3 else float(v) for v in rng.uniform(-2, 2, 3))
        pose = pos + rot
        cam = rt.Camera(W, H, K, tuple(D))
        cam.set_pose(pose)
        ro, rd = ray_oracle.camera_rays(W, H, K, D, pose)
        o, d = cam.rays(as_numpy=True)
        where = "%dx%d K %s D %s pose %s" % (W, H, K, tuple(D), pose)
        to, td = cam.rays()
        torch.cuda.synchronize()
        assert o.shape == (H, W, 3) and to.shape == (H, W, 3), where
        for path, (go, gd) in (("numpy", (o, d)), ("torch", (to.cpu().numpy(), td.cpu().numpy()))):
            for what, g, r in (("origins", go, ro), ("directions", gd, rd)):
                bad = differing_rows(g.reshape(-1, 3), r.reshape(-1, 3))
                assert bad.size == 0, "%s %s %s: %d pixels differ, first %s" % (where, path, what, bad.size, bad[:3])
        nan_seen += int(np.isnan(rd).any())
    assert nan_seen > 0                                         # (at least one principal point on a pixel centre gave the 0 / 0 ray)
