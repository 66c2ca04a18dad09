"""Ray queries without a GPU: the test oracle's cast of arbitrary rays (tests/ray_oracle.c) is pinned to the oracle's frames, and the
C-ABI and Python wrappers reject bad arguments before they touch a device (the GPU side: test_gpu_ray_query.py)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import ray_oracle
import scene_defs as sd

FLT_MAX = np.finfo(np.float32).max


def _pinned(orc, desc, W, H, K, D, pose):
    so = desc.build_oracle(orc)
    try:
        ref = so.render(W, H, K, D, pose, threads=8)
        org, dirs = ray_oracle.camera_rays(W, H, K, D, pose)
        got = ray_oracle.cast_rays(so, org, dirs)
        assert np.array_equal(got["instance"], ref["hit_inst"])
        assert np.array_equal(got["triangle"], ref["hit_tri"])
        assert np.array_equal(got["pops"], ref["pops"])
        assert ((got["t"] < FLT_MAX) == (got["instance"] >= 0)).all()
        occ = ray_oracle.cast_rays(so, org, dirs, lighting_pass=1)["occluded"]
        assert np.array_equal(occ, (got["t"] < FLT_MAX).astype(np.uint8))
        return got
    finally:
        so.close()


def test_shim_camera_casts_equal_oracle_frames(orc, scenes, blob5k):
    """orcx_camera_rays + orcx_cast_rays give orc_render's hit_inst / hit_tri / pops planes, pixel for pixel."""
    c1 = scenes.C1
    got = _pinned(orc, sd.c1_scene(scenes), c1["width"], c1["height"], c1["K"], c1["D"], c1["cam_pose"])
    assert (got["instance"] == 0).any()
    _pinned(orc, sd.blob_scene(scenes, blob5k), 320, 180, scenes.scaled_K(320), scenes.D_REF, scenes.C2_CAMERAS["mid"])
    m = sd.MULTI_CAMERA
    got = _pinned(orc, sd.multi_instance_scene(scenes, blob5k), m["width"], m["height"], scenes.scaled_K(m["width"]), scenes.D_REF, m["pose"])
    assert len(np.unique(got["instance"])) >= 3
    _pinned(orc, sd.deep_stack_scene(28), 96, 64, scenes.scaled_K(96), scenes.D_REF, (0.0, -1.0, 0.0, 0, 0, 0))


def test_shim_occlusion_bound(orc, scenes, blob5k):
    """lighting_pass with a per-ray bound: occluded exactly when a hit closer than the bound exists (= the closest hit is closer)."""
    so = sd.blob_scene(scenes, blob5k).build_oracle(orc)
    try:
        org, dirs = ray_oracle.camera_rays(64, 36, scenes.scaled_K(64), scenes.D_REF, scenes.C2_CAMERAS["mid"])
        closest = ray_oracle.cast_rays(so, org, dirs)
        rng = np.random.default_rng(3)
        with np.errstate(over="ignore"):
            tmax = (closest["t"] * rng.uniform(0.5, 1.5, closest["t"].shape)).astype(np.float32)
        tmax.flat[::7] = np.inf
        tmax.flat[::11] = 0.0
        occ = ray_oracle.cast_rays(so, org, dirs, lighting_pass=1, tmax=tmax)["occluded"]
        want = (closest["instance"] >= 0) & (closest["t"] < tmax)
        assert np.array_equal(occ, want.astype(np.uint8))
        assert 0 < occ.sum() < occ.size
    finally:
        so.close()


def test_c_abi_rejects_bad_arguments(rt):
    h = rt.libs()[0]
    hits = rt.RtRayHits()
    assert h.rt_trace_rays(None, None, None, 0, C.byref(hits), None, 0, None, 0) == -1            # NULL scene
    assert h.rt_occluded(None, None, None, None, 0, None, None, 0, None, 0) == -1
    # n < 0, NULL rays, a short workspace: refused before the scene is looked at (a handle that is never dereferenced)
    bogus = C.c_void_p(16)
    assert h.rt_trace_rays(bogus, None, None, -1, C.byref(hits), None, 0, None, 0) == -1
    assert h.rt_occluded(bogus, None, None, None, -5, None, None, 0, None, 0) == -1
    assert h.rt_trace_rays(bogus, None, None, 3, C.byref(hits), None, 0, None, 0) == -1
    assert h.rt_trace_rays(bogus, C.c_void_p(64), C.c_void_p(64), 3, None, None, 0, None, 0) == -1    # no RtRayHits
    assert h.rt_trace_rays(bogus, C.c_void_p(64), C.c_void_p(64), 3, C.byref(hits), C.c_void_p(64),
                           h.rt_trace_workspace_bytes(3) - 1, None, 0) == -1
    assert h.rt_occluded(bogus, C.c_void_p(64), C.c_void_p(64), None, 3, None, None, 0, None, 0) == -1    # no output
    assert h.rt_camera_rays(None, C.c_void_p(64), C.c_void_p(64), None, 0) == -1
    sizes = [h.rt_trace_workspace_bytes(n) for n in (0, 1, 63, 64, 4097, 1 << 24, 2 ** 31 - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
    assert sizes[-1] >= 4 * (2 ** 31 - 1)                                                         # (size_t: no overflow)
    assert h.rt_trace_workspace_bytes(-1) == 0


def test_python_wrappers_check_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    # the handle is never asked for: every bad call below fails in the argument check
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    o = np.zeros((10, 3), np.float32)
    bad = [(o.astype(np.float64), o), (o, o[:, :2].copy()), (o, np.zeros((11, 3), np.float32)), (o, np.zeros((3, 10), np.float32).T),
           (o.reshape(-1), o.reshape(-1)), (o, [[0, 0, 1]] * 10)]
    for a, b in bad:
        with pytest.raises(ValueError):
            s.trace_rays(a, b)
        with pytest.raises(ValueError):
            s.occluded(a, b)
    with pytest.raises(ValueError):
        s.trace_rays(o, o, outputs=("t", "colour"))
    with pytest.raises(ValueError):
        s.trace_rays(o, o, outputs=())
    with pytest.raises(ValueError):
        s.occluded(o, o, tmax=np.zeros(9, np.float32))
    with pytest.raises(ValueError):
        s.occluded(o, o, tmax=np.zeros(10, np.float64))
    torch = pytest.importorskip("torch")
    t = torch.zeros((10, 3), dtype=torch.float32)
    for a, b in [(t, t), (t, o), (t.double(), t), (torch.zeros((3, 10)).t(), t)]:
        with pytest.raises(ValueError):
            s.trace_rays(a, b)
    assert not touched
    s.close()


@pytest.mark.parametrize("seed", [0, 3, 5, 8])
def test_query_fuzz_rules_on_the_oracle(orc, scenes, seed):
    """What test_gpu_ray_query_fuzz.py relies on, pinned on the oracle (so that a GPU failure of these rules points at the kernel):
    the ray families and bounds of test_fuzz_adversarial_queries[seed] are the same on every draw, every family is non-empty and hits
    something; for every hit at t, occluded(tmax = t) is 0 and occluded(tmax = nextafter(t, +inf)) is 1, and a miss is never occluded."""
    import query_rays as qr
    desc, W, H, K, cam_pose, info = qr.query_scene(scenes, seed)
    so = desc.build_oracle(orc)
    try:
        cam = ray_oracle.camera_rays(W, H, K, scenes.D_REF, cam_pose)
        draws = []
        for _ in range(2):
            rng = np.random.default_rng(89000 + seed)
            fams = qr.families(rng, so, cam, n=600)
            o, d = qr.flatten(fams)
            ref = ray_oracle.cast_rays(so, o, d)
            tf = qr.tmax_families(rng, orc, desc, o, d, ref["t"])
            draws.append((fams, tf))
        (fa, ta), (fb, tb) = draws
        assert [f[0] for f in fa] == [f[0] for f in fb] and [t[0] for t in ta] == [t[0] for t in tb]
        for x, y in zip(fa, fb):
            assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) and np.array_equal(x[2].view(np.uint32), y[2].view(np.uint32)), x[0]
        for x, y in zip(ta, tb):
            assert np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)), x[0]
        assert len(ta) == 4 + 3 * len(desc.instances)
        # the octant blocks are whole waves of an unbinned call: the rays are a multiple of 64 long, and at least half the blocks'
        # aligned 64-ray slots hold one world octant with no zero direction component
        fo, fd = qr.flatten(fa)
        assert len(fo) % 64 == 0 and fa[-1][0] == "octant_blocks" and len(fa[-1][1]) % 64 == 0
        waves = fd.reshape(-1, 64, 3)
        coherent = (np.signbit(waves) == np.signbit(waves[:, :1])).all(axis=(1, 2)) & (waves != 0).all(axis=(1, 2))
        assert coherent[-len(fa[-1][1]) // 64:].sum() >= len(fa[-1][1]) // 128, info
        for name, fo, fd in fa:
            assert len(fo) > 0 and np.isfinite(fo).all() and np.isfinite(fd).all(), (info, name)
            assert (ray_oracle.cast_rays(so, fo, fd)["instance"] >= 0).any(), (info, name)
        hit = ref["instance"] >= 0
        t = ref["t"]
        at = ray_oracle.cast_rays(so, o, d, lighting_pass=1, tmax=t)["occluded"]
        above = ray_oracle.cast_rays(so, o, d, lighting_pass=1, tmax=qr.around(t)[2])["occluded"]
        assert not at[hit].any() and above[hit].all() and not above[~hit].any(), info
        anyt = qr.special_tmax(np.random.default_rng(seed), len(o))
        assert not ray_oracle.cast_rays(so, o, d, lighting_pass=1, tmax=anyt)["occluded"][~hit].any(), info
    finally:
        so.close()
