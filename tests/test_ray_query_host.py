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
