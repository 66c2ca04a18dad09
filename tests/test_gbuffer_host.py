"""G-buffer frames without a device: every RT_E_INVALID case of rt_render_gbuffer is refused before the scene is touched, the Python
wrapper checks its arguments before any device call, and the depth shim (tests/gbuffer_oracle.c: the oracle's own apply_lre) is pinned
-- an identity pose gives the location's z exactly, a yawed pose agrees with float64."""
import ctypes as C

import numpy as np
import pytest

import gbuffer_oracle

F32 = np.float32
FLT_MAX = np.finfo(F32).max


def _cams(rt, n, w=16, h=8, sizes=None):
    cams = (rt.RtCameraParams * n)()
    for i in range(n):
        cams[i].width, cams[i].height = (w, h) if sizes is None else sizes[i]
    return cams


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    """Every RT_E_INVALID case of the header, with a scene handle that is never dereferenced.  The call is additive: the ABI version
    stays."""
    h = rt.libs()[0]
    assert hasattr(h, "rt_render_gbuffer") and "rt_render_gbuffer" in rt.RT_HIP_SYMBOLS
    assert [f[0] for f in rt.RtGBuffer._fields_] == list(rt.Camera.GBUFFER_OUTPUTS) == ["t", "depth", "instance", "triangle", "location", "normal", "uv"]
    assert C.sizeof(rt.RtGBuffer) == 7 * C.sizeof(C.c_void_p)
    p = C.c_void_p(64)
    bogus = C.c_void_p(16)
    out, none = rt.RtGBuffer(t=p), rt.RtGBuffer()
    cams = _cams(rt, 32)
    imgs = (C.c_void_p * 32)(*[64 + i for i in range(32)])
    call = h.rt_render_gbuffer
    assert call(None, cams, 2, None, 0, C.byref(out), None, 0) == -1                    # NULL scene
    assert call(bogus, None, 2, None, 0, C.byref(out), None, 0) == -1                   # NULL cams
    assert call(bogus, cams, 2, None, 0, None, None, 0) == -1                           # NULL out
    for count in (0, -1, 33, 2 ** 31 - 1):
        assert call(bogus, cams, count, None, 0, C.byref(out), None, 0) == -1           # count outside 1..RT_MAX_BATCH
    assert call(bogus, _cams(rt, 3, sizes=[(16, 8), (16, 8), (16, 9)]), 3, None, 0, C.byref(out), None, 0) == -1    # sizes differ
    assert call(bogus, _cams(rt, 2, sizes=[(16, 8), (17, 8)]), 2, None, 0, C.byref(out), None, 0) == -1
    assert call(bogus, _cams(rt, 1, 0, 8), 1, None, 0, C.byref(out), None, 0) == -1    # an empty frame
    assert call(bogus, cams, 2, None, 0, C.byref(none), None, 0) == -1                  # no plane and no images
    holed = (C.c_void_p * 3)(64, None, 66)
    assert call(bogus, cams, 3, holed, 48, C.byref(out), None, 0) == -1                 # a NULL entry in d_imgs
    assert call(bogus, cams, 3, holed, 48, C.byref(none), None, 0) == -1
    assert call(bogus, cams, 2, imgs, 47, C.byref(out), None, 0) == -1                  # pitch < 3 * width
    assert call(bogus, cams, 2, imgs, 0, C.byref(none), None, 0) == -1
    assert h.rt_abi_version() == 2
    s = rt.libs()[1]
    assert hasattr(s, "rth_camera_render_gbuffer") and "rth_camera_render_gbuffer" in rt.RT_HOST_SYMBOLS


def test_python_wrapper_checks_before_the_device(rt, scenes, monkeypatch):
    """Unknown, repeated or missing outputs and malformed poses raise ValueError before anything is staged or launched."""
    cam = rt.Camera(16, 8, scenes.scaled_K(16), scenes.D_REF)
    sc = rt.Scene()
    staged = []
    monkeypatch.setattr(rt, "_staging", lambda *a, **k: staged.append(1))
    for outs in (("t", "colour"), ("pops",), ("t", "t"), (), ("image",), "depth"):
        with pytest.raises(ValueError):
            cam.render_gbuffer(sc, outputs=outs)
    for poses in ([], [(0, 0, 0)], (0, 0, 0, 0, 0, 0), np.zeros((2, 3, 6)), np.zeros((0, 6))):
        with pytest.raises(ValueError):
            cam.render_gbuffer(sc, poses=poses)
    assert not staged
    assert rt.RT_MAX_BATCH == 32
    cam.close()
    sc.close()


def test_depth_shim_identity_pose_is_location_z():
    rng = np.random.default_rng(3)
    loc = rng.uniform(-50, 50, (4096, 3)).astype(F32)
    inst = rng.integers(-1, 3, 4096).astype(np.int32)
    assert (inst < 0).any() and (inst >= 0).any()
    d = gbuffer_oracle.depth((0,) * 6, loc, inst)
    assert d.dtype == F32 and np.array_equal(d[inst >= 0].view(np.uint32), loc[inst >= 0, 2].view(np.uint32))
    assert (d[inst < 0] == FLT_MAX).all()


def test_depth_shim_yawed_pose_against_float64(oracle):
    """A pose yawed by 0.7 rad: the shim's depth against the same quaternion product (transforms.hpp:165-176) evaluated in float64 on
    the SAME fp32 quaternion, the oracle's euler2quat of the pose's angles -- what is left is the rounding of apply_quat's fp32
    products and sums.  Bound: 2 ulp of the largest coordinate among the inputs (locations and locations - camera position).
    In exact arithmetic a yaw alone (the first Euler angle: a rotation about z) leaves z what it was, which the float64 side shows."""
    rng = np.random.default_rng(4)
    loc = rng.uniform(-20, 20, (2000, 3)).astype(F32)
    pose = (1.5, -2.0, 0.25, 0.7, 0.0, 0.0)
    d = gbuffer_oracle.depth(pose, loc, np.zeros(2000, np.int32)).astype(np.float64)
    q = np.asarray(oracle.euler2quat([F32(x) for x in pose[3:]]), F32).astype(np.float64)
    v = (loc - np.array(pose[:3], F32)).astype(np.float64)          # (the fp32 subtraction apply_lre makes: exact inputs of the product)
    a = -v[:, 0] * q[1] - v[:, 1] * q[2] - v[:, 2] * q[3]
    b = v[:, 0] * q[0] + v[:, 1] * q[3] - v[:, 2] * q[2]
    c = v[:, 1] * q[0] + v[:, 2] * q[1] - v[:, 0] * q[3]
    dd = v[:, 2] * q[0] + v[:, 0] * q[2] - v[:, 1] * q[1]
    want = q[0] * dd - q[3] * a - q[1] * c + q[2] * b
    np.testing.assert_allclose(want, v[:, 2] * (q ** 2).sum(), rtol=0, atol=1e-12)      # (|q|^2 is 1 up to the fp32 rounding of q)
    big = max(np.abs(loc).max(), np.abs(v).max())
    ulp = float(np.spacing(F32(big)))
    worst = np.abs(d - want).max() / ulp
    print("depth shim against float64: worst %.2f ulp of the largest coordinate %.3f" % (worst, big))
    assert worst <= 2.0
