"""Point clouds without a device: every RT_E_INVALID case of rt_point_cloud_offsets(_table) and rt_point_cloud_fill that can be judged
without a scene is refused before anything is touched, rt_point_cloud_workspace_bytes is monotone in every argument, the Python
wrapper checks its arguments before any device call, and the shim behind the oracle's `local` (tests/point_cloud_oracle.c: the
oracle's own apply_lre, all three components) is pinned -- its z is gbuffer_oracle.depth bit for bit, an identity pose returns the
location, a rotation keeps the length."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import gbuffer_oracle
import point_cloud_oracle as pco

F32 = np.float32
FIELDS = ("range", "pixel", "frame", "instance", "triangle", "position", "local", "normal", "uv")
EVERY = 0x1ff
INF = float("inf")


def _cams(rt, n, w=16, h=8, sizes=None):
    cams = (rt.RtCameraParams * n)()
    for i in range(n):
        cams[i].width, cams[i].height = (w, h) if sizes is None else sizes[i]
    return cams


def test_the_struct_and_the_bits_follow_the_header(rt):
    assert [f[0] for f in rt.RtPointCloud._fields_] == list(rt.Camera.CLOUD_OUTPUTS) == list(rt.Sensor.CLOUD_OUTPUTS) == list(FIELDS) == list(pco.FIELDS)
    assert C.sizeof(rt.RtPointCloud) == 9 * C.sizeof(C.c_void_p)
    assert [rt.RT_CLOUD_BITS[k] for k in FIELDS] == [1, 2, 4, 8, 16, 32, 64, 128, 256]
    header = open(os.path.join(rt.ROOT, "include", "rt_hip.h")).read()
    for k, bit in rt.RT_CLOUD_BITS.items():
        assert "#define RT_CLOUD_%-8s 0x%03xu" % (k.upper(), bit) in header, k
    assert "#define RT_CLOUD_ALL      0x1ffu" in header
    for name in ("rt_point_cloud_workspace_bytes", "rt_point_cloud_offsets", "rt_point_cloud_offsets_table", "rt_point_cloud_fill"):
        assert hasattr(rt.libs()[0], name) and name in rt.RT_HIP_SYMBOLS
    for name in ("rth_camera_point_cloud_offsets", "rth_sensor_point_cloud_offsets", "rth_point_cloud_fill"):
        assert hasattr(rt.libs()[1], name) and name in rt.RT_HOST_SYMBOLS
    assert rt.libs()[0].rt_abi_version() == 2                            # the calls are additive


def test_offsets_rejects_bad_arguments(rt):
    """Every case with a scene handle (and a table handle) that is never dereferenced: each call has one bad argument."""
    h = rt.libs()[0]
    bogus, p, tab = C.c_void_p(16), C.c_void_p(64), C.c_void_p(32)
    cams = _cams(rt, 32)
    big = h.rt_point_cloud_workspace_bytes(16, 8, 32, EVERY)

    def both(scene, cams_, count, lo, hi, fields, offsets, ws, ws_bytes, table=tab):
        a = h.rt_point_cloud_offsets(scene, cams_, count, lo, hi, None, fields, offsets, ws, ws_bytes, None, 0)
        b = h.rt_point_cloud_offsets_table(scene, table, cams_, count, lo, hi, None, fields, offsets, ws, ws_bytes, None, 0)
        assert a == b
        return a

    assert both(None, cams, 2, 0.0, INF, 1, p, p, big) == -1                             # NULL scene
    assert both(bogus, None, 2, 0.0, INF, 1, p, p, big) == -1                            # NULL cams
    for count in (0, -1, 33, 2 ** 31 - 1):
        assert both(bogus, cams, count, 0.0, INF, 1, p, p, big) == -1                    # count outside 1..RT_MAX_BATCH
    assert both(bogus, _cams(rt, 3, sizes=[(16, 8), (16, 8), (16, 9)]), 3, 0.0, INF, 1, p, p, big) == -1      # sizes differ
    assert both(bogus, _cams(rt, 1, 0, 8), 1, 0.0, INF, 1, p, p, big) == -1              # an empty frame
    assert both(bogus, cams, 2, 0.0, INF, 1, None, p, big) == -1                         # NULL d_offsets
    assert both(bogus, cams, 2, 0.0, INF, 1, p, None, big) == -1                         # NULL workspace
    for fields in (1, 0x40, EVERY):
        need = h.rt_point_cloud_workspace_bytes(16, 8, 2, fields)
        assert need > 0 and both(bogus, cams, 2, 0.0, INF, fields, p, p, need - 1) == -1     # a workspace one byte short
    assert both(bogus, cams, 2, 0.0, INF, 0, p, p, big) == -1                            # no field
    for fields in (0x200, 0x201, 0x80000001, 0xffffffff):
        assert both(bogus, cams, 2, 0.0, INF, fields, p, p, big) == -1                   # unknown bits
    nan = float("nan")
    for lo, hi in ((nan, 1.0), (0.0, nan), (nan, nan), (2.0, 1.0), (INF, 1.0), (0.0, -INF)):
        assert both(bogus, cams, 2, lo, hi, 1, p, p, big) == -1                          # a NaN bound, min_range > max_range
    assert h.rt_point_cloud_offsets_table(bogus, None, cams, 2, 0.0, INF, None, 1, p, p, big, None, 0) == -1     # NULL table


def test_fill_rejects_bad_arguments(rt):
    """rt_point_cloud_fill takes no scene: every refusal is judged on the host, and a call with capacity 0 that is refused for
    nothing returns RT_OK without a launch"""
    h = rt.libs()[0]
    p = C.c_void_p(64)
    cams = _cams(rt, 32)
    big = h.rt_point_cloud_workspace_bytes(16, 8, 32, EVERY)
    out, none = rt.RtPointCloud(range=p), rt.RtPointCloud()
    call = h.rt_point_cloud_fill
    assert call(None, 2, 1, p, big, 0, C.byref(out), None, 0) == -1                      # NULL cams
    for count in (0, -1, 33):
        assert call(cams, count, 1, p, big, 0, C.byref(out), None, 0) == -1
    assert call(_cams(rt, 2, sizes=[(16, 8), (17, 8)]), 2, 1, p, big, 0, C.byref(out), None, 0) == -1
    assert call(_cams(rt, 1, 16, 0), 1, 1, p, big, 0, C.byref(out), None, 0) == -1
    assert call(cams, 2, 1, None, big, 0, C.byref(out), None, 0) == -1                   # NULL workspace
    assert call(cams, 2, 1, p, h.rt_point_cloud_workspace_bytes(16, 8, 2, 1) - 1, 0, C.byref(out), None, 0) == -1
    assert call(cams, 2, 0, p, big, 0, C.byref(out), None, 0) == -1                      # no field
    assert call(cams, 2, 0x201, p, big, 0, C.byref(out), None, 0) == -1                  # unknown bits
    assert call(cams, 2, 1, p, big, 0, None, None, 0) == -1                              # NULL out
    assert call(cams, 2, EVERY, p, big, 0, C.byref(none), None, 0) == -1                 # no output at all
    assert call(cams, 2, 1, p, big, -1, C.byref(out), None, 0) == -1                     # a negative capacity
    for k in FIELDS:                                                                     # a pointer whose bit is not in fields
        assert call(cams, 2, EVERY & ~rt.RT_CLOUD_BITS[k], p, big, 0, C.byref(rt.RtPointCloud(**{k: p})), None, 0) == -1, k
        assert call(cams, 2, rt.RT_CLOUD_BITS[k], p, big, 0, C.byref(rt.RtPointCloud(**{k: p})), None, 0) == 0, k
    assert call(cams, 2, EVERY, p, big, 0, C.byref(out), None, 0) == 0                   # a bit without a pointer is fine: not wanted


def test_workspace_bytes_is_monotone_and_zero_for_no_frame(rt):
    ws = rt.libs()[0].rt_point_cloud_workspace_bytes
    for w, h, n, f in ((0, 8, 1, 1), (8, 0, 1, 1), (-1, 8, 1, 1), (8, 8, 0, 1), (8, 8, -3, 1), (8, 8, 33, 1), (8, 8, 1, 0), (8, 8, 1, 0x200),
                       (2 ** 31 - 1, 2 ** 31 - 1, 32, 1)):
        assert ws(w, h, n, f) == 0, (w, h, n, f)
    sizes = (1, 7, 8, 9, 63, 64, 65, 640, 1920)
    for f in (1, 0x42, EVERY):
        for n in (1, 2, 31, 32):
            for a, b in zip(sizes, sizes[1:]):
                assert 0 < ws(a, 8, n, f) <= ws(b, 8, n, f) and 0 < ws(8, a, n, f) <= ws(8, b, n, f)
        for a, b in zip(range(1, 32), range(2, 33)):
            assert ws(37, 21, a, f) < ws(37, 21, b, f)
    for f in range(1, EVERY + 1):                                        # a field more never needs less; what stages a plane needs more
        for k, bit in rt.RT_CLOUD_BITS.items():
            if not f & bit:
                more = ws(37, 21, 4, f | bit)
                assert more >= ws(37, 21, 4, f)
                if k in ("triangle", "normal", "uv") or (k in ("position", "local") and not f & 0x60):
                    assert more > ws(37, 21, 4, f), (f, k)
    # the staged planes are in it: t and instance always, 12 bytes more per pixel for a location
    px = 32 * 1920 * 1080
    assert ws(1920, 1080, 32, 1) >= 8 * px and ws(1920, 1080, 32, 0x40) - ws(1920, 1080, 32, 1) >= 12 * px
    assert ws(1920, 1080, 32, 0x60) == ws(1920, 1080, 32, 0x40) == ws(1920, 1080, 32, 0x20)


def test_python_wrapper_checks_before_the_device(rt, scenes, monkeypatch):
    """Unknown, repeated or missing outputs, malformed poses, a mask of the wrong shape or type and a bad range gate raise ValueError
    before anything is staged or launched."""
    cam = rt.Camera(16, 8, scenes.scaled_K(16), scenes.D_REF)
    sc = rt.Scene()
    staged = []
    monkeypatch.setattr(rt, "_staging", lambda *a, **k: staged.append(1))
    for outs in (("range", "depth"), ("t",), ("local", "local"), (), ("offsets",), "range"):
        with pytest.raises(ValueError):
            cam.point_cloud(sc, outputs=outs)
    for poses in ([], [(0, 0, 0)], (0, 0, 0, 0, 0, 0), np.zeros((2, 3, 6)), np.zeros((0, 6))):
        with pytest.raises(ValueError):
            cam.point_cloud(sc, poses=poses)
    for mask in (np.ones((16, 8), bool), np.ones((8, 16, 1), bool), np.ones(128, np.uint8), np.ones((8, 16), np.float32), np.ones((8, 16), np.int32), 1):
        with pytest.raises(ValueError):
            cam.point_cloud(sc, mask=mask)
    for lo, hi in ((math.nan, 1.0), (0.0, math.nan), (2.0, 1.0), (math.inf, 0.0)):
        with pytest.raises(ValueError):
            cam.point_cloud(sc, min_range=lo, max_range=hi)
    assert not staged
    import inspect
    for owner in (rt.Camera, rt.Sensor):
        sig = inspect.signature(owner.point_cloud)
        assert list(sig.parameters) == ["self", "scene", "poses", "outputs", "min_range", "max_range", "mask", "stream", "as_numpy"]
        assert sig.parameters["outputs"].default == ("local", "range", "pixel") and sig.parameters["max_range"].default == math.inf
        assert owner.point_cloud.__doc__
    cam.close()
    sc.close()


def test_local_shim_z_is_the_depth_shim():
    """apply_lre's z through this shim and through gbuffer_oracle.depth on random poses and points: the same bits"""
    rng = np.random.default_rng(8)
    for _ in range(16):
        pose = np.concatenate([rng.uniform(-10, 10, 3), rng.uniform(-math.pi, math.pi, 3)]).astype(F32)
        loc = rng.uniform(-50, 50, (512, 3)).astype(F32)
        local = pco.apply_lre(pose, loc)
        assert local.dtype == F32 and local.shape == loc.shape
        depth = gbuffer_oracle.depth(pose, loc, np.zeros(512, np.int32))
        assert np.array_equal(local[:, 2].view(np.uint32), depth.view(np.uint32))
        # a rigid motion: the distance to the sensor is kept (to fp32 rounding of the products: a few ulp of the largest coordinate)
        d = np.linalg.norm((loc - pose[:3]).astype(np.float64), axis=1)
        assert np.abs(np.linalg.norm(local.astype(np.float64), axis=1) - d).max() <= 8 * float(np.spacing(F32(64.0)))
    ident = pco.apply_lre((0,) * 6, loc)
    assert np.array_equal(ident.view(np.uint32), loc.view(np.uint32))


def test_oracle_cloud_on_hand_made_planes():
    """the numpy reference itself on two 2 x 3 frames written by hand: keep rule, order, offsets, pixel and frame"""
    t = np.array([[[1, 2, 3], [4, 5, np.nan]], [[2, 2, 9], [1, 3, 3]]], F32)
    inst = np.array([[[0, -1, 0], [1, 0, 0]], [[0, 0, 0], [-1, 1, 0]]], np.int32)
    planes = dict(t=t, instance=inst, triangle=inst + 10, location=np.stack([t, t, t], -1), normal=np.zeros(t.shape + (3,), F32),
                  uv=np.zeros(t.shape + (2,), F32))
    poses = [(0,) * 6, (1, 0, 0, 0, 0, 0)]
    c = pco.cloud(planes, poses, min_range=2.0, max_range=5.0, mask=np.array([[1, 1, 1], [0, 2, 1]], np.uint8))
    assert c["offsets"].tolist() == [0, 2, 6] and c["offsets"].dtype == np.int64
    assert c["pixel"].tolist() == [2, 4, 0, 1, 4, 5] and c["frame"].tolist() == [0, 0, 1, 1, 1, 1]
    assert c["range"].tolist() == [3, 5, 2, 2, 3, 3] and c["triangle"].tolist() == [10, 10, 10, 10, 11, 10]
    assert c["local"][:2].tolist() == [[3, 3, 3], [5, 5, 5]] and c["local"][2].tolist() == [1, 2, 2]
