"""Sensor frames without a device: every RT_E_INVALID case of the ray-table calls that can be judged without a table is refused with
handles that are never dereferenced (a size that differs from a table's needs a table: tests/test_gpu_sensor.py), the Python wrapper
checks its arguments before anything is staged, the ray shim (tests/sensor_oracle.c: the oracle's own invert_lre, apply_euler and
normalize3) is pinned, the generators of sensors.py have the geometry their docstrings state, and the tiled layout of a table is
restated in numpy."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import sensor_oracle

F32 = np.float32


@pytest.fixture(scope="module")
def sensors():
    return importlib.import_module("cuda-raytracing_amd.sensors")


def _poses(rt, n, w=16, h=8, sizes=None):
    cams = (rt.RtCameraParams * n)()
    for i in range(n):
        cams[i].width, cams[i].height = (w, h) if sizes is None else sizes[i]
    return cams


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    h, s = rt.libs()
    for name in ("rt_ray_table_create", "rt_ray_table_info", "rt_ray_table_destroy", "rt_camera_directions", "rt_ray_table_rays", "rt_render_gbuffer_table"):
        assert hasattr(h, name) and name in rt.RT_HIP_SYMBOLS, name
    for name in ("rth_sensor_create", "rth_sensor_destroy", "rth_sensor_set_pose", "rth_sensor_set_stream", "rth_sensor_rays", "rth_sensor_render_gbuffer",
                 "rth_camera_directions"):
        assert hasattr(s, name) and name in rt.RT_HOST_SYMBOLS, name
    p, bogus, tab = C.c_void_p(64), C.c_void_p(16), C.c_void_p(32)          # never dereferenced
    made = C.c_void_p()
    # rt_ray_table_create
    create = h.rt_ray_table_create
    assert create(None, 16, 8, None, 0, C.byref(made)) == -1                            # NULL d_dirs
    assert create(p, 16, 8, None, 0, None) == -1                                        # NULL out
    for w_, h_ in ((0, 8), (16, 0), (-1, 8), (16, -3)):
        assert create(p, w_, h_, None, 0, C.byref(made)) == -1                          # a size < 1
    assert create(p, 1, 65535 * 8 + 1, None, 0, C.byref(made)) == -1                    # 65 536 rows of tiles
    assert create(p, 4097 * 8, 4096 * 8 + 1, None, 0, C.byref(made)) == -1              # 4097 x 4097 tiles > 2^24
    assert made.value is None
    # rt_ray_table_info / destroy
    wi, hi, nb = C.c_int32(), C.c_int32(), C.c_size_t()
    assert h.rt_ray_table_info(None, C.byref(wi), C.byref(hi), C.byref(nb)) == -1
    assert h.rt_ray_table_destroy(None) == 0
    # rt_camera_directions
    assert h.rt_camera_directions(None, p, None, 0) == -1
    assert h.rt_camera_directions(_poses(rt, 1), None, None, 0) == -1
    assert h.rt_camera_directions(_poses(rt, 1, 0, 8), p, None, 0) == -1
    assert h.rt_camera_directions(_poses(rt, 1, 16, 0), p, None, 0) == -1
    # rt_ray_table_rays
    rays = h.rt_ray_table_rays
    assert rays(None, _poses(rt, 1), p, p, None, 0) == -1
    assert rays(tab, None, p, p, None, 0) == -1
    assert rays(tab, _poses(rt, 1), None, p, None, 0) == -1
    assert rays(tab, _poses(rt, 1), p, None, None, 0) == -1
    assert rays(tab, _poses(rt, 1, 0, 8), p, p, None, 0) == -1
    # rt_render_gbuffer_table: the cases of rt_render_gbuffer and a NULL table
    out, none = rt.RtGBuffer(t=p), rt.RtGBuffer()
    cams = _poses(rt, 32)
    imgs = (C.c_void_p * 32)(*[64 + i for i in range(32)])
    call = h.rt_render_gbuffer_table
    assert call(bogus, None, cams, 2, None, 0, C.byref(out), None, 0) == -1             # NULL table
    assert call(None, tab, cams, 2, None, 0, C.byref(out), None, 0) == -1               # NULL scene
    assert call(bogus, tab, None, 2, None, 0, C.byref(out), None, 0) == -1              # NULL poses
    assert call(bogus, tab, cams, 2, None, 0, None, None, 0) == -1                      # NULL out
    for count in (0, -1, 33, 2 ** 31 - 1):
        assert call(bogus, tab, cams, count, None, 0, C.byref(out), None, 0) == -1      # count outside 1..RT_MAX_BATCH
    assert call(bogus, tab, _poses(rt, 3, sizes=[(16, 8), (16, 8), (16, 9)]), 3, None, 0, C.byref(out), None, 0) == -1   # sizes differ
    assert call(bogus, tab, _poses(rt, 1, 0, 8), 1, None, 0, C.byref(out), None, 0) == -1
    assert call(bogus, tab, cams, 2, None, 0, C.byref(none), None, 0) == -1             # no plane and no images
    holed = (C.c_void_p * 3)(64, None, 66)
    assert call(bogus, tab, cams, 3, holed, 48, C.byref(out), None, 0) == -1            # a NULL entry in d_imgs
    assert call(bogus, tab, cams, 2, imgs, 47, C.byref(out), None, 0) == -1             # pitch < 3 * width
    assert call(bogus, tab, cams, 2, imgs, 0, C.byref(none), None, 0) == -1
    assert h.rt_abi_version() == 2
    # the facade refuses NULL handles and bad sizes before any device call
    d = np.zeros((8, 16, 3), F32)
    fp = d.ctypes.data_as(C.POINTER(C.c_float))
    assert s.rth_sensor_create(None, 16, 8, C.byref(made)) == -1
    assert s.rth_sensor_create(fp, 0, 8, C.byref(made)) == -1
    assert s.rth_sensor_create(fp, 16, 8, None) == -1
    assert s.rth_sensor_rays(None, None, p, p, None, 0) == -1
    assert s.rth_sensor_render_gbuffer(None, bogus, fp, 1, C.byref(out), None, 0, None, 0) == -1
    assert s.rth_camera_directions(None, p, None, 0) == -1


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    """Sensor() refuses malformed directions before the device; render_gbuffer and rays refuse what Camera.render_gbuffer refuses
    before anything is staged (a Sensor object without a table stands in: nothing reaches the library)."""
    staged = []
    monkeypatch.setattr(rt, "_staging", lambda *a, **k: staged.append(1))
    for bad in (np.zeros((8, 16), F32), np.zeros((8, 16, 2), F32), np.zeros((0, 16, 3), F32), np.zeros((8, 16, 3), np.float64), np.zeros((2, 8, 16, 3), F32)):
        with pytest.raises(ValueError):
            rt.Sensor(bad)
    sn = rt.Sensor.__new__(rt.Sensor)
    sn.h, sn.width, sn.height, sn._pose = None, 16, 8, [0.0] * 6
    sc = rt.Scene()
    for outs in (("t", "colour"), ("pops",), ("t", "t"), (), ("image",), "depth"):
        with pytest.raises(ValueError):
            sn.render_gbuffer(sc, outputs=outs)
    for poses in ([], [(0, 0, 0)], (0, 0, 0, 0, 0, 0), np.zeros((2, 3, 6)), np.zeros((0, 6))):
        with pytest.raises(ValueError):
            sn.render_gbuffer(sc, poses=poses)
    for pose in ((0, 0, 0), np.zeros((2, 6))):
        with pytest.raises(ValueError):
            sn.rays(pose)
    assert not staged
    assert rt.Sensor.GBUFFER_OUTPUTS == rt.Camera.GBUFFER_OUTPUTS
    sc.close()


# ---------------------------------------------------------------------------------------------------------------- the shim

def test_ray_shim_identity_pose_is_normalize3():
    rng = np.random.default_rng(5)
    c = (rng.normal(size=(4096, 3)) * rng.choice([1e-3, 1.0, 3.0], size=(4096, 1))).astype(F32)
    c[:6] = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    o, d = sensor_oracle.rays(c, (1.0, 2.0, 3.0, 0.0, 0.0, 0.0))
    assert np.array_equal(d.view(np.uint32), sensor_oracle.normalize(c).view(np.uint32))
    assert (o == np.array([1.0, 2.0, 3.0], F32)).all()
    # (normalize3 is the reference's: one Newton step on the bit-trick guess, utils.hpp:37-47 -- unit length to 0.2 %, not to an ulp)
    np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, rtol=0, atol=2e-3)


def _euler2quat64(e):
    """transforms.hpp:148-163 in float64: (w, x, y, z) of (yaw, pitch, roll)"""
    sy, cy, sp, cp, sr, cr = math.sin(e[0] / 2), math.cos(e[0] / 2), math.sin(e[1] / 2), math.cos(e[1] / 2), math.sin(e[2] / 2), math.cos(e[2] / 2)
    return (sy * sp * sr + cy * cp * cr, cy * sp * cr + sy * cp * sr, -sy * sp * cr + cy * cp * sr, cy * sp * sr - sy * cp * cr)


def _apply_quat64(q, v):
    """transforms.hpp:165-176 in float64 on v [n, 3]"""
    a = -v[:, 0] * q[1] - v[:, 1] * q[2] - v[:, 2] * q[3]
    b = v[:, 0] * q[0] + v[:, 1] * q[3] - v[:, 2] * q[2]
    c = v[:, 1] * q[0] + v[:, 2] * q[1] - v[:, 0] * q[3]
    d = v[:, 2] * q[0] + v[:, 0] * q[2] - v[:, 1] * q[1]
    return np.stack([q[0] * b - q[1] * a - q[2] * d + q[3] * c, q[0] * c - q[2] * a - q[3] * b + q[1] * d, q[0] * d - q[3] * a - q[1] * c + q[2] * b], 1)


def _normalize64(v):
    """normalize3 (utils.hpp:37-47) in float64: the reference normalises with q_rsqrt -- a first guess from the fp32 bit pattern of the
    squared length (an integer operation: it has no float64 form, so the squared length is narrowed for it) and one Newton step, here
    in float64.  The step squares the guess's error away, so the narrowing moves the result by far less than one fp32 rounding."""
    s = (v * v).sum(axis=1)
    y = (np.int32(0x5f3759df) - (s.astype(F32).view(np.int32) >> 1)).view(F32).astype(np.float64)
    y = y * (1.5 - 0.5 * s * y * y)
    return v * y[:, None]


def test_ray_shim_yawed_and_pitched_pose_against_float64(oracle):
    """Unit entries under a yawed and pitched pose: the shim against euler2quat, apply_quat and normalize3 evaluated in float64 on the
    angles of the oracle's own invert_lre(pose), taken as the fp32 numbers they are.  What is left is the fp32 rounding of the half
    angles, the six sines and cosines, the quaternion's products and sums, apply_quat's and normalize3's: a dozen roundings of at
    most 6e-8 each on numbers no larger than 1, so 1e-6 absolute."""
    rng = np.random.default_rng(6)
    c = rng.normal(size=(2000, 3))
    c = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(F32)
    pose = (0.5, -1.0, 2.0, 0.7, -0.3, 0.0)
    o, d = sensor_oracle.rays(c, pose)
    assert (o == np.array(pose[:3], F32)).all()
    inv = np.asarray(oracle.invert_lre([F32(v) for v in pose]), F32).astype(np.float64)
    assert abs(inv[3]) > 0.1 and abs(inv[4]) > 0.1                    # (both angles are at work)
    want = _normalize64(_apply_quat64(_euler2quat64(inv[3:]), c.astype(np.float64)))
    worst = np.abs(d.astype(np.float64) - want).max()
    print("ray shim against float64: worst %.3g" % worst)
    assert worst <= 1e-6
    assert np.abs(d - c).max() > 0.1                                  # (and the pose did turn them)


# ---------------------------------------------------------------------------------------------------------------- generators

def _unit(d, atol=1e-6):
    assert d.dtype == F32 and d.flags["C_CONTIGUOUS"] and np.isfinite(d).all()
    np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=-1), 1.0, rtol=0, atol=atol)


def test_equirectangular(sensors):
    d, valid = sensors.equirectangular(64, 24, with_mask=True)
    assert d.shape == (24, 64, 3) and valid.all()
    _unit(d)
    az = np.arctan2(d[..., 0].astype(np.float64), d[..., 1].astype(np.float64))
    el = np.arcsin(np.clip(d[..., 2].astype(np.float64), -1, 1))
    assert (np.diff(az, axis=1) > 0).all() and (np.diff(el, axis=0) < 0).all()             # azimuth grows with x, elevation falls with y
    np.testing.assert_allclose(az[5], -math.pi + (np.arange(64) + 0.5) / 64 * 2 * math.pi, atol=1e-6)
    np.testing.assert_allclose(el[:, 7], math.pi / 2 - (np.arange(24) + 0.5) / 24 * math.pi, atol=1e-6)
    # an odd width has a centre column: it looks along +y at the horizon
    e = sensors.equirectangular(65, 25)
    np.testing.assert_allclose(e[12, 32], (0, 1, 0), atol=1e-6)
    assert e[12, 40, 0] > 0 and e[3, 32, 2] > 0 and e[20, 32, 2] < 0                       # right of centre -> +x, top rows -> +z
    octants = {tuple(v) for v in (d.reshape(-1, 3) > 0)}
    assert len(octants) == 8
    part = sensors.equirectangular(16, 8, azimuth=(-0.5, 0.5), elevation=(-0.25, 0.25))
    _unit(part)
    assert (part[..., 1] > 0.8).all()


def test_spinning_lidar(sensors):
    els = np.radians(np.linspace(-15.0, 15.0, 16))
    d, valid = sensors.spinning_lidar(els, 128, with_mask=True)
    assert d.shape == (16, 128, 3) and valid.all()
    _unit(d)
    el = np.arcsin(d[..., 2].astype(np.float64))
    np.testing.assert_allclose(el, np.broadcast_to(els[:, None], el.shape), atol=1e-6)     # one constant elevation per row
    az = np.arctan2(d[..., 0].astype(np.float64), d[..., 1].astype(np.float64))
    assert (np.diff(az, axis=1) > 0).all()
    np.testing.assert_allclose(az[3], -math.pi + (np.arange(128) + 0.5) / 128 * 2 * math.pi, atol=1e-6)


def test_fisheye_equidistant(sensors):
    d, valid = sensors.fisheye_equidistant(33, 33, math.radians(180.0), with_mask=True)
    _unit(d)
    np.testing.assert_allclose(d[16, 16], (0, 1, 0), atol=1e-6)                             # the centre pixel looks along +y
    assert valid[16, 16] and not valid[0, 0] and not valid.all() and valid.sum() > 700
    assert (d[~valid] == np.array(sensors.FALLBACK, F32)).all()
    # equidistant: the angle off the axis is proportional to the distance from the centre, fov / 2 at the circle
    u, v = np.meshgrid(np.arange(33) + 0.5 - 16.5, np.arange(33) + 0.5 - 16.5)
    r = np.hypot(u, v)
    theta = np.arccos(np.clip(d[..., 1].astype(np.float64), -1, 1))
    np.testing.assert_allclose(theta[valid], r[valid] / 16.5 * math.pi / 2, atol=2e-6)
    assert d[16, 30, 0] > 0.5 and d[2, 16, 2] > 0.5 and d[30, 16, 2] < -0.5                 # right -> +x, top -> +z
    off = sensors.fisheye_equidistant(40, 24, 2.0, centre=(10.5, 8.5))
    np.testing.assert_allclose(off[8, 10], (0, 1, 0), atol=1e-6)


K_BC = (300.0, 0.0, 79.5, 0.0, 310.0, 59.5, 0.0, 0.0, 1.0)


def test_brown_conrady_without_distortion_is_the_pinhole(sensors):
    d, valid = sensors.brown_conrady(160, 120, K_BC, (0, 0, 0, 0), with_mask=True)
    assert valid.all()
    _unit(d)
    x, y = np.meshgrid(np.arange(160.0), np.arange(120.0))
    p = np.einsum("ij,hwj->hwi", np.linalg.inv(np.array(K_BC).reshape(3, 3)), np.stack([x, y, np.ones_like(x)], -1))
    want = np.stack([p[..., 0], p[..., 2], -p[..., 1]], -1)                                # raycast.cu:182
    want /= np.linalg.norm(want, axis=-1, keepdims=True)
    np.testing.assert_allclose(d.astype(np.float64), want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("dist", [(-0.28, 0.07, 0.0012, -0.0007), (-0.28, 0.07, 0.0012, -0.0007, 0.011), (0.09, -0.02, 0.0, 0.0)])
def test_brown_conrady_reprojects_to_its_pixel(sensors, dist):
    """the direction of every valid pixel, pushed through the forward model restated here (OpenCV's projectPoints), lands within
    1e-3 pixel of the pixel it came from"""
    d, valid = sensors.brown_conrady(160, 120, K_BC, dist, with_mask=True)
    _unit(d)
    assert valid.mean() > 0.9
    assert (d[~valid] == np.array(sensors.FALLBACK, F32)).all()
    d64 = d.astype(np.float64)
    xn, yn = d64[..., 0] / d64[..., 1], -d64[..., 2] / d64[..., 1]
    k1, k2, p1, p2 = dist[:4]
    k3 = dist[4] if len(dist) > 4 else 0.0
    r2 = xn * xn + yn * yn
    radial = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = xn * radial + 2 * p1 * xn * yn + p2 * (r2 + 2 * xn * xn)
    yd = yn * radial + p1 * (r2 + 2 * yn * yn) + 2 * p2 * xn * yn
    px, py = K_BC[0] * xd + K_BC[2], K_BC[4] * yd + K_BC[5]
    x, y = np.meshgrid(np.arange(160.0), np.arange(120.0))
    err = np.hypot(px - x, py - y)
    print("brown_conrady %s: worst re-projection error %.3g px over %d valid pixels" % (dist, err[valid].max(), valid.sum()))
    assert err[valid].max() <= 1e-3
    assert sensors.BROWN_CONRADY_ITERATIONS == 20 and "20 fixed-point iterations" in " ".join(sensors.brown_conrady.__doc__.split())


# ---------------------------------------------------------------------------------------------------------------- the layout

def pack(dirs):
    """The tiled layout of rt_hip.h restated: tile-major, one 8x8 tile = 3 x 64 floats, x / y / z planes 64 apart, tile index
    ty * tiles_x + tx, lane (y & 7) * 8 + (x & 7), room for whole tiles, lanes beyond a ragged edge (0, 1, 0)."""
    h, w = dirs.shape[:2]
    tx, ty = (w + 7) // 8, (h + 7) // 8
    out = np.full(tx * ty * 192, np.nan, F32)
    seen = np.zeros(out.size, bool)
    for y in range(ty * 8):
        for x in range(tx * 8):
            base = ((y // 8) * tx + x // 8) * 192 + (y & 7) * 8 + (x & 7)
            v = dirs[y, x] if (x < w and y < h) else (0.0, 1.0, 0.0)
            for k in range(3):
                assert not seen[base + 64 * k]
                seen[base + 64 * k] = True
                out[base + 64 * k] = v[k]
    assert seen.all()                                                   # every word of the table is some lane's: no holes, no overlap
    return out


@pytest.mark.parametrize("w,h", [(37, 21), (40, 24)])
def test_pack_layout_restated(w, h):
    """What rt_ray_table_info's device_bytes implies -- tiles_x * tiles_y * 768 bytes -- is exactly what the stated indexing covers.
    (The GPU test compares info's figure with the same formula and the table's contents, through its rays, with these directions.)"""
    rng = np.random.default_rng(w)
    d = rng.normal(size=(h, w, 3)).astype(F32)
    t = pack(d)
    assert t.nbytes == ((w + 7) // 8) * ((h + 7) // 8) * 768
    assert np.isfinite(t).all()
    # and back: pixel (x, y) is found where the kernels look for it
    for x, y in ((0, 0), (w - 1, h - 1), (8, 7), (7, 8), (w - 1, 0), (0, h - 1)):
        base = ((y // 8) * ((w + 7) // 8) + x // 8) * 192 + (y & 7) * 8 + (x & 7)
        assert (t[[base, base + 64, base + 128]] == d[y, x]).all()
    pad = ((w + 7) // 8 * 8) * ((h + 7) // 8 * 8) - w * h
    assert (t.reshape(-1, 3, 64)[:, 1, :] == 1.0).sum() >= pad
