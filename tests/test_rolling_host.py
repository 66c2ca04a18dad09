"""Rolling frames without a device: every RT_E_INVALID case of rt_render_gbuffer_rolling, rt_point_cloud_offsets_rolling and
rt_point_cloud_fill_rolling that can be judged without a scene (and without reading the table) is refused before anything is touched,
rt_rolling_slices handles ragged extents, the workspace sizes are monotone in every argument, the Python wrapper raises its
ValueErrors before any device call, and sensors.rolling_poses interpolates in float64 and rounds once."""
import ctypes as C
import importlib
import inspect
import math
import os

import numpy as np
import pytest

EVERY = 0x1ff
INF = float("inf")


@pytest.fixture(scope="module")
def sensors():
    return importlib.import_module("cuda-raytracing_amd.sensors")


def test_the_struct_and_the_symbols_follow_the_header(rt):
    assert C.sizeof(rt.RtRollingPose) == 48 and [f[0] for f in rt.RtRollingPose._fields_] == ["camera_pose", "inv_camera_pose"]
    header = open(os.path.join(rt.ROOT, "include", "rt_hip.h")).read()
    assert "typedef struct RtRollingPose" in header and "rolling frames" in header
    for name in ("rt_rolling_slices", "rt_rolling_workspace_bytes", "rt_render_gbuffer_rolling", "rt_point_cloud_rolling_workspace_bytes",
                 "rt_point_cloud_offsets_rolling", "rt_point_cloud_fill_rolling"):
        assert hasattr(rt.libs()[0], name) and name in rt.RT_HIP_SYMBOLS and name in header
    host = open(os.path.join(rt.ROOT, "include", "rt_host.h")).read()
    for name in ("rth_sensor_render_rolling", "rth_sensor_point_cloud_offsets_rolling", "rth_point_cloud_fill_rolling"):
        assert hasattr(rt.libs()[1], name) and name in rt.RT_HOST_SYMBOLS and name in host
    assert rt.libs()[0].rt_abi_version() == 2                            # the calls are additive
    assert rt.Sensor.ROLLING_OUTPUTS == rt.Sensor.GBUFFER_OUTPUTS + ("local",)


def test_slices_of_ragged_extents(rt):
    f = rt.libs()[0].rt_rolling_slices
    n = C.c_int32(-7)
    for w, h, axis, sp, want in ((128, 16, 0, 8, 16), (64, 24, 0, 16, 4), (64, 24, 1, 8, 3), (40, 24, 0, 16, 3), (13, 5, 0, 8, 2), (13, 5, 1, 8, 1),
                                 (8, 8, 0, 8, 1), (1, 1, 0, 8, 1), (1, 1, 1, 4096, 1), (2048, 1024, 0, 8, 256), (1920, 1080, 1, 8, 135),
                                 (9, 17, 0, 8, 2), (9, 17, 1, 8, 3), (9, 17, 1, 16, 2), (2 ** 31 - 1, 1, 0, 8, 2 ** 28)):
        assert f(w, h, axis, sp, C.byref(n)) == 0 and n.value == want, (w, h, axis, sp, n.value)
    n.value = -7
    for w, h, axis, sp in ((0, 8, 0, 8), (8, 0, 0, 8), (-1, 8, 0, 8), (8, 8, 2, 8), (8, 8, -1, 8), (8, 8, 0, 0), (8, 8, 0, 4), (8, 8, 0, 7), (8, 8, 0, 12),
                           (8, 8, 1, -8), (8, 8, 0, 9)):
        assert f(w, h, axis, sp, C.byref(n)) == -1 and n.value == -7, (w, h, axis, sp)
    assert f(8, 8, 0, 8, None) == -1


def test_workspace_sizes_are_monotone(rt):
    h = rt.libs()[0]
    ws, cws, static = h.rt_rolling_workspace_bytes, h.rt_point_cloud_rolling_workspace_bytes, h.rt_point_cloud_workspace_bytes
    for n, s in ((0, 4), (-1, 4), (33, 4), (4, 0), (4, -2)):
        assert ws(n, s) == 0 and cws(16, 8, n, 1, s) == 0, (n, s)
    for w, hh, n, f in ((0, 8, 1, 1), (8, 0, 1, 1), (8, 8, 1, 0), (8, 8, 1, 0x200)):
        assert cws(w, hh, n, f, 2) == 0
    for n in (1, 2, 31, 32):
        for a, b in zip((1, 2, 3, 16, 135, 256, 8192), (2, 3, 16, 135, 256, 8192, 2 ** 20)):
            assert 48 * n * a <= ws(n, a) <= ws(n, b) and ws(n, a) % 256 == 0
            assert cws(37, 21, n, EVERY, a) <= cws(37, 21, n, EVERY, b)
    for s in (1, 3, 256):
        for a, b in zip(range(1, 32), range(2, 33)):
            assert ws(a, s) <= ws(b, s) and cws(37, 21, a, 0x41, s) < cws(37, 21, b, 0x41, s)
        assert ws(1, s) < ws(32, s)
    assert ws(32, 256) == 32 * 256 * 48
    # the cloud workspace is the static one followed by the records
    for f in (1, 0x40, EVERY):
        for n, s in ((1, 1), (4, 16), (32, 256)):
            assert cws(37, 21, n, f, s) == static(37, 21, n, f) + ws(n, s)
    sizes = (1, 7, 8, 9, 63, 64, 65, 640)
    for a, b in zip(sizes, sizes[1:]):
        assert 0 < cws(a, 8, 2, EVERY, 4) <= cws(b, 8, 2, EVERY, 4) and 0 < cws(8, a, 2, EVERY, 4) <= cws(8, b, 2, EVERY, 4)


def test_render_rejects_bad_arguments(rt):
    """Every case with a scene and a table handle that are never dereferenced: each call has one bad argument."""
    h = rt.libs()[0]
    bogus, tab, p = C.c_void_p(16), C.c_void_p(32), C.c_void_p(64)
    poses = (rt.RtRollingPose * 64)()
    out, none = rt.RtGBuffer(t=p), rt.RtGBuffer()
    imgs, holed = (C.c_void_p * 2)(p, p), (C.c_void_p * 2)(p, None)

    def call(scene=bogus, table=tab, poses_=poses, count=2, axis=0, sp=8, d_imgs=None, pitch=0, out_=out, local=None, ws=p, ws_bytes=1 << 20):
        return h.rt_render_gbuffer_rolling(scene, table, poses_, count, axis, sp, d_imgs, pitch, C.byref(out_) if out_ is not None else None, local, ws,
                                           ws_bytes, None, 0)

    assert call(scene=None) == -1 and call(table=None) == -1 and call(poses_=None) == -1 and call(out_=None) == -1 and call(ws=None) == -1
    for count in (0, -1, 33, 2 ** 31 - 1):
        assert call(count=count) == -1
    for axis in (2, -1, 7):
        assert call(axis=axis) == -1
    for sp in (0, 4, 7, 9, 12, -8, -16):
        assert call(sp=sp) == -1
    assert call(out_=none) == -1                                         # no output at all
    assert call(out_=none, d_imgs=holed, pitch=4096) == -1               # a NULL entry in d_imgs


def test_cloud_calls_reject_bad_arguments(rt):
    h = rt.libs()[0]
    bogus, tab, p = C.c_void_p(16), C.c_void_p(32), C.c_void_p(64)
    poses = (rt.RtRollingPose * 64)()
    big = 1 << 24

    def offsets(scene=bogus, table=tab, poses_=poses, count=2, axis=0, sp=8, lo=0.0, hi=INF, fields=1, off=p, ws=p, ws_bytes=big):
        return h.rt_point_cloud_offsets_rolling(scene, table, poses_, count, axis, sp, lo, hi, None, fields, off, ws, ws_bytes, None, 0)

    assert offsets(scene=None) == -1 and offsets(table=None) == -1 and offsets(poses_=None) == -1 and offsets(off=None) == -1 and offsets(ws=None) == -1
    for count in (0, -1, 33):
        assert offsets(count=count) == -1
    for axis, sp in ((2, 8), (-1, 8), (0, 0), (0, 4), (1, 12), (1, -8)):
        assert offsets(axis=axis, sp=sp) == -1
    nan = float("nan")
    for lo, hi in ((nan, 1.0), (0.0, nan), (2.0, 1.0), (INF, 1.0)):
        assert offsets(lo=lo, hi=hi) == -1
    for fields in (0, 0x200, 0x201, 0xffffffff):
        assert offsets(fields=fields) == -1

    # the fill takes neither scene nor table: every refusal is judged on the host, capacity 0 launches nothing
    fill = h.rt_point_cloud_fill_rolling
    out, none = rt.RtPointCloud(range=p), rt.RtPointCloud()
    need = h.rt_point_cloud_rolling_workspace_bytes(16, 8, 2, 1, 2)
    assert need > 0 and fill(16, 8, 2, 0, 8, 1, p, need, 0, C.byref(out), None, 0) == 0
    assert fill(16, 8, 2, 0, 8, 1, p, need - 1, 0, C.byref(out), None, 0) == -1          # a workspace one byte short
    assert fill(16, 8, 2, 0, 8, 1, p, h.rt_point_cloud_workspace_bytes(16, 8, 2, 1), 0, C.byref(out), None, 0) == -1     # the static cloud's size: no room for the records
    for w, hh, n, axis, sp, f in ((0, 8, 2, 0, 8, 1), (16, 0, 2, 0, 8, 1), (16, 8, 0, 0, 8, 1), (16, 8, 33, 0, 8, 1), (16, 8, 2, 2, 8, 1), (16, 8, 2, 0, 4, 1),
                                  (16, 8, 2, 0, 12, 1), (16, 8, 2, 0, 8, 0), (16, 8, 2, 0, 8, 0x200)):
        assert fill(w, hh, n, axis, sp, f, p, big, 0, C.byref(out), None, 0) == -1, (w, hh, n, axis, sp, f)
    assert fill(16, 8, 2, 0, 8, 1, None, big, 0, C.byref(out), None, 0) == -1            # NULL workspace
    assert fill(16, 8, 2, 0, 8, 1, p, big, 0, None, None, 0) == -1                       # NULL out
    assert fill(16, 8, 2, 0, 8, EVERY, p, big, 0, C.byref(none), None, 0) == -1          # no output at all
    assert fill(16, 8, 2, 0, 8, 1, p, big, -1, C.byref(out), None, 0) == -1              # a negative capacity
    for k, bit in rt.RT_CLOUD_BITS.items():                                              # a pointer whose bit is not in fields
        assert fill(16, 8, 2, 0, 8, EVERY & ~bit, p, big, 0, C.byref(rt.RtPointCloud(**{k: p})), None, 0) == -1, k
        assert fill(16, 8, 2, 0, 8, bit, p, big, 0, C.byref(rt.RtPointCloud(**{k: p})), None, 0) == 0, k


class _Owner:
    """what the argument checks read of a Sensor: no table, no device"""
    width, height, h = 40, 24, None


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    staged = []
    monkeypatch.setattr(rt, "_staging", lambda *a, **k: staged.append(1))
    owner, sc = _Owner(), object()
    render = lambda **k: rt.Sensor.render_rolling(owner, sc, **k)        # noqa: E731
    cloud = lambda **k: rt.Sensor.rolling_point_cloud(owner, sc, **k)    # noqa: E731
    good = np.zeros((2, 3, 6), np.float32)                              # 40 columns in slices of 16: three
    for call in (render, cloud):
        for poses in (np.zeros((2, 6)), np.zeros((3, 6)), np.zeros((0, 3, 6)), np.zeros((2, 3, 5)), np.zeros((2, 2, 6)), np.zeros((2, 4, 6)), [], 1.0):
            with pytest.raises(ValueError):
                call(poses=poses, axis="x", slice_pixels=16)
        with pytest.raises(ValueError):
            call(poses=good, axis="y", slice_pixels=16)                 # (24 rows in slices of 16: two)
        for axis in ("z", 0, 1, None, "X"):
            with pytest.raises(ValueError):
                call(poses=good, axis=axis, slice_pixels=16)
        for sp in (0, 4, 12, -8, 8.5, True):
            with pytest.raises(ValueError):
                call(poses=np.zeros((2, 5, 6)), axis="x", slice_pixels=sp)
    for outs in (("range",), ("t", "t"), (), "depth", ("local", "offsets")):
        with pytest.raises(ValueError):
            render(poses=good, slice_pixels=16, outputs=outs)
    for outs in (("depth",), ("local", "local"), ()):
        with pytest.raises(ValueError):
            cloud(poses=good, slice_pixels=16, outputs=outs)
    for lo, hi in ((math.nan, 1.0), (2.0, 1.0)):
        with pytest.raises(ValueError):
            cloud(poses=good, slice_pixels=16, min_range=lo, max_range=hi)
    with pytest.raises(ValueError):
        cloud(poses=good, slice_pixels=16, mask=np.ones((40, 24), bool))
    assert not staged
    sig = inspect.signature(rt.Sensor.render_rolling)
    assert list(sig.parameters) == ["self", "scene", "poses", "axis", "slice_pixels", "outputs", "image", "stream", "as_numpy"]
    assert sig.parameters["axis"].default == "x" and sig.parameters["slice_pixels"].default == 8
    sig = inspect.signature(rt.Sensor.rolling_point_cloud)
    assert list(sig.parameters) == ["self", "scene", "poses", "axis", "slice_pixels", "outputs", "min_range", "max_range", "mask", "stream", "as_numpy"]
    assert rt.Sensor.render_rolling.__doc__ and rt.Sensor.rolling_point_cloud.__doc__


def test_rolling_poses_end_points_and_rounding(sensors):
    start = np.array([0.1, -0.2, 0.3, 0.4, -0.15, 0.0], np.float32)
    end = np.array([0.15, -0.24, 0.32, 0.7, -0.1, 0.1], np.float32)
    for n in (1, 2, 3, 16, 135, 256):
        P = sensors.rolling_poses(start, end, n)
        assert P.shape == (n, 6) and P.dtype == np.float32 and P.flags["C_CONTIGUOUS"]
        assert np.array_equal(P[0], start)                              # slice 0 fires at `start`, bit for bit
        a, b = start.astype(np.float64), end.astype(np.float64)
        want = np.stack([(a + (b - a) * s / n).astype(np.float32) for s in range(n)])    # float64, rounded once
        assert np.array_equal(P.view(np.uint32), want.view(np.uint32))
        assert not np.array_equal(P[-1], end) and np.all(np.abs(P[-1].astype(np.float64) - b) <= np.abs(b - a) / n + 1e-7)  # `end` is the next frame's start
        if n > 1:
            assert np.all(np.diff(P[:, 0]) > 0) and np.all(np.diff(P[:, 1]) < 0)
    # chained frames: the slice after the last of one frame is the first of the next
    mid = sensors.rolling_poses(end, start, 4)
    assert np.array_equal(mid[0], end)
    # a float32 interpolation would round twice: float64 inputs are honoured
    P = sensors.rolling_poses([1 / 3] * 6, [2 / 3] * 6, 3)
    assert np.array_equal(P[1], np.full(6, np.float32(1 / 3 + (1 / 3) / 3)))
    for bad in ((start[:5], end, 4), (start, end, 0), (start, end, -1), (start, end, 2.5), (np.zeros((2, 6)), end, 2)):
        with pytest.raises(ValueError):
            sensors.rolling_poses(*bad)
