"""Visibility masks without a device: every RT_E_INVALID case of rt_visibility that can be judged without a scene is refused before
anything is touched (the scene handle is never dereferenced), rth_scene_visibility refuses a scene that was not uploaded, the Python
wrappers raise their ValueErrors before any device call, and the oracle module (tests/visibility_oracle.py) gives the masks written
out below on a hand-made three-triangle scene: a pixel occluded by a front face, one seen through a back face, one facing but
occluded, one visible but not facing, a miss."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import scene_defs as sd
import visibility_oracle as vo


def test_the_struct_and_the_symbols_follow_the_header(rt):
    assert C.sizeof(rt.RtVisibility) == 16 and [f[0] for f in rt.RtVisibility._fields_] == ["visible", "facing"]
    header = open(os.path.join(rt.ROOT, "include", "rt_hip.h")).read()
    assert "typedef struct RtVisibility { int32_t *visible, *facing; } RtVisibility;" in header and "visibility masks" in header
    assert hasattr(rt.libs()[0], "rt_visibility") and "rt_visibility" in rt.RT_HIP_SYMBOLS and "int rt_visibility(" in header
    host = open(os.path.join(rt.ROOT, "include", "rt_host.h")).read()
    assert hasattr(rt.libs()[1], "rth_scene_visibility") and "rth_scene_visibility" in rt.RT_HOST_SYMBOLS and "rth_scene_visibility" in host
    assert rt.libs()[0].rt_abi_version() == 2                            # the call is additive
    assert rt.Scene.VISIBILITY_OUTPUTS == rt.Camera.VISIBILITY_OUTPUTS == rt.Sensor.VISIBILITY_OUTPUTS == ("visible", "facing")


def test_rt_visibility_rejects_bad_arguments(rt):
    """Every case with a scene handle and planes that are never dereferenced: each call has one bad argument."""
    f = rt.libs()[0].rt_visibility
    bogus, p = C.c_void_p(16), C.c_void_p(64)
    both, vis, fac, none = rt.RtVisibility(p, p), rt.RtVisibility(visible=p), rt.RtVisibility(facing=p), rt.RtVisibility()

    def call(scene=bogus, inst=p, loc=p, nrm=p, w=40, h=24, n=2, pts=p, K=4, bias=2.0 ** -10, out=both):
        return f(scene, inst, loc, nrm, w, h, n, pts, K, bias, C.byref(out) if out is not None else None, None, 0)

    assert call(scene=None) == -1 and call(inst=None) == -1 and call(loc=None) == -1 and call(pts=None) == -1 and call(out=None) == -1
    assert call(out=none) == -1                                          # both outputs NULL
    assert call(nrm=None, out=both) == -1 and call(nrm=None, out=fac) == -1     # facing wanted, no normal plane
    for w, h, n in ((0, 24, 2), (40, 0, 2), (40, 24, 0), (-1, 24, 2), (40, -8, 2), (40, 24, -1)):
        assert call(w=w, h=h, n=n) == -1, (w, h, n)
    for w, h, n in ((2 ** 16, 2 ** 15, 1), (2 ** 31 - 1, 2, 1), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 11, 2 ** 10, 2 ** 10), (46341, 46341, 1),
                    (3, 2 ** 30, 1), (1, 2 ** 30, 2)):
        assert w * h * n > 2 ** 31 - 1 and call(w=w, h=h, n=n) == -1, (w, h, n)
    for K in (0, -1, 33, 64, 2 ** 31 - 1):
        assert call(K=K) == -1, K
    for bias in (-2.0 ** -10, 1.0, 1.5, math.nan, math.inf, -math.inf, -0.5):
        assert call(bias=bias) == -1, bias
    assert vis.facing is None and call(nrm=None, out=none) == -1


def test_the_facade_refuses_a_scene_without_a_device_scene(rt):
    g = rt.libs()[1].rth_scene_visibility
    p = C.c_void_p(64)
    out = rt.RtVisibility(visible=p)
    s = rt.Scene()                                                       # never uploaded
    try:
        assert g(s.h, p, p, None, 40, 24, 1, p, 1, 0.0, C.byref(out), None, 0) == -1
        assert g(s.h, p, p, None, 40, 24, 1, p, 1, 0.0, None, None, 0) == -1
        assert g(None, p, p, None, 40, 24, 1, p, 1, 0.0, C.byref(out), None, 0) == -1
    finally:
        s.close()


class _Owner:
    """what the argument checks read of a Camera or a Sensor: no table, no device"""
    width, height, h = 40, 24, None


def test_python_wrappers_check_before_the_device(rt, monkeypatch):
    staged = []
    monkeypatch.setattr(rt, "_staging", lambda *a, **k: staged.append(1))
    inst, loc, nrm = np.zeros((2, 24, 40), np.int32), np.zeros((2, 24, 40, 3), np.float32), np.zeros((2, 24, 40, 3), np.float32)
    pts = np.zeros((4, 3), np.float32)
    scene = object()
    vis = lambda **k: rt.Scene.visibility(scene, **dict(dict(instance=inst, location=loc, points=pts), **k))       # noqa: E731
    # shapes and dtypes of the planes
    for bad in (dict(instance=inst.astype(np.int64)), dict(instance=inst[0]), dict(instance=inst[:, :, :39]), dict(instance=inst[:, ::2]),
                dict(location=loc.astype(np.float64)), dict(location=loc[..., :2]), dict(location=loc[0], instance=inst[0]),
                dict(location=np.zeros((0, 24, 40, 3), np.float32), instance=np.zeros((0, 24, 40), np.int32)),
                dict(instance=inst.tolist()), dict(instance=None), dict(location=None)):
        with pytest.raises(ValueError):
            vis(**bad)
    # facing needs a normal plane of the location's shape and type
    for bad in (dict(), dict(normal=nrm[0]), dict(normal=nrm.astype(np.float64)), dict(normal=nrm[..., 0]), dict(normal=nrm.tolist())):
        with pytest.raises(ValueError):
            vis(outputs=("visible", "facing"), **bad)
    calls = [vis,
             lambda **k: rt.Camera.render_visibility(_Owner(), scene, **dict(dict(points=pts, poses=np.zeros((2, 6))), **k)),    # noqa: E731
             lambda **k: rt.Sensor.render_visibility(_Owner(), scene, **dict(dict(points=pts, poses=np.zeros((2, 6))), **k))]   # noqa: E731
    for call in calls:
        for points in (np.zeros((0, 3)), np.zeros((33, 3)), np.zeros((4, 2)), np.zeros((3, 4, 3)), np.zeros((1, 2, 4, 3)), np.zeros(3), 1.0, None,
                       "abc", [[0, 0]]):
            with pytest.raises(ValueError):
                call(points=points)
        for bias in (-0.001, 1.0, 2.0, math.nan, math.inf, "0.1", None, True, np.float64(1.0) - 1e-9):     # (the last is 1.0f in float32)
            with pytest.raises(ValueError):
                call(bias=bias)
        for outs in ((), ("visible", "visible"), ("lit",), "visible", ("visible", "t"), ("facing", "facing")):
            with pytest.raises(ValueError):
                call(outputs=outs)
    for call in calls[1:]:
        for gb in (("range",), ("t", "t"), ("visible",)):
            with pytest.raises(ValueError):
                call(gbuffer=gb)
        for poses in (np.zeros((2, 5)), np.zeros((0, 6)), np.zeros(6)):
            with pytest.raises(ValueError):
                call(poses=poses)
        with pytest.raises(ValueError):
            call(points=np.zeros((3, 4, 3)), poses=np.zeros((2, 6)))    # per-frame points for another number of frames
    assert not staged
    sig = inspect.signature(rt.Scene.visibility)
    assert list(sig.parameters) == ["self", "instance", "location", "points", "normal", "bias", "outputs", "stream", "as_numpy"]
    assert sig.parameters["bias"].default == 2.0 ** -10 and sig.parameters["outputs"].default == ("visible",)
    for cls in (rt.Camera, rt.Sensor):
        sig = inspect.signature(cls.render_visibility)
        assert list(sig.parameters) == ["self", "scene", "points", "poses", "bias", "outputs", "gbuffer", "image", "stream", "as_numpy"]
        assert sig.parameters["bias"].default == 2.0 ** -10 and sig.parameters["gbuffer"].default == () and cls.render_visibility.__doc__
    assert rt.Scene.visibility.__doc__


# ---- the oracle's rule on a scene small enough to reason about --------------------------------------------------------------------
# A floor at z = 0 whose front looks up; above it, at z = 1, a triangle whose front looks up (towards the point above) and one
# whose front looks DOWN.  Point 0 is above the floor at (0, 0, 3), point 1 below it at (0, 0, -3).
#   pixel 0, X = (-2, 0, 0): the ray from point 0 crosses z = 1 at (-4/3, 0), inside the up-looking triangle: occluded, though the floor
#                            there FACES the point; from below the ray meets only the floor's own back: visible, not facing.
#   pixel 1, X = ( 2, 0, 0): the ray from point 0 crosses the down-looking triangle at (4/3, 0) from behind: seen through the back face.
#   pixel 2, X = ( 0, 3, 0): the ray crosses z = 1 at (0, 2), outside both.
#   pixel 3: a miss.
FLOOR = (-10, -10, 0, 10, -10, 0, 0, 10, 0)
UP = (-2.5, -1, 1, -0.5, -1, 1, -1.5, 1.5, 1)
DOWN = (0.5, -1, 1, 1.5, 1.5, 1, 2.5, -1, 1)
POINTS = ((0.0, 0.0, 3.0), (0.0, 0.0, -3.0))
VISIBLE = (0b10, 0b11, 0b11, 0)
FACING = (0b01, 0b01, 0b01, 0)


@pytest.fixture(scope="module")
def three(orc):
    o = orc.oracle()
    tris = np.stack([o.tri_from_vertices(np.asarray(t, np.float32)) for t in (FLOOR, UP, DOWN)])
    assert np.array_equal(tris[:, 9:12], np.float32([[0, 0, 1], [0, 0, 1], [0, 0, -1]]) * np.abs(tris[:, 11:12]))      # the fronts
    so = sd.SceneDesc([((0.5, 0.5, 0.5), None)], [("tris", tris)], [(0, 0, (0,) * 6, (1, 1, 1))]).build_oracle(orc)
    yield so
    so.close()


def _planes():
    inst = np.int32([0, 0, 0, -1]).reshape(1, 1, 4)
    loc = np.float32([(-2, 0, 0), (2, 0, 0), (0, 3, 0), (0, 0, 0)]).reshape(1, 1, 4, 3)
    nrm = np.float32([(0, 0, 1)] * 3 + [(0, 0, 0)]).reshape(1, 1, 4, 3)
    return inst, loc, nrm


def test_the_oracle_on_three_triangles(three):
    inst, loc, nrm = _planes()
    got = vo.masks(three, inst, loc, nrm, POINTS)
    assert got["visible"].dtype == np.int32 and got["visible"].shape == (1, 1, 4)
    assert got["visible"].ravel().tolist() == list(VISIBLE) and got["facing"].ravel().tolist() == list(FACING)
    lit = got["visible"] & got["facing"]
    assert lit.ravel().tolist() == [0, 1, 1, 0]                          # pixel 0 faces point 0 and is occluded from it
    # per-frame points: frame 1 swaps the two points, and so the bits
    two = vo.masks(three, np.concatenate([inst, inst]), np.concatenate([loc, loc]), np.concatenate([nrm, nrm]), [POINTS, POINTS[::-1]])
    assert two["visible"][1].ravel().tolist() == [0b01, 0b11, 0b11, 0] and two["facing"][1].ravel().tolist() == [0b10, 0b10, 0b10, 0]
    assert np.array_equal(two["visible"][0], got["visible"][0])
    # visible alone needs no normal plane; 32 points use the sign bit and the planes stay int32
    assert set(vo.masks(three, inst, loc, None, POINTS)) == {"visible"}
    wide = vo.masks(three, inst, loc, nrm, [POINTS[1]] * 31 + [POINTS[0]])
    assert wide["visible"].ravel().tolist() == [2 ** 31 - 1, -1, -1, 0] and wide["facing"].ravel().tolist() == [-2 ** 31] * 3 + [0]


def test_the_bias_is_relative_and_zero_lets_the_surface_shadow_itself(three):
    inst, loc, _nrm = _planes()
    L, v, tmax = vo.rays(loc, vo.points_of(POINTS, 1), 0.25)
    d = np.sqrt(np.float32(4 + 9))
    assert np.array_equal(L[0, 0, 0, 0], np.float32(POINTS[0])) and np.array_equal(v[0, 0, 0, 0], np.float32((-2, 0, -3)))
    assert tmax[0, 0, 0, 0] == np.float32(d * np.float32(0.75)) and tmax.shape == (1, 1, 4, 2)
    # a quarter short of the surface the ray has passed z = 1 (at two thirds of the way): the occluder still counts; at 0.5 it does not
    assert vo.masks(three, inst, loc, None, POINTS, bias=0.25)["visible"].ravel().tolist() == list(VISIBLE)
    assert vo.masks(three, inst, loc, None, POINTS, bias=0.5)["visible"].ravel().tolist() == [0b11, 0b11, 0b11, 0]
    # bias 0: the bound is the distance itself, and wherever the floor is accepted below it the pixel shadows itself; never from below
    zero = vo.masks(three, inst, loc, None, POINTS, bias=0.0)["visible"].ravel()
    assert all(int(z) & 0b10 for z in zero[:3]) and zero[3] == 0 and zero[0] == 0b10
