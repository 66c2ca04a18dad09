"""The C-ABI of the region queries without a GPU: rt_region_offsets_workspace_bytes equals the layout the other *_offsets calls share
(test_query_offsets_host.py restates it), rt_region_offsets refuses a short workspace, and rt_count_in_regions / rt_region_offsets /
rt_list_in_regions return RT_E_INVALID for a NULL scene and for every bad argument -- a plane count of 0 or 9 among them -- before
they touch a device: the scene and the buffers are bogus addresses, so a call that got past its checks would not return."""
import ctypes as C

import numpy as np
import pytest

from test_query_offsets_host import ALIGN, SIZES, WS, layout


@pytest.mark.parametrize("n", SIZES)
def test_workspace_bytes_equal_the_shared_layout(rt, n):
    h = rt.libs()[0]
    got = int(h.rt_region_offsets_workspace_bytes(n))
    assert got == layout(n)[0], (n, got)
    assert all(got == int(getattr(h, name)(n)) for name in WS + ("rt_box_offsets_workspace_bytes", "rt_section_offsets_workspace_bytes")), n


def test_workspace_bytes_of_no_queries_is_zero(rt):
    h = rt.libs()[0]
    for n in (0, -1, -1024, -2 ** 31):
        assert h.rt_region_offsets_workspace_bytes(n) == 0, n


@pytest.mark.parametrize("n", [1, 1000, 1023, 1024, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1])
def test_region_offsets_rejects_a_short_workspace_before_the_device(rt, n):
    h = rt.libs()[0]
    p, bogus = C.c_void_p(64), C.c_void_p(16)
    ws = layout(n)[0]
    for short in (ws - 1, ws - ALIGN, 0):
        assert h.rt_region_offsets(bogus, p, n, 6, p, p, short, None, 0) == -1, (n, short)


def test_exports_and_rejects_bad_arguments(rt):
    h = rt.libs()[0]
    for name in ("rt_count_in_regions", "rt_region_offsets_workspace_bytes", "rt_region_offsets", "rt_list_in_regions"):
        assert hasattr(h, name) and name in rt.RT_HIP_SYMBOLS
    assert [f for f, _t in rt.RtRegionCounts._fields_] == ["count", "inside", "any", "pops"]
    assert [f for f, _t in rt.RtRegionList._fields_] == ["instance", "triangle", "inside", "normal", "count", "pops"]
    assert rt.REGION_MAX_PLANES == 8
    ws = h.rt_region_offsets_workspace_bytes(1000)
    p, bogus = C.c_void_p(64), C.c_void_p(16)
    cnt = rt.RtRegionCounts(count=p)
    assert h.rt_count_in_regions(None, p, 3, 6, C.byref(cnt), None, 0) == -1
    assert h.rt_count_in_regions(None, p, 0, 6, C.byref(cnt), None, 0) == -1                # a NULL scene even with n == 0
    assert h.rt_count_in_regions(bogus, p, -1, 6, C.byref(cnt), None, 0) == -1
    assert h.rt_count_in_regions(bogus, None, 3, 6, C.byref(cnt), None, 0) == -1
    assert h.rt_count_in_regions(bogus, p, 3, 6, None, None, 0) == -1
    assert h.rt_count_in_regions(bogus, p, 3, 6, C.byref(rt.RtRegionCounts()), None, 0) == -1   # no output at all
    for K in (0, 9, -1, 2 ** 31 - 1):                                                       # planes_per_region outside 1..8
        assert h.rt_count_in_regions(bogus, p, 3, K, C.byref(cnt), None, 0) == -1, K
        assert h.rt_count_in_regions(bogus, None, 0, K, None, None, 0) == -1, K             # even with n == 0
    for K in range(1, 9):
        assert h.rt_count_in_regions(bogus, None, 0, K, None, None, 0) == 0, K              # n == 0: nothing launched
    assert h.rt_region_offsets(None, p, 3, 6, p, p, ws, None, 0) == -1
    assert h.rt_region_offsets(bogus, p, -1, 6, p, p, ws, None, 0) == -1
    assert h.rt_region_offsets(bogus, None, 3, 6, p, p, ws, None, 0) == -1
    assert h.rt_region_offsets(bogus, p, 3, 6, None, p, ws, None, 0) == -1
    assert h.rt_region_offsets(bogus, p, 3, 6, p, None, ws, None, 0) == -1                  # no workspace
    assert h.rt_region_offsets(bogus, p, 1000, 6, p, p, ws - 1, None, 0) == -1              # workspace too small
    assert h.rt_region_offsets(bogus, p, 3, 0, p, p, ws, None, 0) == -1                     # K = 0
    assert h.rt_region_offsets(bogus, p, 3, 9, p, p, ws, None, 0) == -1                     # K = 9
    assert h.rt_region_offsets(bogus, None, 0, 9, None, None, 0, None, 0) == -1
    assert h.rt_region_offsets(bogus, None, 0, 8, None, None, 0, None, 0) == 0              # n == 0: d_offsets not written
    keys = dict(instance=C.c_void_p(64), triangle=C.c_void_p(128))
    out = rt.RtRegionList(**keys)
    assert h.rt_list_in_regions(None, p, 3, 6, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_in_regions(bogus, p, -1, 6, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_in_regions(bogus, None, 3, 6, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_in_regions(bogus, p, 3, 6, None, 4, None, None, 0) == -1
    for missing in keys:                                                                    # every key field is required
        part = rt.RtRegionList(**{k: v for k, v in keys.items() if k != missing}, inside=p, normal=p, count=p, pops=p)
        assert h.rt_list_in_regions(bogus, p, 3, 6, None, 4, C.byref(part), None, 0) == -1, missing
    assert h.rt_list_in_regions(bogus, p, 3, 6, p, 4, C.byref(out), None, 0) == -1          # both room forms
    assert h.rt_list_in_regions(bogus, p, 3, 6, None, 0, C.byref(out), None, 0) == -1       # neither
    assert h.rt_list_in_regions(bogus, p, 0, 6, p, 2, C.byref(out), None, 0) == -1
    assert h.rt_list_in_regions(bogus, p, 3, 0, None, 4, C.byref(out), None, 0) == -1       # K = 0
    assert h.rt_list_in_regions(bogus, p, 3, 9, None, 4, C.byref(out), None, 0) == -1       # K = 9
    assert h.rt_list_in_regions(bogus, None, 0, 1, None, 2, None, None, 0) == 0             # n == 0


@pytest.fixture
def untouched(rt, monkeypatch):
    """A scene whose device handle must never be asked for: the Python wrappers reject bad arguments first"""
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    s = rt.Scene()
    yield s
    assert not touched
    s.close()


@pytest.mark.parametrize("shape", [(2, 3), (4, 0, 2, 3), (4, 9, 2, 3), (4, 6, 3, 2), (4, 6, 2, 4), (6,)])
def test_python_rejects_bad_region_shapes_before_any_device_call(untouched, shape):
    with pytest.raises(ValueError):
        untouched.count_in_regions(np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        untouched.list_in_regions(np.zeros(shape, np.float32), max_hits=4)


def test_python_rejects_bad_arguments_before_any_device_call(rt, untouched):
    s = untouched
    good = np.zeros((4, 6, 2, 3), np.float32)
    for bad in (good.astype(np.float64), good[:, :, :, ::-1], good.tolist()):
        with pytest.raises(ValueError):
            s.count_in_regions(bad)
        with pytest.raises(ValueError):
            s.list_in_regions(bad)
    for outputs in ((), ("segment",), ("count", "nope")):
        with pytest.raises(ValueError):
            s.count_in_regions(good, outputs=outputs)
    for outputs in ((), ("count",), ("instance", "instance"), ("instance", "segment")):
        with pytest.raises(ValueError):
            s.list_in_regions(good, outputs=outputs)
    for mh in (0, -1, 1.5, True, 2 ** 31):
        with pytest.raises(ValueError):
            s.list_in_regions(good, max_hits=mh)
    assert rt.Scene.REGION_COUNT_OUTPUTS == ("count", "inside", "any", "pops")
    assert rt.Scene.REGION_LIST_OUTPUTS == ("instance", "triangle", "inside", "normal")
