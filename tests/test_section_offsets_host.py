"""The C-ABI of the plane sections without a GPU: rt_section_offsets_workspace_bytes equals the layout the other *_offsets calls share
(test_query_offsets_host.py restates it), rt_section_offsets refuses a short workspace, and rt_count_sections / rt_section_offsets /
rt_list_sections return RT_E_INVALID for a NULL scene and for every bad argument before they touch a device: the scene and the buffers
are bogus addresses, so a call that got past its checks would not return."""
import ctypes as C

import pytest

from test_query_offsets_host import ALIGN, SIZES, WS, layout


@pytest.mark.parametrize("n", SIZES)
def test_workspace_bytes_equal_the_shared_layout(rt, n):
    h = rt.libs()[0]
    got = int(h.rt_section_offsets_workspace_bytes(n))
    assert got == layout(n)[0], (n, got)
    assert all(got == int(getattr(h, name)(n)) for name in WS + ("rt_box_offsets_workspace_bytes",)), n


def test_workspace_bytes_of_no_queries_is_zero(rt):
    h = rt.libs()[0]
    for n in (0, -1, -1024, -2 ** 31):
        assert h.rt_section_offsets_workspace_bytes(n) == 0, n


@pytest.mark.parametrize("n", [1, 1000, 1023, 1024, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1])
def test_section_offsets_rejects_a_short_workspace_before_the_device(rt, n):
    h = rt.libs()[0]
    p, bogus = C.c_void_p(64), C.c_void_p(16)
    ws = layout(n)[0]
    for short in (ws - 1, ws - ALIGN, 0):
        assert h.rt_section_offsets(bogus, p, n, p, p, short, None, 0) == -1, (n, short)


def test_exports_and_rejects_bad_arguments(rt):
    h = rt.libs()[0]
    for name in ("rt_count_sections", "rt_section_offsets_workspace_bytes", "rt_section_offsets", "rt_list_sections"):
        assert hasattr(h, name) and name in rt.RT_HIP_SYMBOLS
    assert [f for f, _t in rt.RtSectionCounts._fields_] == ["count", "any", "pops"]
    assert [f for f, _t in rt.RtSectionList._fields_] == ["instance", "triangle", "segment", "normal", "count", "pops"]
    ws = h.rt_section_offsets_workspace_bytes(1000)
    p, bogus = C.c_void_p(64), C.c_void_p(16)
    cnt = rt.RtSectionCounts(count=p)
    assert h.rt_count_sections(None, p, 3, C.byref(cnt), None, 0) == -1
    assert h.rt_count_sections(None, p, 0, C.byref(cnt), None, 0) == -1                    # a NULL scene even with n == 0
    assert h.rt_count_sections(bogus, p, -1, C.byref(cnt), None, 0) == -1
    assert h.rt_count_sections(bogus, None, 3, C.byref(cnt), None, 0) == -1
    assert h.rt_count_sections(bogus, p, 3, None, None, 0) == -1
    assert h.rt_count_sections(bogus, p, 3, C.byref(rt.RtSectionCounts()), None, 0) == -1  # no output at all
    assert h.rt_count_sections(bogus, None, 0, None, None, 0) == 0                          # n == 0: nothing launched
    assert h.rt_section_offsets(None, p, 3, p, p, ws, None, 0) == -1
    assert h.rt_section_offsets(bogus, p, -1, p, p, ws, None, 0) == -1
    assert h.rt_section_offsets(bogus, None, 3, p, p, ws, None, 0) == -1
    assert h.rt_section_offsets(bogus, p, 3, None, p, ws, None, 0) == -1
    assert h.rt_section_offsets(bogus, p, 3, p, None, ws, None, 0) == -1                    # no workspace
    assert h.rt_section_offsets(bogus, p, 1000, p, p, ws - 1, None, 0) == -1                # workspace too small
    assert h.rt_section_offsets(bogus, None, 0, None, None, 0, None, 0) == 0                # n == 0: d_offsets not written
    keys = dict(instance=C.c_void_p(64), triangle=C.c_void_p(128))
    out = rt.RtSectionList(**keys)
    assert h.rt_list_sections(None, p, 3, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_sections(bogus, p, -1, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_sections(bogus, None, 3, None, 4, C.byref(out), None, 0) == -1
    assert h.rt_list_sections(bogus, p, 3, None, 4, None, None, 0) == -1
    for missing in keys:                                                                    # every key field is required
        part = rt.RtSectionList(**{k: v for k, v in keys.items() if k != missing}, segment=p, normal=p, count=p, pops=p)
        assert h.rt_list_sections(bogus, p, 3, None, 4, C.byref(part), None, 0) == -1, missing
    assert h.rt_list_sections(bogus, p, 3, p, 4, C.byref(out), None, 0) == -1               # both room forms
    assert h.rt_list_sections(bogus, p, 3, None, 0, C.byref(out), None, 0) == -1            # neither
    assert h.rt_list_sections(bogus, p, 0, p, 2, C.byref(out), None, 0) == -1
    assert h.rt_list_sections(bogus, None, 0, None, 2, None, None, 0) == 0                  # n == 0
