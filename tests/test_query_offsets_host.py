"""The workspace of the three *_offsets calls (rt_crossing_offsets / rt_nearby_offsets / rt_intersecting_offsets) without a GPU:
rt_*_offsets_workspace_bytes is pure host code shared by the three families, pinned here against a Python restatement of the
documented layout at the sizes where the scan gains a level, and each *_offsets call rejects a workspace one byte short before
it touches a device (the GPU side: test_gpu_query_scale.py)."""
import ctypes as C

import pytest

SCAN_BLOCK = 1024                                               # elements one scan block covers (kScanBlock)
ALIGN = 256
SIZES = [0, 1, 1023, 1024, 1025, 2 ** 20 - 2, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 30, 2 ** 31 - 1]
WS = ("rt_crossing_offsets_workspace_bytes", "rt_nearby_offsets_workspace_bytes", "rt_intersecting_offsets_workspace_bytes")


def _up(b):
    return -(-b // ALIGN) * ALIGN


def layout(n):
    """The documented layout -> (bytes, levels): the counts int32 [n] rounded up to 256 B, then per level of the scan over m = n + 1
    elements ceil(m / 1024) int64 block totals rounded up to 256 B, the next level scanning those totals, until a level has one
    block.  n <= 0: (0, 0)."""
    if n <= 0:
        return 0, 0
    total, m, levels = _up(4 * n), n + 1, 0
    while True:
        b = -(-m // SCAN_BLOCK)
        total += _up(8 * b)
        levels += 1
        if b == 1:
            return total, levels
        m = b


def levels_of(n, ws):
    """The number of levels a workspace of `ws` bytes holds for n queries: level sizes are taken off until nothing is left
    (-1 when they never come out even)"""
    left, m, levels = ws - _up(4 * n), n + 1, 0
    while left > 0:
        b = -(-m // SCAN_BLOCK)
        left -= _up(8 * b)
        levels += 1
        m = b
    return levels if left == 0 else -1


def _expected_levels(n):
    """m = n + 1 elements fit one block up to n = 1023, 1024 blocks (one block of totals) up to n = 2^20 - 1, 2^20 blocks up to
    n = 2^30 - 1; int32 n beyond that needs a fourth level"""
    return 0 if n <= 0 else 1 + sum(n >= SCAN_BLOCK ** k for k in (1, 2, 3))


def test_restatement_has_the_levels_the_arithmetic_says():
    for n in SIZES:
        assert layout(n)[1] == _expected_levels(n), n
    assert layout(1023) == (4096 + 256, 1)                      # m = 1024: one block
    assert layout(1024) == (4096 + 256 + 256, 2)                # m = 1025: two blocks, then one
    assert layout(2 ** 20 - 1) == (4 * 2 ** 20 + 8192 + 256, 2)           # m = 2^20: 1024 blocks, then one
    assert layout(2 ** 20) == (4 * 2 ** 20 + _up(8 * 1025) + 256 + 256, 3)       # m = 2^20 + 1: 1025 blocks, two, one
    assert [_expected_levels(n) for n in SIZES] == [0, 1, 1, 2, 2, 2, 2, 3, 3, 4, 4]


@pytest.mark.parametrize("n", SIZES)
def test_workspace_bytes_equal_the_documented_layout(rt, n):
    h = rt.libs()[0]
    got = [int(getattr(h, name)(n)) for name in WS]
    assert got[0] == got[1] == got[2], (n, got)
    want, levels = layout(n)
    assert got[0] == want, (n, got[0], want)
    assert levels_of(n, got[0]) == levels == _expected_levels(n), (n, got[0])


def test_workspace_bytes_of_no_queries_is_zero(rt):
    h = rt.libs()[0]
    for name in WS:
        for n in (0, -1, -1024, -2 ** 31):
            assert getattr(h, name)(n) == 0, (name, n)


@pytest.mark.parametrize("n", [1, 1000, 1023, 1024, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1])
def test_offsets_calls_reject_a_short_workspace_before_the_device(rt, n):
    """One byte short (and an empty workspace) is RT_E_INVALID from all three, at every level count; the scene and the buffers are
    bogus addresses, as in test_crossing_list_host.test_c_abi_exports_and_rejects_bad_arguments: a call that got past the check would
    not return."""
    h = rt.libs()[0]
    p, bogus = C.c_void_p(64), C.c_void_p(16)
    ws = layout(n)[0]
    for short in (ws - 1, ws - ALIGN, 0):
        assert h.rt_crossing_offsets(bogus, p, p, None, n, p, p, short, None, 0) == -1, (n, short)
        assert h.rt_nearby_offsets(bogus, p, None, n, p, p, short, None, 0) == -1, (n, short)
        assert h.rt_intersecting_offsets(bogus, p, None, n, p, p, short, None, 0) == -1, (n, short)
