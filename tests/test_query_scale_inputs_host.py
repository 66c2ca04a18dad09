"""The inputs of test_gpu_query_scale.py's region cases without a GPU: the builders there are plain functions, and every condition the
GPU tests rely on -- the wedges' counts in closed form, the bands of the last 64 regions' counts, how many of them fill a room from
instance 0 alone, the mix of inside flags and the sign changes of the normal along a list, the hit and miss shares of the two pools
and what the three-level scan asks of its counts -- is asserted here against the brute-force shim (tests/region_oracle.c) on the
oracle's scenes.  A GPU test that fails then fails on the library, not on its inputs."""
import numpy as np
import pytest

import query_points as qp
import region_oracle as ro
import scene_defs as sd
import test_gpu_query_scale as qs
from test_crossing_host import _cube

F32 = np.float32
K_FIXED = 2049


@pytest.fixture(scope="module")
def stacks(orc):
    """(the quad stack, the stack with half of its windings reversed) as oracle scenes"""
    so = [qs._stack_desc(orc.oracle(), flipped).build_oracle(orc) for flipped in (False, True)]
    yield so
    for s in so:
        s.close()


def _changes(a):
    return int((a[1:] != a[:-1]).sum())


def test_flipped_stack_keeps_the_geometry_and_reverses_half_of_the_normals(orc, stacks):
    o_ = orc.oracle()
    (plain, zs, none), (flipped, zs2, down) = qs._stack_tris(o_), qs._stack_tris(o_, flipped=True)
    assert np.array_equal(zs, zs2) and not none.any() and 500 <= down.sum() <= 700
    assert plain.shape == flipped.shape and len(plain) == 2 * qs.QUADS
    v0, v1 = plain[:, :9].reshape(-1, 3, 3), flipped[:, :9].reshape(-1, 3, 3)
    rev = np.repeat(down, 2)
    assert np.array_equal(v1[~rev], v0[~rev]) and np.array_equal(v1[rev], v0[rev][:, ::-1])     # the same vertices, reversed
    assert np.array_equal(zs, np.random.default_rng(3).permutation(1200).astype(F32) * F32(0.01))
    # the world normals as the list gives them, over the whole stack: one value on the plain stack, two opposite ones on the flipped
    whole = qs._wedge(0, 600, 1199)[None]
    lists = [ro.list_in_regions(so, whole) for so in stacks]
    for k in ("instance", "triangle", "inside", "offsets"):
        assert np.array_equal(lists[0][k], lists[1][k]), k
    n0, n1 = lists[0]["normal"], lists[1]["normal"]
    assert len(n0) == 4 * qs.QUADS and len(np.unique(n0, axis=0)) == 1 and (n0[:, :2] == 0).all() and n0[0, 2] > 0.99
    assert (n1[:, :2] == 0).all() and set(np.unique(n1[:, 2])) == {n0[0, 2], -n0[0, 2]}
    assert _changes(n0[:, 2]) == 0
    # 600 quads per instance in shuffled order, a random half reversed: about 300 sign changes per instance
    assert _changes(n1[:, 2] > 0) >= 400, _changes(n1[:, 2] > 0)


@pytest.mark.parametrize("spec,count,inside", [((100, 150, 399), 1200, 600), ((500, 50, 599), 400, 200), ((0, 10, 24), 100, 60),
                                               ((1175, 3, 1199), 100, 88), ((7, 1, 7), 4, 0), ((0, 600, 1199), 4800, 2400)])
def test_wedge_counts_in_closed_form(stacks, spec, count, inside):
    assert qs._wedge_counts(*spec) == (count, inside)
    for so in stacks:                                           # (the windings change no count)
        c = ro.count_in_regions(so, qs._wedge(*spec)[None])
        assert (int(c["count"][0]), int(c["inside"][0])) == (count, inside)


def test_csr_regions(stacks):
    regions, want_c, want_in, rng = qs._csr_regions()
    assert regions.shape == (400, 2, 2, 3) and regions.dtype == F32
    for so in stacks:
        c = ro.count_in_regions(so, regions)
        assert np.array_equal(c["count"], want_c) and np.array_equal(c["inside"], want_in)
    c = want_c.astype(np.int64)
    assert c.max() == 1200 and (c == 400).sum() == 2 and (c == 100).sum() == 4 and (c == 0).sum() == 150
    assert set(np.unique(c)) == {0, 4, 8, 12, 100, 400, 1200}
    assert (~np.isfinite(regions)).sum() == 0 and ((regions[:, :, 1] == 0).all(axis=2).any(axis=1)).sum() == 1      # one zero normal
    assert (regions[:, 0, 0] == 50).all(axis=1).sum() == 75                                                        # far off
    room = qs._csr_region_rooms(want_c, rng)
    assert (room < c).any() and (room > c).any() and (room == c).any() and (room == 0).any() and (room[c == 400] == 200).all()
    assert all((room[c == v] < v).any() and (room[c == v] > v).any() for v in (4, 8, 100))
    assert room.sum() + 5 + 64 <= 4096
    off = qs._cumsum(room)
    ref = ro.rooms(stacks[1], regions, offsets=off)
    assert np.array_equal(ref["count"], want_c)
    assert qs._mixed_flags(ref["inside"], c, room, off) == 7
    i = int(np.argmax(c))                                       # the list of 1200 entries: flags and normal signs alternate
    a, e = off[i], off[i] + min(room[i], c[i])
    assert e - a >= 1199
    flags, up = ref["inside"][a:e], ref["normal"][a:e, 2] > 0
    # 300 quads per instance in shuffled z: about 150 changes of either per instance (the two triangles of a quad agree)
    assert _changes(flags) >= 200 and _changes(up) >= 200, (_changes(flags), _changes(up))
    assert _changes(flags != up) >= 200                         # (and the two do not move together)
    plain = ro.rooms(stacks[0], regions, offsets=off)
    assert len(np.unique(plain["normal"][a:e], axis=0)) == 1 and np.array_equal(plain["inside"], ref["inside"])


def test_last_64_regions(stacks):
    last, want_c, want_in = qs._last64_regions()
    assert last.shape == (64, 2, 2, 3)
    for so in stacks:
        c = ro.count_in_regions(so, last)
        assert np.array_equal(c["count"], want_c) and np.array_equal(c["inside"], want_in)
    qs._last64_bands(want_c, K_FIXED)
    assert (want_c // 2 >= K_FIXED).sum() >= 17                 # these fill their room from instance 0 alone
    ref = ro.rooms(stacks[1], last, max_hits=K_FIXED)
    assert np.array_equal(ref["count"], want_c)
    full = np.flatnonzero(want_c // 2 >= K_FIXED)
    assert (ref["instance"].reshape(64, K_FIXED)[full] == 0).all()
    assert qs._mixed_flags(ref["inside"], want_c.astype(np.int64), np.full(64, K_FIXED), np.arange(64) * K_FIXED) == 49
    big = int(np.argmax(want_c))
    up = ref["normal"].reshape(64, K_FIXED, 3)[big, :, 2] > 0
    assert _changes(up) >= 400 and _changes(ref["inside"].reshape(64, K_FIXED)[big]) >= 400
    assert (ro.count_in_regions(stacks[1], np.tile(qs.FAR_REGION, (64, 1, 1, 1)))["count"] == 0).all()


def test_region_pool_on_the_multi_instance_scene(rt, orc, scenes, blob5k):
    desc = sd.multi_instance_scene(scenes, blob5k)
    so = desc.build_oracle(orc)
    try:
        lo, hi = (a.astype(np.float64) for a in qp.scene_box(orc.oracle(), desc, desc.oracle_meshes))
        regions = qs._region_pool(rt, lo, hi)
        assert regions.shape == (qs.POOL, 6, 2, 3) and regions.dtype == F32 and np.isfinite(regions).all()
        c = ro.count_in_regions(so, regions)["count"]
        assert (c > 0).sum() >= 16 and (c == 0).sum() >= 16 and c.max() > 64
        assert (c > 0).sum() > qs.POOL // 8 and (c == 0).sum() > qs.POOL // 8 and (c > 64).sum() >= 16
        for n in (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049):       # (what the block-edge test asks of every prefix)
            _q, cn = qs._prefix(((regions, None), c), n)
            last = (n - 1) // qs.SCAN_BLOCK * qs.SCAN_BLOCK
            assert cn[-1] > 0 and cn[last:].sum() > 0
    finally:
        so.close()


def test_cube_corners_for_the_three_level_scan(orc):
    desc = sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", _cube(orc))], [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    so = desc.build_oracle(orc)
    try:
        regions = qs._cube_corners()
        assert regions.shape == (qs.DISTINCT, 3, 2, 3) and len(np.unique(regions.reshape(qs.DISTINCT, -1), axis=0)) == qs.DISTINCT
        c0 = ro.count_in_regions(so, regions)["count"]
        assert (c0 > 0).sum() > qs.DISTINCT // 8 and (c0 == 0).sum() > qs.DISTINCT // 8
        B = qs.SCAN_BLOCK
        assert not any(np.array_equal(c0[:B], c0[k * B:(k + 1) * B]) for k in (1, 2, 3))
        n = 2 ** 20 + 1
        totals = qs._block_totals(np.resize(c0, n))
        assert len(np.unique(totals[:-1])) >= 2 and len(totals) > B
    finally:
        so.close()
