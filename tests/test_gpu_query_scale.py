"""What the query families share, at the sizes where it can go wrong (the arithmetic of each family is test_gpu_crossing_list.py's,
test_gpu_nearby.py's, test_gpu_tri_intersect.py's, test_gpu_boxes.py's, test_gpu_sections.py's and test_gpu_regions.py's business): the
CSR scan behind the six *_offsets calls (crossing, nearby, intersecting, box, section, region) at its block edges and on its three-level
path, totals and room positions past 2^31 and 2^32, the box list's heap rooms at slots past 2^31 and 2^32, the section list's heap
rooms where the slot times the width of a segment or a normal passes 2^32 and where the slot itself does, the region list's heap rooms
where the slot -- which is also the byte index of the one-byte inside flag -- passes 2^31 and 2^32 and where 3 * slot passes 2^32,
occupancy grids that need the grid kernel's second launch row and its limit of 2^24 cells on an axis, and every query kernel with a
partly filled last workgroup on the deep scene.  The C-ABI is called directly on torch buffers: the Python wrappers would allocate
`total` rows.

The region family adds: rt_region_offsets, the only *_offsets call with an extra argument (planes_per_region) and a dispatch over four
plane capacities in front of the scan, at K = 6 on the block edges and at K = 3 (the capacity-4 kernel with a plane unused) on the
three-level path; and rt_list_in_regions' rooms on a quad stack with half of its quads' windings reversed, so that the inside flag and
the sign of the normal both change from entry to entry along a list and a flag or a record slot that the heap leaves behind shows.

Every offsets check compares with np.concatenate([[0], np.cumsum(counts)]) of the CPU shims' counts (crossing_oracle, nearby_oracle,
tri_intersect_oracle, box_oracle, section_oracle, region_oracle), never with the library's own counts.  Every buffer a kernel may write
is allocated at its full size; the large cases read back small windows only.  Totals beyond 2^32 are not repeated for boxes: the scan
and its 64-bit sums are one piece of code for all six families, tested through rt_crossing_offsets below.  The builders of the region
inputs need no GPU: tests/test_query_scale_inputs_host.py holds them to the shim in every ordinary run."""
import ctypes as C

import numpy as np
import pytest

import box_oracle as bo
import crossing_list_oracle as xl
import crossing_oracle as xo
import nearby_oracle as nb
import point_oracle
import query_points as qp
import ray_oracle
import region_oracle as ro
import scene_defs as sd
import section_oracle as sc
import tri_intersect_oracle as ti
from test_crossing_host import _cube
from test_gpu_crossings import _eq, _product
from test_gpu_tri_intersect import families as tri_families

pytestmark = pytest.mark.gpu
F32 = np.float32
SCAN_BLOCK = 1024                                               # elements per block of the scan over n + 1 offsets (kScanBlock)
GUARD = 0x5A
GUARD64 = int.from_bytes(bytes([GUARD]) * 8, "little")
FAMILIES = ("crossing", "nearby", "intersecting", "box", "section", "region")


def _cumsum(counts):
    return np.concatenate([[0], np.cumsum(counts.astype(np.int64))])


def _block_totals(counts):
    """the totals of the scan's level-0 blocks: n + 1 elements (the last one 0) in blocks of SCAN_BLOCK"""
    c = np.append(counts.astype(np.int64), 0)
    c = np.concatenate([c, np.zeros((-len(c)) % SCAN_BLOCK, np.int64)])
    return c.reshape(-1, SCAN_BLOCK).sum(axis=1)


def _planes_of(family, q):
    """planes_per_region of a region pool, which carries its K in its shape [n, K, 2, 3]; None for every other family"""
    return int(q[0].shape[1]) if family == "region" else None


def _ws_bytes(h, family, n, planes_per_region=None):
    """rt_<family>_offsets_workspace_bytes(n); a region's workspace holds one count per region whatever its planes_per_region"""
    assert (planes_per_region is not None) == (family == "region")
    return int(getattr(h, "rt_%s_offsets_workspace_bytes" % family)(n))


def _call_offsets(h, family, handle, q, n, off, ws, ws_bytes, planes_per_region=None):
    """rt_<family>_offsets on device pointers, synchronous on the NULL stream; q: the family's two query arrays (the second may be
    None); planes_per_region: for the region family alone"""
    a, b = q[0].data_ptr(), None if q[1] is None else q[1].data_ptr()
    if family == "region":
        return h.rt_region_offsets(handle, a, n, planes_per_region, off, ws, ws_bytes, None, 1)
    if family == "crossing":
        return h.rt_crossing_offsets(handle, a, b, None, n, off, ws, ws_bytes, None, 1)
    if family == "nearby":
        return h.rt_nearby_offsets(handle, a, b, n, off, ws, ws_bytes, None, 1)
    if family == "box":
        return h.rt_box_offsets(handle, a, n, off, ws, ws_bytes, None, 1)
    if family == "section":
        return h.rt_section_offsets(handle, a, n, off, ws, ws_bytes, None, 1)
    return h.rt_intersecting_offsets(handle, a, b, n, off, ws, ws_bytes, None, 1)


def _up(arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


class _Offsets:
    """Guarded buffers for one n: offsets int64 [n + 1] with 8 guard words behind, the workspace with 256 guard bytes behind"""

    def __init__(self, h, family, n, planes_per_region=None):
        import torch
        self.h, self.family, self.n, self.planes = h, family, n, planes_per_region
        self.ws_bytes = _ws_bytes(h, family, n, planes_per_region)
        self.off = torch.full((n + 1 + 8,), GUARD64, dtype=torch.int64, device="cuda")
        self.ws = torch.full((self.ws_bytes + 256,), GUARD, dtype=torch.uint8, device="cuda")

    def run(self, handle, q, where):
        """one call -> the offsets [n + 1]; the guards behind the offsets and behind the workspace are checked"""
        import torch
        torch.cuda.synchronize()
        assert _planes_of(self.family, q) == self.planes
        rc = _call_offsets(self.h, self.family, handle, q, self.n, self.off.data_ptr(), self.ws.data_ptr(), self.ws_bytes, self.planes)
        assert rc == 0, (where, rc)
        got = self.off.cpu().numpy()
        assert (got[self.n + 1:] == GUARD64).all(), "%s: the words behind offsets[n] were written: %s" % (where, got[self.n + 1:])
        tail = self.ws[self.ws_bytes:].cpu().numpy()
        assert (tail == GUARD).all(), "%s: %d bytes behind the workspace were written" % (where, int((tail != GUARD).sum()))
        return got[:self.n + 1]


def _same_offsets(got, ref, where):
    bad = np.flatnonzero(got != ref)
    assert bad.size == 0, "%s: %d of %d offsets differ, first at %d (block %d): got %s want %s" % (
        where, bad.size, len(ref), bad[0], bad[0] // SCAN_BLOCK, got[bad[:3]], ref[bad[:3]])


# ---- scenes, uploaded once per module ----------------------------------------------------------------------------------------
class _Pair:
    def __init__(self, rt, orc, desc):
        self.desc = desc
        self.so = desc.build_oracle(orc)
        self.sp = _product(rt, desc)
        self.handle = self.sp.device_handle

    def close(self):
        self.sp.close()
        self.so.close()


@pytest.fixture(scope="module")
def multi(rt, orc, scenes, blob5k):
    p = _Pair(rt, orc, sd.multi_instance_scene(scenes, blob5k))
    yield p
    p.close()


@pytest.fixture(scope="module")
def cube(rt, orc):
    p = _Pair(rt, orc, sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", _cube(orc))], [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))]))
    yield p
    p.close()


@pytest.fixture(scope="module")
def deep(rt, orc):
    p = _Pair(rt, orc, sd.deep_stack_scene(28))
    yield p
    p.close()


def _stack_tris(o_, flipped=False):
    """test_gpu_crossing_list.test_thousand_crossings_sorted's 1200 parallel quads as 2400 triangle records in shuffled order: quad j of
    the list lies at z = zs[j].  flipped: a random half of the quads (drawn from a generator of its own: the order stays what it was)
    have both triangles' windings reversed, so their normals point down; the vertices, and with them every count, are unchanged.
    -> (records [2400, ...], zs [1200], down [1200] bool)"""
    rng = np.random.default_rng(3)
    zs = rng.permutation(1200).astype(F32) * F32(0.01)
    down = np.random.default_rng(109).random(1200) < 0.5 if flipped else np.zeros(1200, bool)
    tris = []
    for z, rev in zip(zs, down):
        for f in ((0, 1, 2), (0, 2, 3)):
            v = np.array([(0, 0, z), (1, 0, z), (1, 1, z), (0, 1, z)], F32)[list(f[::-1] if rev else f)]
            tris.append(np.asarray(o_.tri_from_vertices(v.ravel()), F32))
    return np.stack(tris), zs, down


def _stack_desc(o_, flipped=False):
    """the quads as two coincident instances"""
    inst = (0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))
    return sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", _stack_tris(o_, flipped)[0])], [inst, inst])


@pytest.fixture(scope="module")
def stack(rt, orc):
    """test_gpu_crossing_list.test_thousand_crossings_sorted's 1200 parallel quads (2400 triangles, in shuffled order), as two
    coincident instances: a ray along z crosses one triangle of every quad of both, about 2400 crossings"""
    p = _Pair(rt, orc, _stack_desc(orc.oracle()))
    yield p
    p.close()


@pytest.fixture(scope="module")
def flipstack(rt, orc):
    """the same stack with the winding of a random half of its quads reversed: the world normals are (0, 0, +-c) and the sign changes
    about 300 times along a list of 1200 entries, so an entry that ends up with another entry's record slot shows in `normal`"""
    p = _Pair(rt, orc, _stack_desc(orc.oracle(), flipped=True))
    yield p
    p.close()


# ---- B1: the scan's block edges ------------------------------------------------------------------------------------------------
POOL = 2049


def _obb_regions(rt, rng, centres, size):
    """K = 6 oriented boxes: random frames, edges of 0.4 to 1 times `size`"""
    m = len(centres)
    q = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(m)])
    half = 0.5 * size[:, None] * rng.uniform(0.4, 1.0, (m, 3))
    return rt.regions_from_obbs(np.ascontiguousarray(centres, F32), np.ascontiguousarray(q, F32), np.ascontiguousarray(half, F32))


def _region_pool(rt, lo, hi):
    """POOL K = 6 regions for a scene whose box is lo..hi: oriented boxes of 1e-3 to 0.6 of the diagonal in and around the box (the
    large ones hold hundreds of pairs, most small ones none), a fifth of them far outside -> [POOL, 6, 2, 3] float32"""
    rng = np.random.default_rng(107)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    span, diag = np.maximum(hi - lo, 1e-3), float(np.linalg.norm(hi - lo))
    c = lo + span * rng.uniform(-0.1, 1.1, (POOL, 3))
    size = diag * 10.0 ** rng.uniform(-3, np.log10(0.6), POOL)
    u = rng.normal(size=(POOL, 3))
    far = rng.random(POOL) < 0.2
    c[far] = ((lo + hi) / 2 + u / np.linalg.norm(u, axis=1, keepdims=True) * diag * rng.uniform(1.5, 4, (POOL, 1)))[far]
    return np.ascontiguousarray(_obb_regions(rt, rng, c, size), F32)


@pytest.fixture(scope="module")
def pools(rt, orc, multi):
    """Per family: POOL queries on the multi-instance scene (hits and misses mixed) with the shim's counts, computed once, and the
    indices of the queries with a count above 0"""
    rng = np.random.default_rng(41)
    o = rng.uniform(-1.5, 1.5, (POOL, 3)).astype(F32)
    d = rng.normal(size=(POOL, 3)).astype(F32)
    pts = rng.uniform(-1.5, 1.5, (POOL, 3)).astype(F32)
    md = rng.uniform(0.02, 0.3, POOL).astype(F32)
    tris = np.concatenate([f[1] for f in tri_families(rng, orc.oracle(), multi.desc, n=400)])
    tris = np.ascontiguousarray(tris[rng.permutation(len(tris))[:POOL]], F32)
    assert len(tris) == POOL
    bc, be = rng.uniform(-1.5, 1.5, (POOL, 3)), rng.uniform(0.02, 0.3, (POOL, 3))
    boxes = np.ascontiguousarray(np.stack([bc - be / 2, bc + be / 2], axis=1), F32)
    # planes: a generator of their own (the draws above stay what they were); about a quarter lie outside the scene.  Counts run
    # to several hundred, so a count launch that stops at the first pair (every count capped at 1) changes most offsets
    rng = np.random.default_rng(41)
    pp, u = rng.uniform(-1.5, 1.5, (POOL, 3)), rng.normal(size=(POOL, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    lo, hi = (a.astype(np.float64) for a in qp.scene_box(orc.oracle(), multi.desc, multi.desc.oracle_meshes))
    far = rng.random(POOL) < 0.25
    pp[far] = (lo + hi) / 2 + u[far] * np.linalg.norm(hi - lo) * rng.uniform(1.5, 4, (int(far.sum()), 1))
    planes = np.ascontiguousarray(np.stack([pp, u], axis=1), F32)
    out = {"crossing": ((o, d), xo.count_crossings(multi.so, o, d)["count"]),
           "nearby": ((pts, md), nb.count_nearby(multi.so, pts, md)),
           "intersecting": ((tris, None), ti.count_intersecting(multi.so, tris)),
           "box": ((boxes, None), bo.count_in_boxes(multi.so, boxes)),
           "section": ((planes, None), sc.count_sections(multi.so, planes))}
    regions = _region_pool(rt, lo, hi)
    out["region"] = ((regions, None), ro.count_in_regions(multi.so, regions)["count"])
    assert out["section"][1].max() > 64, out["section"][1].max()
    assert out["region"][1].max() > 64 and regions.shape == (POOL, 6, 2, 3), out["region"][1].max()
    for family, (_q, c) in out.items():
        assert (c > 0).sum() >= 16 and (c == 0).sum() >= 16, (family, int((c > 0).sum()))
    return out


def _prefix(pool, n):
    """The first n queries of a pool with the last min(n, 3) replaced by queries whose count is above 0 -> (queries, counts).  The
    last counted element of the scan, and with it the last block that holds counts, is then never empty."""
    q, c = pool
    idx = np.arange(n)
    hits = np.flatnonzero(c > 0)
    k = min(n, 3)
    idx[n - k:] = hits[-k:]
    return tuple(None if a is None else np.ascontiguousarray(a[idx]) for a in q), c[idx]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049])
@pytest.mark.parametrize("family", FAMILIES)
def test_offsets_at_scan_block_edges(rt, multi, pools, family, n):
    """d_offsets[0..n] is the cumulative sum of the shim's counts with n + 1 below, at and above one and two scan blocks (and the
    query kernels' workgroup of 64); nothing behind offsets[n] or behind the workspace is written; a second call with the queries
    in reverse order into the SAME buffers, not cleared, gives that order's cumulative sum (no dependence on prior contents)."""
    h = rt.libs()[0]
    q, counts = _prefix(pools[family], n)
    ref = _cumsum(counts)
    last = (n - 1) // SCAN_BLOCK * SCAN_BLOCK                  # the last scan block that holds a count
    assert counts[-1] > 0 and counts[last:].sum() > 0 and ref[-1] > ref[last]
    buf = _Offsets(h, family, n, _planes_of(family, q))
    got = buf.run(multi.handle, _up(q), "%s n=%d" % (family, n))
    _same_offsets(got, ref, "%s n=%d" % (family, n))
    rq = tuple(None if a is None else a[::-1].copy() for a in q)
    got = buf.run(multi.handle, _up(rq), "%s n=%d again" % (family, n))
    _same_offsets(got, _cumsum(counts[::-1]), "%s n=%d, buffers reused" % (family, n))


# ---- B2: the three-level scan --------------------------------------------------------------------------------------------------
DISTINCT = 4096


def _cube_corners():
    """DISTINCT distinct K = 3 regions around the unit cube: the corner of three random half-spaces through one point in or near the
    cube -> [DISTINCT, 3, 2, 3] float32.  K = 3 runs the capacity-4 kernels with one plane unused."""
    rng = np.random.default_rng(113)
    p = rng.uniform(-0.5, 1.5, (DISTINCT, 1, 3))
    u = rng.normal(size=(DISTINCT, 3, 3))
    return np.ascontiguousarray(np.stack([np.broadcast_to(p, u.shape), u / np.linalg.norm(u, axis=2, keepdims=True)], axis=2), F32)


@pytest.fixture(scope="module")
def cube_queries(cube):
    """DISTINCT distinct queries per family around the unit cube, hits and misses mixed without a period, and the shim's counts"""
    rng = np.random.default_rng(43)
    u = rng.normal(size=(DISTINCT, 3))
    o = (0.5 + 3.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(F32)
    aim = rng.uniform(-0.6, 1.6, (DISTINCT, 3))
    d = (aim - o).astype(F32)
    pts = rng.uniform(-0.5, 1.5, (DISTINCT, 3)).astype(F32)
    md = rng.uniform(0.05, 0.5, DISTINCT).astype(F32)
    cen = rng.uniform(-0.3, 1.3, (DISTINCT, 1, 3))
    tris = np.ascontiguousarray(cen + rng.normal(size=(DISTINCT, 3, 3)) * 0.15, F32)
    bc, be = rng.uniform(-0.5, 1.5, (DISTINCT, 3)), rng.uniform(0.05, 0.5, (DISTINCT, 3))
    boxes = np.ascontiguousarray(np.stack([bc - be / 2, bc + be / 2], axis=1), F32)
    rng = np.random.default_rng(43)                             # (planes: a generator of their own, as in pools)
    pp, u = rng.uniform(-0.5, 1.5, (DISTINCT, 3)), rng.normal(size=(DISTINCT, 3))
    planes = np.ascontiguousarray(np.stack([pp, u / np.linalg.norm(u, axis=1, keepdims=True)], axis=1), F32)
    return {"crossing": ((o, d), xo.count_crossings(cube.so, o, d)["count"]),
            "nearby": ((pts, md), nb.count_nearby(cube.so, pts, md)),
            "intersecting": ((tris, None), ti.count_intersecting(cube.so, tris)),
            "box": ((boxes, None), bo.count_in_boxes(cube.so, boxes)),
            "section": ((planes, None), sc.count_sections(cube.so, planes)),
            "region": ((_cube_corners(), None), ro.count_in_regions(cube.so, _cube_corners())["count"])}


def _tiled(pool, n):
    q, c = pool
    return tuple(None if a is None else np.resize(a, (n,) + a.shape[1:]) for a in q), np.resize(c, n)


def _three_levels(rt, cube, cube_queries, family, n):
    h = rt.libs()[0]
    q, counts = _tiled(cube_queries[family], n)
    c0 = cube_queries[family][1]
    assert n + 1 > SCAN_BLOCK ** 2                              # three levels: more than 1024 level-0 blocks
    assert (c0 > 0).sum() > DISTINCT // 8 and (c0 == 0).sum() > DISTINCT // 8, family
    assert not any(np.array_equal(c0[:SCAN_BLOCK], c0[k * SCAN_BLOCK:(k + 1) * SCAN_BLOCK]) for k in (1, 2, 3)), "period 1024"
    totals = _block_totals(counts)
    assert len(np.unique(totals[:-1])) >= 2 and len(totals) > SCAN_BLOCK, (family, np.unique(totals))
    ref = _cumsum(counts)
    got = _Offsets(h, family, n, _planes_of(family, q)).run(cube.handle, _up(q), "%s n=%d" % (family, n))
    _same_offsets(got, ref, "%s n=%d" % (family, n))


@pytest.mark.parametrize("n", [2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 1025])
def test_three_level_scan_crossing(rt, cube, cube_queries, n):
    """rt_crossing_offsets just below the three-level threshold (n + 1 = 2^20: the widest two-level scan), at 1025 level-0 blocks,
    at 1025 blocks plus one element and at 1026 blocks plus an element: the whole offsets array equals the cumulative sum of the
    shim's counts of 4096 distinct rays, tiled.  The level-0 block totals differ from block to block, so totals added to the wrong
    block, or into the wrong level's array, change offsets."""
    if n + 1 > SCAN_BLOCK ** 2:
        _three_levels(rt, cube, cube_queries, "crossing", n)
        return
    h = rt.libs()[0]
    q, counts = _tiled(cube_queries["crossing"], n)
    assert len(_block_totals(counts)) == SCAN_BLOCK
    got = _Offsets(h, "crossing", n).run(cube.handle, _up(q), "crossing n=%d" % n)
    _same_offsets(got, _cumsum(counts), "crossing n=%d" % n)


@pytest.mark.parametrize("family", ["nearby", "intersecting", "box", "section", "region"])
def test_three_level_scan_other_families(rt, cube, cube_queries, family):
    """The same at n = 2^20 + 1 through rt_nearby_offsets, rt_intersecting_offsets, rt_box_offsets, rt_section_offsets and
    rt_region_offsets: one scan, but each family's own count launch (the regions' with K = 3 planes, one below its kernel's capacity)"""
    _three_levels(rt, cube, cube_queries, family, 2 ** 20 + 1)


# ---- B3: totals beyond 2^31 and 2^32 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lo,hi", [(2 ** 20 + 1, 2 ** 31, 2 ** 32), (1850000, 2 ** 32, 2 ** 33)])
def test_totals_beyond_32_bits(rt, stack, n, lo, hi):
    """rt_crossing_offsets on the quad stack, 64 distinct rays of about 2400 crossings each, tiled: with n = 2^20 + 1 the total lies
    between 2^31 and 2^32 (a signed 32-bit intermediate anywhere in the scan shows), with n = 1.85 M above 2^32 (an unsigned one
    shows).  All offsets are compared.  The stack is instanced twice because one instance gives 1200 crossings per ray, and the
    total at n = 2^20 + 1 would stay below 2^31.  The count kernel does the work of `total` crossings, 2.5 and 4.4 G here; on an
    MI355X each case takes 0.06 s, upload and read-back of the offsets included, so both stay in the suite as they are."""
    h = rt.libs()[0]
    rng = np.random.default_rng(3)
    o = np.concatenate([rng.uniform(0.2, 0.8, (64, 2)), np.full((64, 1), -1.0)], axis=1).astype(F32)
    d = np.concatenate([rng.uniform(-0.01, 0.01, (64, 2)), np.ones((64, 1))], axis=1).astype(F32)
    c64 = xo.count_crossings(stack.so, o, d)["count"]
    assert (c64 >= 2400).all() and (c64 <= 2 * 2400).all(), c64
    counts = np.resize(c64, n)
    ref = _cumsum(counts)
    assert lo < ref[-1] < hi, (int(ref[-1]), lo, hi)
    got = _Offsets(h, "crossing", n).run(stack.handle, _up((np.resize(o, (n, 3)), np.resize(d, (n, 3)))), "quad stack n=%d" % n)
    _same_offsets(got, ref, "quad stack n=%d (total %d)" % (n, ref[-1]))


# ---- B4: room positions beyond 2^31 and 2^32 in the list kernel -----------------------------------------------------------------
def _need_memory(nbytes):
    import torch
    free, total = torch.cuda.mem_get_info()
    if free < 2 * nbytes:
        pytest.skip("needs %d bytes of device memory twice over, %d of %d free" % (nbytes, free, total))


def _list_sign_only(rt, handle, q, n, offsets_ptr, max_hits, sign_ptr):
    """rt_list_crossings with the sign field alone (no key field: the selection path), synchronous on the NULL stream"""
    import torch
    lst = rt.RtCrossingList(sign=sign_ptr)
    torch.cuda.synchronize()
    return rt.libs()[0].rt_list_crossings(handle, q[0].data_ptr(), q[1].data_ptr(), None, n, offsets_ptr, max_hits, C.byref(lst), None, 1)


@pytest.mark.parametrize("base", [2 ** 31 + 5, 2 ** 32 + 5])
def test_csr_rooms_beyond_32_bits(rt, cube, cube_queries, base):
    """400 rays on the cube with hand-made offsets base + cumsum(room), rooms below, at and above each count: the int8 sign rooms land
    at byte `base` and beyond of a buffer that large and equal the shim's; the guard bytes 64 either side of them and in the first
    4096 bytes of the buffer (where a start cut to 32 bits would land) are untouched.  Only those windows are ever written by the
    test or read back."""
    import torch
    rng = np.random.default_rng(47)
    (o, d), c = cube_queries["crossing"]
    o, d, c = o[:400], d[:400], c[:400].astype(np.int64)
    room = np.maximum(c + rng.integers(-1, 3, 400), 0)
    assert (room < c).any() and (room > c).any() and (room == 0).any() and (c > 0).sum() > 50
    rooms = int(room.sum())
    assert rooms + 5 + 64 <= 4096                               # (offsets mod 2^32 fall inside the head window)
    offsets = (base + _cumsum(room)).astype(np.int64)
    nbytes = base + rooms + 64
    _need_memory(nbytes)
    lo, hi = base - 64, base + rooms + 64
    ref = xl.rooms(cube.so, o, d, offsets=offsets - lo, slots=hi - lo, fill=dict(sign=GUARD))
    buf = None
    try:
        buf = torch.empty(nbytes, dtype=torch.int8, device="cuda")
        buf[lo:hi].fill_(GUARD)
        buf[:4096].fill_(GUARD)
        q = _up((o, d))
        doff = torch.from_numpy(offsets).cuda()
        assert _list_sign_only(rt, cube.handle, q, 400, doff.data_ptr(), 0, buf.data_ptr()) == 0
        window, head = buf[lo:hi].cpu().numpy(), buf[:4096].cpu().numpy()
        assert (head == GUARD).all(), "%d of the buffer's first 4096 bytes were written" % int((head != GUARD).sum())
        _eq(window, ref["sign"], "sign rooms at byte %d" % base)
        assert set(np.unique(window[64:64 + rooms])) == {-1, 0, 1}
    finally:
        del buf
        torch.cuda.empty_cache()


def test_fixed_rooms_beyond_31_bits(rt, cube):
    """max_hits = 2049 and n = 2^20 + 64: the int8 sign rooms of the last 64 rays, the only ones that hit the cube, start beyond byte
    2^31 and equal the shim's fixed rooms; the rooms of a sample of the other rays (the first, the last, and those around byte 2^31)
    are all padding."""
    import torch
    K, n = 2049, 2 ** 20 + 64
    rng = np.random.default_rng(53)
    o = np.full((n, 3), 50.0, F32)                              # far off, pointing away: no crossing
    d = np.tile(np.array([[1.0, 0.5, 0.25]], F32), (n, 1))
    o[-64:] = np.concatenate([np.full((64, 1), -1.0), rng.uniform(0.1, 0.9, (64, 2))], axis=1).astype(F32)
    d[-64:] = np.concatenate([np.ones((64, 1)), rng.uniform(-0.05, 0.05, (64, 2))], axis=1).astype(F32)
    ref = xl.rooms(cube.so, o[-64:], d[-64:], max_hits=K)
    assert (ref["count"] == 2).all() and (n - 64) * K > 2 ** 31
    assert (xo.count_crossings(cube.so, o[:64], d[:64])["count"] == 0).all()
    nbytes = n * K
    _need_memory(nbytes)
    buf = None
    try:
        buf = torch.empty(nbytes, dtype=torch.int8, device="cuda")
        sample = sorted({0, 1, 63, 64, 2 ** 19, 2 ** 31 // K - 1, 2 ** 31 // K, 2 ** 31 // K + 1, n - 66, n - 65})
        for i in sample:
            buf[i * K:(i + 1) * K].fill_(GUARD)
        buf[(n - 64) * K:].fill_(GUARD)
        assert _list_sign_only(rt, cube.handle, _up((o, d)), n, None, K, buf.data_ptr()) == 0
        last = buf[(n - 64) * K:].cpu().numpy()
        _eq(last, ref["sign"], "the last 64 rooms")
        assert (np.abs(last.reshape(64, K)[:, :2]) == 1).all()
        for i in sample:
            room = buf[i * K:(i + 1) * K].cpu().numpy()
            assert (room == 0).all(), "room %d (a ray without crossings): %d bytes are not padding" % (i, int((room != 0).sum()))
    finally:
        del buf
        torch.cuda.empty_cache()


# ---- B4b: the box list's heap rooms at slots beyond 2^31 and 2^32 ----------------------------------------------------------------
GUARD32 = int(np.frombuffer(bytes([GUARD]) * 4, np.int32)[0])
QUADS = 1200                                                    # the stack scene: quad k at z = float32(k) * float32(0.01), twice


def _slab(a, b):
    """the box over the whole footprint of the stack's quads a..b: 2 triangles of 2 instances each, 4 * (b - a + 1) pairs"""
    return np.array([[-0.5, -0.5, a * 0.01 - 0.005], [1.5, 1.5, b * 0.01 + 0.005]], F32)


def _thin(rng, m):
    """m small boxes 0.004 thick in z somewhere in and around the stack: most hold one quad's triangles or none"""
    c = np.concatenate([rng.uniform(0.1, 0.9, (m, 2)), rng.uniform(-0.5, 12.5, (m, 1))], axis=1)
    e = np.concatenate([rng.uniform(0.02, 0.3, (m, 2)), np.full((m, 1), 0.004)], axis=1)
    return np.stack([c - e / 2, c + e / 2], axis=1).astype(F32)


FAR_BOX = np.array([[50, 50, 50], [51, 51, 51]], F32)


def _box_list(rt, handle, boxes, n, offsets_ptr, max_hits, inst, tri, cnt):
    """rt_list_in_boxes on device buffers, synchronous on the NULL stream"""
    import torch
    lst = rt.RtBoxList(inst.data_ptr(), tri.data_ptr(), None if cnt is None else cnt.data_ptr(), None)
    torch.cuda.synchronize()
    return rt.libs()[0].rt_list_in_boxes(handle, boxes.data_ptr(), n, offsets_ptr, max_hits, C.byref(lst), None, 1)


def _csr_boxes():
    """400 boxes on the quad stack, shuffled: one of 1200 pairs, two of 400, four of 100, 150 far off and 243 thin ones -> (boxes,
    rooms below, at and above each count, two of the large ones at half their count, some of 0)"""
    rng = np.random.default_rng(67)
    big = [_slab(100, 399), _slab(500, 599), _slab(700, 799)] + [_slab(a, a + 24) for a in (0, 450, 900, 1175)]
    boxes = np.concatenate([np.stack(big), np.tile(FAR_BOX, (150, 1, 1)), _thin(rng, 243)])
    boxes = np.ascontiguousarray(boxes[rng.permutation(len(boxes))])
    return boxes, rng


@pytest.mark.parametrize("base", [2 ** 31 + 5, 2 ** 32 + 5])
def test_box_csr_rooms_beyond_32_bits(rt, stack, base):
    """test_csr_rooms_beyond_32_bits for rt_list_in_boxes, whose rooms are max-heaps with 64-bit slot arithmetic of their own (BxRoom's
    get and put, room_insert, room_sift_down, room_sort): 400 boxes on the quad stack with hand-made offsets base + cumsum(room), counted in
    int32 slots, rooms below, at and above each count (two deep heaps at half their count, so most arrivals replace the root).  The
    lists run to 1200 keys.  Both key arrays' windows around the rooms equal the shim's rooms, guard words 64 either side included,
    and the first 4096 slots of each array (where a start cut to 32 bits would land) keep their guards.  count equals the shim's."""
    import torch
    boxes, rng = _csr_boxes()
    n = len(boxes)
    c = bo.count_in_boxes(stack.so, boxes).astype(np.int64)
    assert c.max() == 1200 and (c >= 400).sum() == 3 and (c >= 100).sum() == 7 and (c == 0).sum() > 150 and ((c > 0) & (c <= 4)).sum() > 50
    room = np.maximum(c + rng.integers(-1, 3, n), 0)
    half = np.flatnonzero(c == 400)
    room[half] = c[half] // 2
    assert (room < c).any() and (room > c).any() and (room == c).any() and (room == 0).any()
    rooms = int(room.sum())
    assert rooms + 5 + 64 <= 4096                               # (offsets mod 2^32 fall inside the head window)
    offsets = (base + _cumsum(room)).astype(np.int64)
    nslots = base + rooms + 64
    _need_memory(2 * 4 * nslots)
    lo, hi = base - 64, base + rooms + 64
    ref = bo.rooms(stack.so, boxes, offsets=offsets - lo, slots=hi - lo, fill=GUARD32)
    bufs = None
    try:
        bufs = {k: torch.empty(nslots, dtype=torch.int32, device="cuda") for k in bo.FIELDS}
        for b in bufs.values():
            b[lo:hi].fill_(GUARD32)
            b[:4096].fill_(GUARD32)
        cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        doff = torch.from_numpy(offsets).cuda()
        bt, = _up((boxes,))
        assert _box_list(rt, stack.handle, bt, n, doff.data_ptr(), 0, bufs["instance"], bufs["triangle"], cnt) == 0
        for k in bo.FIELDS:
            window, head = bufs[k][lo:hi].cpu().numpy(), bufs[k][:4096].cpu().numpy()
            assert (head == GUARD32).all(), "%s: %d of the array's first 4096 slots were written" % (k, int((head != GUARD32).sum()))
            _eq(window, ref[k], "%s rooms at slot %d" % (k, base))
        _eq(cnt.cpu().numpy(), ref["count"], "count")
    finally:
        del bufs
        torch.cuda.empty_cache()


def test_box_fixed_rooms_beyond_31_bits(rt, stack):
    """max_hits = 2049 and n = 2^20 + 64 on the quad stack: the rooms of the last 64 boxes, the only ones with pairs, start beyond
    slot 2^31 of both key arrays and equal the shim's fixed rooms, with count and without it.  Their counts lie below K, between K
    and the scene's 4800, and at 4800; 16 of them fill their room from instance 0 alone, so the run without count asks `go` before
    instance 1 with a full room and reads the room's root at slot i * K > 2^31.  (That read cannot change a room: a full room's keys
    all come from earlier instances, so a correct read always ends the traversal, and a wrong one that goes on finds the same keys.
    What the run shows is that the read stays inside the array and the rooms are right.)  The rooms of a sample of the other boxes
    (the first, the last, and those around slot 2^31) are all padding."""
    import torch
    K, n = 2049, 2 ** 20 + 64
    rng = np.random.default_rng(71)
    few, mid, full = rng.integers(100, 500, 16), rng.integers(520, 1000, 16), rng.integers(1030, 1190, 16)
    last = [_slab(int(a), int(a + m - 1)) for m in np.concatenate([few, mid, full]) for a in [rng.integers(0, QUADS - m)]]
    last = np.concatenate([np.stack(last), _thin(rng, 15), _slab(-10, QUADS + 10)[None]])
    last = np.ascontiguousarray(last[rng.permutation(64)])
    boxes = np.tile(FAR_BOX, (n, 1, 1))
    boxes[-64:] = last
    ref = bo.rooms(stack.so, last, max_hits=K)
    c = ref["count"]
    assert ((c > 0) & (c < K)).sum() >= 16 and ((c >= K) & (c < 4 * QUADS)).sum() >= 32 and (c == 4 * QUADS).sum() == 1, c
    assert (c // 2 >= K).sum() >= 16 and (n - 64) * K > 2 ** 31
    assert (bo.count_in_boxes(stack.so, boxes[:64]) == 0).all()
    _need_memory(2 * 4 * n * K)
    bufs = None
    try:
        bufs = {k: torch.empty(n * K, dtype=torch.int32, device="cuda") for k in bo.FIELDS}
        sample = sorted({0, 1, 63, 64, 2 ** 19, 2 ** 31 // K - 1, 2 ** 31 // K, 2 ** 31 // K + 1, n - 66, n - 65})
        bt, = _up((boxes,))
        for with_count in (True, False):
            at = "with count" if with_count else "without count"
            for b in bufs.values():
                for i in sample:
                    b[i * K:(i + 1) * K].fill_(GUARD32)
                b[(n - 64) * K:].fill_(GUARD32)
            cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda") if with_count else None
            assert _box_list(rt, stack.handle, bt, n, None, K, bufs["instance"], bufs["triangle"], cnt) == 0
            for k in bo.FIELDS:
                _eq(bufs[k][(n - 64) * K:].cpu().numpy(), ref[k], "%s of the last 64 rooms, %s" % (k, at))
                for i in sample:
                    room = bufs[k][i * K:(i + 1) * K].cpu().numpy()
                    assert (room == -1).all(), "%s of room %d (a box without pairs), %s: %d slots are not padding" % (
                        k, i, at, int((room != -1).sum()))
            if with_count:
                got = cnt.cpu().numpy()
                _eq(got[-64:], c, "count of the last 64")
                assert (got[:-64] == 0).all()
    finally:
        del bufs
        torch.cuda.empty_cache()


# ---- B4d: the section list's heap rooms where 6 * slot and 3 * slot pass 2^32, and where the slot does --------------------------------
GUARDF = np.frombuffer(bytes([GUARD]) * 4, F32)[0]             # the float whose words are GUARD32
SC_WIDTH = dict(instance=1, triangle=1, segment=6, normal=3)    # int32 words per slot
SC_FILL = dict(instance=GUARD32, triangle=GUARD32, segment=GUARDF, normal=GUARDF)
FAR_PLANE = np.array([[50, 50, 50], [1, 1, 1]], F32)
X_HALF = np.array([[0.5, 0.5, 6.0], [1, 0, 0]], F32)            # cuts every triangle of the stack: 4 * QUADS pairs


def _tilt(a, m):
    """the plane through (0.5, 0.5, z0) with normal (1, 0, 1 / (m * 0.01)): over the quads' footprint its z runs through m * 0.01, and
    z0 is set so that this is from half a spacing below quad a to half a spacing above quad a + m - 1.  It cuts both triangles of
    those m quads in both instances, 4 * m pairs"""
    return np.array([[0.5, 0.5, (a + m / 2.0) * 0.01 - 0.005], [1.0, 0.0, 1.0 / (m * 0.01)]], F32)


def _flat_plane(z):
    return np.array([[0.5, 0.5, z], [0, 0, 1]], F32)


def _sc_words(a, k):
    """a shim field as flat int32 words, as the buffers below hold the product's"""
    return np.ascontiguousarray(a).view(np.int32).reshape(-1)


def _section_list(rt, handle, planes, n, offsets_ptr, max_hits, bufs, cnt):
    """rt_list_sections on device buffers (bufs: field -> int32 words, a missing field is not asked for), synchronous on the NULL
    stream"""
    import torch
    lst = rt.RtSectionList(*[bufs[k].data_ptr() if k in bufs else None for k in sc.FIELDS], None if cnt is None else cnt.data_ptr(), None)
    torch.cuda.synchronize()
    return rt.libs()[0].rt_list_sections(handle, planes.data_ptr(), n, offsets_ptr, max_hits, C.byref(lst), None, 1)


def _csr_planes():
    """400 planes on the quad stack, shuffled: one of 1200 pairs, two of 400, four of 100, 150 without pairs (far off, or parallel to
    the quads, on one or between two) and 243 thin tilted ones over one to three quads -> (planes, rng)"""
    rng = np.random.default_rng(101)
    big = [_tilt(100, 300), _tilt(500, 100), _tilt(700, 100)] + [_tilt(a, 25) for a in (0, 450, 900, 1175)]
    none = [FAR_PLANE] * 50 + [_flat_plane(int(k) * 0.01) for k in rng.integers(0, QUADS, 50)] + \
           [_flat_plane(int(k) * 0.01 + 0.004) for k in rng.integers(0, QUADS, 50)]
    thin = [_tilt(int(a), int(m)) for m in rng.choice([1, 2, 3], 243, p=[0.6, 0.3, 0.1]) for a in [rng.integers(0, QUADS - m + 1)]]
    planes = np.stack(big + none + thin)
    return np.ascontiguousarray(planes[rng.permutation(len(planes))]), rng


@pytest.mark.parametrize("fields,base", [((), 2 ** 31 + 5), ((), 2 ** 32 + 5), (("normal",), -(-2 ** 32 // 3) + 5),
                                         (("segment",), -(-2 ** 32 // 6) + 5)],
                         ids=["keys-2^31", "keys-2^32", "normal-2^32/3", "segment-2^32/6"])
def test_section_csr_rooms_at_large_slots(rt, stack, fields, base):
    """test_box_csr_rooms_beyond_32_bits for rt_list_sections, whose heap has slot arithmetic of its own: ScRoom's get and put
    (under room_insert, room_sift_down and room_sort) index segment + 6 * q and normal + 3 * q, and the pair's record slot travels through the heap in the first word of
    the entry's segment (of its normal when no segment is asked for).  400 planes on the quad stack with hand-made offsets base +
    cumsum(room), counted in slots, rooms below, at and above each count (two deep heaps of 400 pairs at half their count, so most
    arrivals replace the root and sift a long way with their slot); the lists run to 1200 entries.  With the keys alone the base is
    2^31 + 5 and 2^32 + 5 (xl_room's start and the key index); with the normal it is ceil(2^32 / 3) + 5, with the segment
    ceil(2^32 / 6) + 5, so that 3 * q and 6 * q pass 2^32 where q does not.  In every given field of W words per slot the window
    around the rooms equals the shim's rooms, guard words of 64 slots either side included, and the first W * 4096 words (where a
    start cut to 32 bits, or a product 3 * q or 6 * q taken in 32 bits, would land: W * base mod 2^32 is 17 and 32) keep their
    guard.  Float fields are compared as int32 words.  count equals the shim's.  (Every quad has the normal (0, 0, 1), so the normal
    case shows where the words go and no more; a slot that room_insert's sift-up or room_sift_down leaves behind shows in the segment case, whose
    segments differ from triangle to triangle.)"""
    import torch
    planes, rng = _csr_planes()
    n = len(planes)
    given = ("instance", "triangle") + fields
    c = sc.count_sections(stack.so, planes).astype(np.int64)
    assert c.max() == 1200 and (c == 400).sum() == 2 and (c == 100).sum() == 4 and (c == 0).sum() == 150, np.unique(c, return_counts=True)
    assert set(np.unique(c)) == {0, 4, 8, 12, 100, 400, 1200}
    room = np.maximum(c + rng.integers(-1, 3, n), 0)
    half = np.flatnonzero(c == 400)
    room[half] = c[half] // 2
    assert (room < c).any() and (room > c).any() and (room == c).any() and (room == 0).any()
    assert all((room[c == v] < v).any() and (room[c == v] > v).any() for v in (4, 8))       # (thin rooms of either kind)
    rooms = int(room.sum())
    assert rooms + 5 + 64 <= 4096                               # (offsets mod 2^32 fall inside the head window)
    for k in given:                                             # (a word index cut to 32 bits falls inside the head window)
        W = SC_WIDTH[k]
        assert W * base < 2 ** 32 or (W * base) % 2 ** 32 + W * (rooms + 64) <= W * 4096, (k, base)
    if fields:                                                  # (the product passes 2^32, the slot not 2^31)
        assert base + rooms + 64 < 2 ** 31 and SC_WIDTH[fields[0]] * base > 2 ** 32
    else:
        assert base > 2 ** 31
    offsets = (base + _cumsum(room)).astype(np.int64)
    nslots = base + rooms + 64
    _need_memory(4 * nslots * sum(SC_WIDTH[k] for k in given))
    lo, hi = base - 64, base + rooms + 64
    ref = sc.rooms(stack.so, planes, offsets=offsets - lo, slots=hi - lo, fill=SC_FILL)
    _eq(ref["count"], c, "the shim's count beside its rooms")
    bufs = None
    try:
        bufs = {k: torch.empty(SC_WIDTH[k] * nslots, dtype=torch.int32, device="cuda") for k in given}
        for k, b in bufs.items():
            b[SC_WIDTH[k] * lo:SC_WIDTH[k] * hi].fill_(GUARD32)
            b[:SC_WIDTH[k] * 4096].fill_(GUARD32)
        cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        doff = torch.from_numpy(offsets).cuda()
        pt, = _up((planes,))
        assert _section_list(rt, stack.handle, pt, n, doff.data_ptr(), 0, bufs, cnt) == 0
        for k in given:
            W = SC_WIDTH[k]
            window, head = bufs[k][W * lo:W * hi].cpu().numpy(), bufs[k][:W * 4096].cpu().numpy()
            assert (head == GUARD32).all(), "%s: %d of the array's first %d words were written" % (k, int((head != GUARD32).sum()), W * 4096)
            _eq(window, _sc_words(ref[k], k), "%s rooms at slot %d" % (k, base))
        _eq(cnt.cpu().numpy(), ref["count"], "count")
    finally:
        del bufs
        torch.cuda.empty_cache()


@pytest.mark.parametrize("fields,n", [((), 2 ** 20 + 64), (("segment",), 2 ** 19 + 64)], ids=["keys", "segment"])
def test_section_fixed_rooms_at_large_slots(rt, stack, fields, n):
    """max_hits = 2049 on the quad stack; every plane but the last 64 lies far off.  With the keys alone n = 2^20 + 64 and the last 64
    rooms start beyond slot 2^31; with the segment n = 2^19 + 64, they start at slot 1 074 266 112, and 6 * q there is about 6.4e9,
    above 2^32.  The last 64 rooms equal the shim's fixed rooms in every given field, with count and without it.  Their counts lie
    below K (16 planes over 25 to 124 quads, and 15 thin ones), between K and the scene's 4800 (32 planes), and at 4800 (x = 0.5);
    17 of them fill their room from instance 0 alone, so the run without count asks `go` before instance 1 with a full room and reads
    the room's root p.instance[i * K] at a slot beyond 2^31 (keys alone) or 2^30 (with the segment).  (That read cannot change a
    room: a full room's keys all come from earlier instances, so a correct read always ends the traversal, and a wrong one that goes
    on finds only greater keys.  What the run shows is that the read stays inside the array and the rooms are right, no more.)  The
    rooms of a sample of the other planes (the first, the last, and those around the slots where q passes 2^31 and 6 * q passes
    2^31 and 2^32) are all padding: keys of -1 and segment words of 0.0."""
    import torch
    K = 2049
    rng = np.random.default_rng(103)
    few, mid, full = rng.integers(25, 125, 16), rng.integers(520, 1000, 16), rng.integers(1030, 1190, 16)
    ms = np.concatenate([few, mid, full, rng.integers(1, 4, 15)])
    last = [_tilt(int(a), int(m)) for m in ms for a in [rng.integers(0, QUADS - m + 1)]] + [X_HALF]
    order = rng.permutation(64)
    last, want = np.ascontiguousarray(np.stack(last)[order]), np.append(4 * ms, 4 * QUADS)[order]
    planes = np.tile(FAR_PLANE, (n, 1, 1))
    planes[-64:] = last
    given = ("instance", "triangle") + fields
    ref = sc.rooms(stack.so, last, max_hits=K)
    c = ref["count"]
    _eq(c, want.astype(np.int32), "the shim's counts of the last 64 planes")
    assert ((c >= 100) & (c < 500)).sum() == 16 and ((c >= K) & (c < 4 * QUADS)).sum() == 32 and (c == 4 * QUADS).sum() == 1, c
    assert ((c > 0) & (c <= 12)).sum() == 15 and (c // 2 >= K).sum() == 17
    W = sum(SC_WIDTH[k] for k in given)
    assert (n - 64) * K * max(SC_WIDTH[k] for k in given) > 2 ** 31 * (1 if not fields else 2)
    assert (sc.count_sections(stack.so, planes[:64]) == 0).all()
    _need_memory(4 * W * n * K)
    marks = [2 ** 31 // K, 2 ** 31 // 6 // K, 2 ** 32 // 6 // K]
    sample = sorted({i for i in [0, 1, 63, 64, n // 2, n - 66, n - 65] + [m + j for m in marks for j in (-1, 0, 1)] if i < n - 64})
    assert len(sample) >= 13
    bufs = None
    try:
        bufs = {k: torch.empty(SC_WIDTH[k] * n * K, dtype=torch.int32, device="cuda") for k in given}
        pt, = _up((planes,))
        for with_count in (True, False):
            at = "with count" if with_count else "without count"
            for k, b in bufs.items():
                w = SC_WIDTH[k] * K
                for i in sample:
                    b[i * w:(i + 1) * w].fill_(GUARD32)
                b[(n - 64) * w:].fill_(GUARD32)
            cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda") if with_count else None
            assert _section_list(rt, stack.handle, pt, n, None, K, bufs, cnt) == 0
            for k in given:
                w = SC_WIDTH[k] * K
                _eq(bufs[k][(n - 64) * w:].cpu().numpy(), _sc_words(ref[k], k), "%s of the last 64 rooms, %s" % (k, at))
                pad = 0 if k == "segment" else -1
                for i in sample:
                    room = bufs[k][i * w:(i + 1) * w].cpu().numpy()
                    assert (room == pad).all(), "%s of room %d (a plane without pairs), %s: %d words are not padding" % (
                        k, i, at, int((room != pad).sum()))
            if with_count:
                got = cnt.cpu().numpy()
                _eq(got[-64:], c, "count of the last 64")
                assert (got[:-64] == 0).all()
    finally:
        del bufs
        torch.cuda.empty_cache()


# ---- B4e: the region list's heap rooms where the slot (the flag's byte index) passes 2^31 and 2^32 and where 3 * slot passes 2^32 ------
RG_WIDTH = dict(instance=1, triangle=1, inside=1, normal=3)     # elements per slot: int32 words, the flag's bytes
RG_FILL = dict(instance=GUARD32, triangle=GUARD32, inside=GUARD, normal=GUARDF)
RG_PAD = dict(instance=-1, triangle=-1, inside=0, normal=0)     # (as words: the floats' padding is 0.0)
FAR_REGION = np.stack([FAR_PLANE, FAR_PLANE])


def _wedge(a, m, b):
    """the K = 2 region above _tilt(a, m) and below z = b * 0.01 + 0.005, half a spacing above quad b (a <= b, 1 <= m <= b - a + 1): it
    touches the quads a..b, both triangles in both instances, and holds the quads a + m..b whole"""
    assert 0 <= a <= b and 1 <= m <= b - a + 1
    return np.stack([_tilt(a, m), np.array([[0.5, 0.5, b * 0.01 + 0.005], [0, 0, -1]], F32)])


def _wedge_counts(a, m, b):
    """-> (count, inside) of _wedge(a, m, b) on the stack, in closed form"""
    return 4 * (b - a + 1), 4 * (b - a - m + 1)


def _wedges(specs):
    """(a, m, b) rows -> (regions [len, 2, 2, 3], count, inside)"""
    c = np.array([_wedge_counts(*s) for s in specs], np.int32).reshape(-1, 2)
    return np.stack([_wedge(*s) for s in specs]), c[:, 0], c[:, 1]


def _csr_regions():
    """400 K = 2 regions on the quad stack, shuffled: one wedge of 1200 pairs, two of 400, four of 100 (half of the pairs of the large
    ones are whole inside, 60 of the 100), 150 without pairs (75 far off, 74 whose two half-spaces z >= z1 and z <= z0 < z1 face
    apart, and the largest wedge with a zero normal in its second plane) and 243 thin wedges over one to three quads -> (regions,
    count and inside in closed form, rng)"""
    rng = np.random.default_rng(127)
    big = [(100, 150, 399), (500, 50, 599), (700, 50, 799)] + [(a, 10, a + 24) for a in (0, 450, 900, 1175)]
    thin = [(int(a), int(rng.integers(1, k + 1)), int(a + k - 1)) for k in rng.choice([1, 2, 3], 243, p=[0.6, 0.3, 0.1])
            for a in [rng.integers(0, QUADS - k + 1)]]
    regions, count, inside = _wedges(big + thin)
    z = np.sort(rng.uniform(0.0, 12.0, (74, 2)), axis=1) + np.array([0.0, 0.001])
    apart = np.stack([np.stack([_flat_plane(z1), np.array([[0.5, 0.5, z0], [0, 0, -1]], F32)]) for z0, z1 in z])
    zero = _wedge(0, 600, 1199)
    zero[1, 1] = 0
    none = np.concatenate([np.tile(FAR_REGION, (75, 1, 1, 1)), apart, zero[None]])
    order = rng.permutation(400)
    regions = np.ascontiguousarray(np.concatenate([regions, none])[order], F32)
    pad = np.zeros(150, np.int32)
    return regions, np.concatenate([count, pad])[order], np.concatenate([inside, pad])[order], rng


def _csr_region_rooms(count, rng):
    """rooms below, at and above each count; the two wedges of 400 pairs get half their count (deep heaps: every pair of the second
    instance, and most of the first's, meets a full room) -> int64 [n]"""
    c = count.astype(np.int64)
    room = np.maximum(c + rng.integers(-1, 3, len(c)), 0)
    room[c == 400] = 200
    return room


def _mixed_flags(flags, c, room, offsets):
    """every list of at least 100 pairs holds both values of the inside flag, each in at least a quarter of its entries -> the number
    of such lists.  flags: the shim's flat `inside`; region i's entries lie at offsets[i] .. offsets[i] + min(room, count)."""
    lists = 0
    for i in np.flatnonzero(c >= 100):
        f = flags[offsets[i]:offsets[i] + min(room[i], c[i])]
        assert len(f) >= 99
        assert set(np.unique(f)) == {0, 1} and 0.25 <= f.mean() <= 0.75, (i, c[i], room[i], f.mean())
        lists += 1
    return lists


def _last64_regions():
    """the fixed-room tests' last 64 regions, shuffled: 16 wedges over 25 to 124 quads, 32 over 520 to 1189, the whole stack, and 15
    thin ones; each wedge's tilted plane spans half of its quads, so half of its pairs are whole inside -> (regions, count, inside)"""
    rng = np.random.default_rng(131)
    spans = np.concatenate([rng.integers(25, 125, 16), rng.integers(520, 1000, 16), rng.integers(1030, 1190, 16), rng.integers(1, 4, 15)])
    specs = [(int(a), max(1, int(s) // 2), int(a + s - 1)) for s in spans for a in [rng.integers(0, QUADS - s + 1)]] + [(0, 600, 1199)]
    regions, count, inside = _wedges(specs)
    order = rng.permutation(64)
    return np.ascontiguousarray(regions[order], F32), count[order], inside[order]


def _last64_bands(c, K):
    """what the fixed-room tests need of the last 64 counts"""
    assert ((c >= 100) & (c < 500)).sum() == 16 and ((c >= K) & (c < 4 * QUADS)).sum() == 32 and (c == 4 * QUADS).sum() == 1, c
    assert ((c > 0) & (c <= 12)).sum() == 15 and (c // 2 >= K).sum() >= 17


def _rg_words(a, k):
    """a shim field as the flat elements the buffers below hold: the flag's bytes, everything else as int32 words"""
    a = np.ascontiguousarray(a)
    return a.reshape(-1) if k == "inside" else a.view(np.int32).reshape(-1)


def _rg_buffer(k, nslots):
    import torch
    return torch.empty(RG_WIDTH[k] * nslots, dtype=torch.uint8 if k == "inside" else torch.int32, device="cuda")


def _rg_guard(k):
    return GUARD if k == "inside" else GUARD32


def _rg_bytes(given, nslots):
    return nslots * sum(RG_WIDTH[k] * (1 if k == "inside" else 4) for k in given)


def _region_list(rt, handle, regions, n, offsets_ptr, max_hits, bufs, cnt):
    """rt_list_in_regions on device buffers (bufs: field -> elements, a missing field is not asked for), synchronous on the NULL
    stream; planes_per_region from the regions' shape"""
    import torch
    lst = rt.RtRegionList(*[bufs[k].data_ptr() if k in bufs else None for k in ro.FIELDS], None if cnt is None else cnt.data_ptr(), None)
    torch.cuda.synchronize()
    return rt.libs()[0].rt_list_in_regions(handle, regions.data_ptr(), n, int(regions.shape[1]), offsets_ptr, max_hits, C.byref(lst), None, 1)


@pytest.mark.parametrize("fields,base", [((), 2 ** 31 + 5), ((), 2 ** 32 + 5), (("inside",), 2 ** 31 + 5), (("inside",), 2 ** 32 + 5),
                                         (("normal",), -(-2 ** 32 // 3) + 5), (("inside", "normal"), -(-2 ** 32 // 3) + 5)],
                         ids=["keys-2^31", "keys-2^32", "inside-2^31", "inside-2^32", "normal-2^32/3", "inside+normal-2^32/3"])
def test_region_csr_rooms_at_large_slots(rt, flipstack, fields, base):
    """test_section_csr_rooms_at_large_slots for rt_list_in_regions, whose heap has slot arithmetic of its own: RgRoom's get and put
    (under room_insert, room_sift_down and room_sort) index the one-byte flag[q], whose byte index is the slot itself, and
    normal + 3 * q; the pair's record slot travels through the heap in the first word of the entry's normal, its inside flag in its own
    byte.  400 K = 2 wedges on the quad stack with half of its windings reversed, with hand-made offsets base + cumsum(room), counted
    in slots, rooms below, at and above each count (two deep heaps of 400 pairs at half their count, so most arrivals replace the
    root and sift a long way with their flag and slot); the lists run to 1200 entries.  With the keys alone, and with the flag, the
    base is 2^31 + 5 and 2^32 + 5 (xl_room's start, the key index and the flag's byte index); with the normal it is
    ceil(2^32 / 3) + 5, so that 3 * q passes 2^32 where q stays below 2^31, alone and with the flag beside it.  The shim's count and
    inside of every region equal their closed forms before anything is allocated.  In every given field of W elements per slot the
    window around the rooms equals the shim's rooms, guards of 64 slots either side included, and the first W * 4096 elements (where a
    start cut to 32 bits, or a product 3 * q taken in 32 bits, would land: 3 * base mod 2^32 is 17) keep their guard.  Floats are
    compared as int32 words; the flag buffer is uint8.  count equals the shim's.  Along every list of at least 100 entries both flag
    values hold at least a quarter each and, the quads being shuffled in z, alternate; the normals are (0, 0, +-c) by the quad's
    winding: an entry left with another's flag or record slot by room_insert's sift-up, room_sift_down or room_sort differs."""
    import torch
    regions, want_c, want_in, rng = _csr_regions()
    n = len(regions)
    given = ("instance", "triangle") + fields
    shim = ro.count_in_regions(flipstack.so, regions)
    _eq(shim["count"], want_c, "the shim's count against 4 * (b - a + 1)")
    _eq(shim["inside"], want_in, "the shim's inside against 4 * (b - a - m + 1)")
    c = want_c.astype(np.int64)
    assert c.max() == 1200 and (c == 400).sum() == 2 and (c == 100).sum() == 4 and (c == 0).sum() == 150, np.unique(c, return_counts=True)
    assert set(np.unique(c)) == {0, 4, 8, 12, 100, 400, 1200}
    room = _csr_region_rooms(want_c, rng)
    assert (room < c).any() and (room > c).any() and (room == c).any() and (room == 0).any() and (room[c == 400] == 200).all()
    assert all((room[c == v] < v).any() and (room[c == v] > v).any() for v in (4, 8))       # (thin rooms of either kind)
    rooms = int(room.sum())
    assert rooms + 5 + 64 <= 4096                               # (offsets mod 2^32 fall inside the head window)
    for k in given:                                             # (an element index cut to 32 bits falls inside the head window)
        W = RG_WIDTH[k]
        assert W * base < 2 ** 32 or (W * base) % 2 ** 32 + W * (rooms + 64) <= W * 4096, (k, base)
    if "normal" in fields:                                      # (the product passes 2^32, the slot not 2^31)
        assert base + rooms + 64 < 2 ** 31 and 3 * base > 2 ** 32
    else:                                                       # (the slot, and with it the flag's byte index, passes the boundary)
        assert base > 2 ** 31
    offsets = (base + _cumsum(room)).astype(np.int64)
    nslots = base + rooms + 64
    _need_memory(_rg_bytes(given, nslots))
    lo, hi = base - 64, base + rooms + 64
    ref = ro.rooms(flipstack.so, regions, offsets=offsets - lo, slots=hi - lo, fill=RG_FILL)
    _eq(ref["count"], want_c, "the shim's count beside its rooms")
    assert _mixed_flags(ref["inside"], c, room, offsets - lo) == 7
    bufs = None
    try:
        bufs = {k: _rg_buffer(k, nslots) for k in given}
        for k, b in bufs.items():
            b[RG_WIDTH[k] * lo:RG_WIDTH[k] * hi].fill_(_rg_guard(k))
            b[:RG_WIDTH[k] * 4096].fill_(_rg_guard(k))
        cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda")
        doff = torch.from_numpy(offsets).cuda()
        bt, = _up((regions,))
        assert _region_list(rt, flipstack.handle, bt, n, doff.data_ptr(), 0, bufs, cnt) == 0
        for k in given:
            W = RG_WIDTH[k]
            window, head = bufs[k][W * lo:W * hi].cpu().numpy(), bufs[k][:W * 4096].cpu().numpy()
            assert (head == _rg_guard(k)).all(), "%s: %d of the array's first %d elements were written" % (
                k, int((head != _rg_guard(k)).sum()), W * 4096)
            _eq(window, _rg_words(ref[k], k), "%s rooms at slot %d" % (k, base))
        _eq(cnt.cpu().numpy(), ref["count"], "count")
    finally:
        del bufs
        torch.cuda.empty_cache()


@pytest.mark.parametrize("fields,n", [(("inside",), 2 ** 20 + 64), (("normal",), 2 ** 19 + 2 ** 18 + 64)], ids=["inside", "normal"])
def test_region_fixed_rooms_at_large_slots(rt, flipstack, fields, n):
    """max_hits = 2049 on the quad stack with half of its windings reversed; every region but the last 64 lies far off.  With the keys
    and the flag n = 2^20 + 64 and the last 64 rooms start beyond slot, and flag byte, 2^31; with the keys and the normal n = 2^19 +
    2^18 + 64, they start at slot 1 611 399 168 < 2^31, and 3 * q there is about 4.83e9, above 2^32.  The last 64 rooms equal the
    shim's fixed rooms in every given field, with count and without it.  Their counts lie below K (16 wedges over 25 to 124 quads,
    and 15 thin ones), between K and the scene's 4800 (32 wedges), and at 4800; 17 of them fill their room from instance 0 alone, so
    the run without count asks `go` before instance 1 with a full room and reads the room's root p.instance[i * K] at a large slot.
    (That read cannot change a room: a full room's keys all come from earlier instances, so a correct read always ends the traversal,
    and a wrong one that goes on finds only greater keys.  What the run shows is that the read stays inside the array and the rooms
    are right, no more.)  The rooms of a sample of the other regions (the first, the last, and those around the slots where q -- the
    flag's byte index -- and 3 * q pass 2^31 and 2^32, and those where the last rooms' 3 * q cut to 32 bits would land) are all
    padding: keys of -1, flags of 0 and normal words of 0.0."""
    import torch
    K = 2049
    last, want_c, want_in = _last64_regions()
    regions = np.tile(FAR_REGION, (n, 1, 1, 1))
    regions[-64:] = last
    given = ("instance", "triangle") + fields
    shim = ro.count_in_regions(flipstack.so, last)
    _eq(shim["count"], want_c, "the shim's count of the last 64 regions against 4 * (b - a + 1)")
    _eq(shim["inside"], want_in, "the shim's inside of the last 64 regions against 4 * (b - a - m + 1)")
    _last64_bands(want_c, K)
    if "normal" in fields:
        assert n * K < 2 ** 31 and 3 * (n - 64) * K > 2 ** 32
    else:
        assert (n - 64) * K > 2 ** 31
    assert (ro.count_in_regions(flipstack.so, regions[:64])["count"] == 0).all()
    _need_memory(_rg_bytes(given, n * K))
    ref = ro.rooms(flipstack.so, last, max_hits=K)
    c = ref["count"]
    _eq(c, want_c, "the shim's count beside its rooms")
    assert _mixed_flags(ref["inside"], c.astype(np.int64), np.full(64, K), np.arange(64) * K) == 49
    marks = [2 ** 31 // K, 2 ** 32 // K, 2 ** 31 // 3 // K, 2 ** 32 // 3 // K]
    # (and the rooms where the last 64 rooms' q, or 3 * q, cut to 32 bits would land: a product taken in 32 bits on both sides of the
    # heap is consistent with itself and leaves the last rooms right; what shows is the slot it wrote into another region's room)
    cut = [(W * (n - 64) * K) % 2 ** 32 // (W * K) + j for W in (1, 3) for j in (0, 1, 32, 63)]
    sample = sorted({i for i in [0, 1, 63, 64, n // 2, n - 66, n - 65] + cut + [m + j for m in marks for j in (-1, 0, 1)] if i < n - 64})
    assert len(sample) >= 13 and ("normal" not in fields or len([i for i in cut[4:] if i in sample]) == 4)
    bufs = None
    try:
        bufs = {k: _rg_buffer(k, n * K) for k in given}
        bt, = _up((regions,))
        for with_count in (True, False):
            at = "with count" if with_count else "without count"
            for k, b in bufs.items():
                w = RG_WIDTH[k] * K
                for i in sample:
                    b[i * w:(i + 1) * w].fill_(_rg_guard(k))
                b[(n - 64) * w:].fill_(_rg_guard(k))
            cnt = torch.full((n,), -9, dtype=torch.int32, device="cuda") if with_count else None
            assert _region_list(rt, flipstack.handle, bt, n, None, K, bufs, cnt) == 0
            for k in given:
                w = RG_WIDTH[k] * K
                _eq(bufs[k][(n - 64) * w:].cpu().numpy(), _rg_words(ref[k], k), "%s of the last 64 rooms, %s" % (k, at))
                for i in sample:
                    room = bufs[k][i * w:(i + 1) * w].cpu().numpy()
                    assert (room == RG_PAD[k]).all(), "%s of room %d (a region without pairs), %s: %d elements are not padding" % (
                        k, i, at, int((room != RG_PAD[k]).sum()))
            if with_count:
                got = cnt.cpu().numpy()
                _eq(got[-64:], c, "count of the last 64")
                assert (got[:-64] == 0).all()
    finally:
        del bufs
        torch.cuda.empty_cache()


# ---- B4c: occupancy grids on the grid kernel's second launch row and at 2^24 cells on an axis ---------------------------------------
ROW = 65536                                                     # bricks per launch row of rt_occupancy_grid (blockIdx.y counts rows)
GRIDS = {
    # the cube's top face z = 1 lies in the last brick's second cell; the column stands inside the cube in x and y
    "A": dict(dims=(1, 1, 262148), spacing=(0.37, 0.37, 0.0003), origin=(0.3, 0.3, 1 - 262145.5 * 0.0003), mix=1),
    # the top face lies in the last layer iz = 65536, the only one of bricks 65536..65539: 25 cells, 12 over the face and 13 beside it
    "B": dict(dims=(5, 5, 65537), spacing=(0.37, 0.47, 0.0003), origin=(-0.5, -0.6, 1 - 65536.5 * 0.0003), mix=8),
}


def _brick_of_cells(dims):
    """the launch's brick index of every cell, [nz, ny, nx]"""
    nx, ny, nz = dims
    bx, by = (nx + 3) // 4, (ny + 3) // 4
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (iz // 4 * by + iy // 4) * bx + ix // 4


def _grid_raw(rt, handle, origin, spacing, dims, outputs):
    """rt_occupancy_grid straight through the C-ABI into buffers with a brick of guard cells either side -> dict of flat arrays"""
    import torch
    cells = int(np.prod(dims, dtype=np.int64))
    occ = torch.full((cells + 128,), GUARD, dtype=torch.uint8, device="cuda") if "occupied" in outputs else None
    cnt = torch.full((cells + 128,), -9, dtype=torch.int32, device="cuda") if "count" in outputs else None
    o, s, d = (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_int32 * 3)(*dims)
    torch.cuda.synchronize()
    rc = rt.libs()[0].rt_occupancy_grid(handle, o, s, d, None if occ is None else occ.data_ptr() + 64,
                                        None if cnt is None else cnt.data_ptr() + 4 * 64, None, 1)
    assert rc == 0, rc
    out = {}
    for k, t, g in (("occupied", occ, GUARD), ("count", cnt, -9)):
        if t is not None:
            a = t.cpu().numpy()
            assert (a[:64] == g).all() and (a[64 + cells:] == g).all(), "%s: cells outside the grid %s were written" % (k, dims)
            out[k] = a[64:64 + cells]
    return out


@pytest.mark.parametrize("case", sorted(GRIDS))
def test_occupancy_grid_on_the_second_launch_row(rt, cube, case):
    """rt_occupancy_grid launches min(bricks, 65536) x ceil(bricks / 65536) workgroups and rebuilds the brick from both indices.
    A: (1, 1, 262148), 65537 bricks, the fewest cells with a brick (one, of four cells) in the second row.  B: (5, 5, 65537),
    2 x 2 x 16385 = 65540 bricks, partial on every axis, four of them (the 25 cells of the last layer) in the second row.  The spacing
    is not representable; the cube's top face lies in the last cells, so the second row's cells hold both kinds: in A at least one
    cell with a count above 0 and one with 0, in B at least 8 of each (the 16 of each that the first row's cells give cannot be asked
    of 25 cells), and the same mix holds below brick 65536.  count with occupied, and occupied alone (the kernel that stops at the
    first pair), equal the shim's count_in_boxes over ALL cells made by grid_boxes -- through the C-ABI into buffers guarded a brick
    either side, whose guards stay, through the numpy path and through the torch path."""
    g = GRIDS[case]
    dims = g["dims"]
    origin, spacing = np.asarray(g["origin"], F32), np.asarray(g["spacing"], F32)
    assert all(float(F32(x)) != x for x in g["spacing"])
    bricks = int(np.prod([(d + 3) // 4 for d in dims]))
    assert ROW < bricks <= ROW + 4
    ref = bo.count_in_boxes(cube.so, bo.grid_boxes(origin, spacing, dims), threads=16).reshape(dims[::-1])
    second = _brick_of_cells(dims) >= ROW
    assert second.sum() == {"A": 4, "B": 25}[case]
    for where, m, want in (("second row", second, g["mix"]), ("first row", ~second, 16 if case == "B" else 1)):
        assert (ref[m] > 0).sum() >= want and (ref[m] == 0).sum() >= want, (case, where, int((ref[m] > 0).sum()), int(m.sum()))
    both = _grid_raw(rt, cube.handle, origin, spacing, dims, ("occupied", "count"))
    _eq(both["count"].reshape(ref.shape), ref, "grid %s count" % case)
    assert np.array_equal(both["occupied"].reshape(ref.shape), (ref > 0).astype(np.uint8)), "grid %s occupied beside count" % case
    alone = _grid_raw(rt, cube.handle, origin, spacing, dims, ("occupied",))
    assert np.array_equal(alone["occupied"].reshape(ref.shape), (ref > 0).astype(np.uint8)), "grid %s occupied alone" % case
    r = cube.sp.occupancy_grid(origin, spacing, dims, outputs=("occupied", "count"), as_numpy=True)
    _eq(r["count"], ref, "grid %s count (numpy path)" % case)
    assert np.array_equal(r["occupied"], ref > 0)
    r = cube.sp.occupancy_grid(origin, spacing, dims, as_numpy=True)
    assert np.array_equal(r["occupied"], ref > 0), "grid %s occupied alone (numpy path)" % case
    t = cube.sp.occupancy_grid(origin, spacing, dims, outputs=("occupied", "count"))
    _eq(t["count"].cpu().numpy(), ref, "grid %s count (torch path)" % case)
    assert np.array_equal(t["occupied"].cpu().numpy(), ref > 0)
    t = cube.sp.occupancy_grid(origin, spacing, dims)
    assert np.array_equal(t["occupied"].cpu().numpy(), ref > 0), "grid %s occupied alone (torch path)" % case


def test_occupancy_grid_at_the_axis_limit(rt, cube):
    """dims = (2^24, 1, 1), the documented maximum of an axis: 4 194 304 bricks in 64 launch rows, and (float)(ix + 1) reaches 2^24.
    The row of cells runs along x inside the cube in y and z; the spacing (1.2e-7, a few units in the last place of the cells'
    bounds, so many cells are planes) is not representable; the face x = 0 falls mid-grid and x = 1 in the last 64 cells.  The shim
    needs minutes for 2^24 cells, so the whole GPU output is compared with it on a subset: the first and the last 65536 cells, 2^18
    cells drawn with a fixed seed, and every cell within 64 of a cell the GPU reports as non-empty.  The GPU reports at most 1024
    such cells, so each of them is checked against the shim, and so are the cells where the shim expects them (the last 64, and the
    other face's).  Cells outside the subset are only known to be empty on the GPU: the shim was not asked about them, because asking
    it about all of them is what takes minutes; a cell the kernel wrongly reports empty far from every face would go unseen unless
    the 2^18 drawn cells hit it."""
    dims = (2 ** 24, 1, 1)
    cells = dims[0]
    spacing = np.asarray((1.2e-7, 0.37, 0.37), F32)
    origin = np.asarray((1 - (cells - 32) * 1.2e-7, 0.3, 0.3), F32)
    assert float(spacing[0]) != 1.2e-7
    rng = np.random.default_rng(73)
    fixed = np.unique(np.concatenate([np.arange(ROW), np.arange(cells - ROW, cells), rng.integers(0, cells, 2 ** 18)]))
    fixed_ref = bo.count_in_boxes(cube.so, bo.grid_cells(origin, spacing, dims, fixed), threads=16)
    assert (fixed_ref[fixed >= cells - 64] > 0).any(), "the shim finds no face in the last 64 cells"

    def check(got, where):
        filled = np.flatnonzero(got["occupied"])
        if "count" in got:
            assert np.array_equal(got["occupied"] == 1, got["count"] > 0), where + ": occupied is not count > 0 on all cells"
        assert len(filled) <= 1024, "%s: %d cells are reported non-empty" % (where, len(filled))
        near = np.unique((filled[:, None] + np.arange(-64, 65)[None, :]).ravel())
        near = near[(near >= 0) & (near < cells)]
        near_ref = bo.count_in_boxes(cube.so, bo.grid_cells(origin, spacing, dims, near), threads=16)
        assert (near_ref[near < cells - 64] > 0).any(), where + ": the shim finds no face before the last 64 cells"
        for sub, ref, what in ((fixed, fixed_ref, "the fixed subset"), (near, near_ref, "the cells near a non-empty one")):
            if "count" in got:
                _eq(got["count"][sub], ref, "%s count on %s" % (where, what))
            assert np.array_equal(got["occupied"][sub] == 1, ref > 0), "%s occupied on %s" % (where, what)

    check(_grid_raw(rt, cube.handle, origin, spacing, dims, ("occupied", "count")), "count and occupied")
    check(_grid_raw(rt, cube.handle, origin, spacing, dims, ("occupied",)), "occupied alone")

# ---- B5: a partly filled last workgroup on the deep scene -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deep_queries(orc, scenes, deep):
    """Pools of rays, points (with finite radii) and triangles on the 28-level chain, each with a measure of how deep its traversal
    goes: the test oracle's node pops of the ray itself, or of the ray from the camera through the point / the triangle's centroid
    (the brute-force shims of the point and triangle families have no traversal to count)"""
    rng = np.random.default_rng(59)
    cam = np.array([0.0, -1.0, 0.0], F32)
    co, cd = ray_oracle.camera_rays(96, 64, scenes.scaled_K(96), scenes.D_REF, (0.0, -1.0, 0.0, 0.0, 0.0, 0.0))
    co, cd = np.ascontiguousarray(co.reshape(-1, 3)), np.ascontiguousarray(cd.reshape(-1, 3))
    pick = rng.choice(len(co), 1500, replace=False)
    ro, rd = np.ascontiguousarray(co[pick]), np.ascontiguousarray(cd[pick])
    pts = qp.flatten(qp.families(rng, orc.oracle(), deep.desc, deep.so, (co, cd), n=150))
    tris = np.ascontiguousarray(np.concatenate([f[1] for f in tri_families(rng, orc.oracle(), deep.desc, n=120)]), F32)
    dist = point_oracle.closest_points(deep.so, pts)["distance"]
    md = (np.where(dist < np.finfo(F32).max, dist, F32(1.0)) * rng.uniform(1.0, 3.0, len(pts))).astype(F32)

    def toward(p):
        p = np.ascontiguousarray(p, F32)
        return ray_oracle.cast_rays(deep.so, np.tile(cam, (len(p), 1)), np.ascontiguousarray(p - cam, F32))["pops"]
    out = dict(rays=((ro, rd), ray_oracle.cast_rays(deep.so, ro, rd)["pops"]), points=((pts, md), toward(pts)),
               tris=((tris,), toward(tris.mean(axis=1))))
    assert out["rays"][1].max() > 16, out["rays"][1].max()      # deeper than the stack's LDS rows
    return out


def _hardest_last(pool, n, rng):
    """n queries of a pool: the n // 2 deepest and random others, ordered by depth, so the deepest sit in the last workgroup"""
    arrays, pops = pool
    order = np.argsort(pops, kind="stable")
    hard = order[len(order) - n // 2:] if n > 1 else order[-1:]
    rest = rng.choice(order[:len(order) - len(hard)], n - len(hard), replace=False)
    idx = np.concatenate([rest, hard])
    idx = idx[np.argsort(pops[idx], kind="stable")]
    assert pops[idx[-1]] == pops.max()
    return tuple(np.ascontiguousarray(a[idx]) for a in arrays)


@pytest.mark.parametrize("n", [1, 63, 65, 129])
def test_partial_workgroup_on_the_deep_scene(deep, deep_queries, n):
    """One call of each family with n one, one below and one above the workgroup of 64, and two groups plus one, on the 28-level chain;
    the queries that visit the most nodes come last, in the partly filled group.  Every result equals the shim's bit for bit.
    What the asserts establish about depth: the tree has more than 16 levels (max_stack > 16, so the kernels run with their spill
    arrays declared) and some pool ray visits more than 16 nodes on the oracle (pops.max() > 16 in the fixture).  Neither says that a
    query's stack held more than its 17 LDS rows: test_gpu_caller_trees.py::test_the_stack_reaches_its_spill_array does that, on
    chains whose boxes cannot prune."""
    sp, so = deep.sp, deep.so
    rng = np.random.default_rng(61 + n)
    o, d = _hardest_last(deep_queries["rays"], n, rng)
    pts, md = _hardest_last(deep_queries["points"], n, rng)
    tris, = _hardest_last(deep_queries["tris"], n, rng)
    assert sp.info()["max_stack"] > 16
    exact = ("distance", "instance", "triangle", "point", "normal", "barycentric", "uv")
    got, ref = sp.closest_points(pts, outputs=exact + ("pops",)), point_oracle.closest_points(so, pts)
    for k in exact:
        _eq(got[k], ref[k], "closest_points n=%d %s" % (n, k))
    got, ref = sp.count_crossings(o, d, outputs=("count", "winding", "pops")), xo.count_crossings(so, o, d)
    for k in ("count", "winding"):
        _eq(got[k], ref[k], "count_crossings n=%d %s" % (n, k))
    _eq(sp.winding_numbers(pts), xo.winding_numbers(so, pts), "winding_numbers n=%d" % n)
    _eq(sp.signed_distance(pts, md), xo.signed_distance(so, pts, md), "signed_distance n=%d" % n)
    got, ref = sp.list_crossings(o, d), xl.list_crossings(so, o, d)
    for k in ("t", "instance", "triangle", "sign", "barycentric", "uv", "point", "offsets", "ray", "count"):
        _eq(got[k], ref[k], "list_crossings n=%d %s" % (n, k))
    got, ref = sp.list_nearby(pts, md, outputs=exact), nb.list_nearby(so, pts, md)
    for k in exact + ("offsets", "point_index", "count"):
        _eq(got[k], ref[k], "list_nearby n=%d %s" % (n, k))
    got, ref = sp.count_intersecting(tris, outputs=("count", "any", "pops")), ti.count_intersecting(so, tris)
    _eq(got["count"], ref, "count_intersecting n=%d count" % n)
    assert np.array_equal(got["any"], ref > 0), "count_intersecting n=%d any" % n
