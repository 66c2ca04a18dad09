"""Region queries without a GPU: the brute-force shim (tests/region_oracle.c) that test_gpu_regions.py compares with is pinned on
hand-made cases with power-of-two coordinates and exact answers -- inside, through a face, beyond a face, past and across a corner
that only the clip decides, a triangle that covers the region's cross-section, the closed and half-open behaviour on a face, -0,
half-spaces, slabs, empty, invalid and NaN regions, degenerate triangles --, on posed instances against world copies, against a
float64 clip on 20 000 random cases, and through the helpers that make regions from boxes, oriented boxes and frusta."""
import numpy as np
import pytest

import box_oracle
import region_oracle as ro
import scene_defs as sd
from test_crossing_host import _cube, _scene
from test_tri_intersect_host import _verts, _world_copy

F32 = np.float32
CUBE = np.array([[(0, 0, 0), (1, 0, 0)], [(1, 1, 1), (-1, 0, 0)], [(0, 0, 0), (0, 1, 0)], [(1, 1, 1), (0, -1, 0)],
                 [(0, 0, 0), (0, 0, 1)], [(1, 1, 1), (0, 0, -1)]], F32)          # the unit cube: x-lo, x-hi, y-lo, y-hi, z-lo, z-hi
PRISM = CUBE[:4]                                                                # the square prism 0 <= x, y <= 1, any z


def _pair(region, tri, pose=(0.0,) * 6):
    hit, inside, h, poly, _m = ro.pair(region, tri, pose)
    return hit, inside, h, poly.tolist()


def test_unit_cube_inside_through_a_face_and_beyond_it(rt):
    assert np.array_equal(rt.regions_from_boxes(np.array([(0, 0, 0), (1, 1, 1)], F32)), CUBE)
    tri = [(.25, .25, .25), (.75, .25, .25), (.25, .75, .5)]
    hit, inside, h, poly = _pair(CUBE, tri)
    assert hit and inside and (h > 0).all() and poly == [list(v) for v in tri]
    # through the face x = 1: the cuts are at t = 1/2 of power-of-two edges, both computed from the end outside
    a, b, c = (.5, .5, .5), (1.5, .5, .5), (.5, .75, .5)
    hit, inside, h, poly = _pair(CUBE, [a, b, c])
    assert hit and not inside and h[1].tolist() == [.5, -.5, .5]
    assert poly == [list(a), [1, .5, .5], [1, .625, .5], list(c)]
    # every rotation of the cycle gives the same polygon, rotated
    assert _pair(CUBE, [b, c, a])[3] == [[1, .625, .5], list(c), list(a), [1, .5, .5]]
    # wholly beyond the face: all three BELOW on x-hi, step 3
    hit, inside, h, poly = _pair(CUBE, [(2, 0, 0), (3, 0, 0), (2, 1, .5)])
    assert not hit and not inside and (h[1] < 0).all() and poly == []


def test_only_the_clip_rejects_a_triangle_past_a_corner():
    """No plane of the prism has the triangle wholly below it, yet its hypotenuse x + y = 3.5 passes outside the corner (1, 1); moved
    by (-1, -1) it cuts the corner off along x + y = 1.5."""
    out = np.array([(3, .5, 0), (.5, 3, 0), (3, 3, 0)], F32)
    hit, inside, h, poly = _pair(PRISM, out)
    assert ((h >= 0).any(1)).all() and not (h >= 0).all()                       # step 3 passes on every plane, step 4 does not
    assert not hit and poly == []
    hit, inside, h, poly = _pair(PRISM, out - F32((1, 1, 0)))
    assert hit and not inside
    assert sorted(poly) == sorted([[1, .5, 0], [1, 1, 0], [.5, 1, 0]])
    assert not _pair(CUBE, out + F32((0, 0, .5)))[0] and _pair(CUBE, out + F32((-1, -1, .5)))[0]


def test_large_triangle_that_contains_the_cross_section():
    tri = np.array([(-4, -4, .5), (12, -4, .5), (-4, 12, .5)], F32)
    hit, inside, h, poly = _pair(CUBE, tri)
    assert hit and not inside
    assert not ((h >= 0).all(0)).any()                                          # no vertex is inside the region
    assert len(poly) == 4
    assert sorted(tuple(round(float(x), 5) for x in v) for v in poly) == [(0, 0, .5), (0, 1, .5), (1, 0, .5), (1, 1, .5)]


def test_closed_on_a_face_and_negative_zero():
    # a vertex on the face x = 1 from outside: it is ABOVE (h = 0), so step 3 passes, and the clip keeps it
    hit, inside, h, poly = _pair(CUBE, [(1, .5, .5), (2, .25, .5), (2, .75, .5)])
    assert hit and not inside and h[1].tolist() == [0, -1, -1] and poly == [[1, .5, .5]] * len(poly) and len(poly) >= 1
    # from inside, the rest inside: wholly inside
    hit, inside, h, poly = _pair(CUBE, [(1, .5, .5), (.5, .25, .5), (.5, .75, .5)])
    assert hit and inside and h[1].tolist() == [0, .5, .5]
    # an edge in the face, the third vertex outside / inside; a triangle lying in the face
    assert _pair(CUBE, [(1, .25, .5), (1, .75, .5), (2, .5, .5)])[:2] == (True, False)
    assert _pair(CUBE, [(1, .25, .5), (1, .75, .5), (.5, .5, .5)])[:2] == (True, True)
    assert _pair(CUBE, [(1, .25, .25), (1, .75, .25), (1, .5, .75)])[:2] == (True, True)
    # just outside the face by one ulp of the height: no pair
    eps = np.nextafter(F32(1), F32(2))
    assert not _pair(CUBE, [(eps, .25, .25), (eps, .75, .25), (eps, .5, .75)])[0]
    # h = -0 at X = P under a normal with three negative components: ABOVE
    hit, inside, h, poly = _pair([[(0, 0, 0), (-1, -1, -1)]], [(0, 0, 0), (-1, 0, 0), (0, -1, 0)])
    assert h[0, 0] == 0 and np.signbit(h[0, 0]) and h[0, 1] == 1 and h[0, 2] == 1 and hit and inside


def test_half_space_slab_and_empty_region():
    up = [(0, 0, 0), (0, 0, 1)]
    above, across, below = [(0, 0, 1), (1, 0, 1), (0, 1, 2)], [(0, 0, -1), (2, 0, 1), (0, 2, 1)], [(0, 0, -1), (1, 0, -1), (0, 1, -2)]
    assert _pair([up], above)[:2] == (True, True) and _pair([up], across)[:2] == (True, False) and not _pair([up], below)[0]
    assert _pair([up], across)[3] == [[1, 0, 0], [2, 0, 1], [0, 2, 1], [0, 1, 0]]
    slab = [up, [(0, 0, 1), (0, 0, -1)]]                                        # 0 <= z <= 1
    assert _pair(slab, [(0, 0, .5), (9, 0, .5), (0, 9, 1)])[:2] == (True, True)
    assert _pair(slab, [(0, 0, -1), (0, 0, 3), (1, 0, 3)])[:2] == (True, False)
    assert not _pair(slab, [(0, 0, 2), (1, 0, 2), (0, 1, 3)])[0]
    # two half-spaces that face away from each other: z >= 1 and z <= 0; a triangle through both passes step 3 and clips to nothing
    empty = [[(0, 0, 1), (0, 0, 1)], [(0, 0, 0), (0, 0, -1)]]
    tri = [(0, 0, -1), (0, 0, 2), (1, 0, 2)]
    hit, inside, h, poly = _pair(empty, tri)
    assert ((h >= 0).any(1)).all() and not hit and poly == []
    assert not _pair(empty, [(0, 0, .5), (1, 0, .5), (0, 1, .5)])[0]


def test_invalid_and_nan_regions(orc):
    tri = [(.25, .25, .25), (.75, .25, .25), (.25, .75, .5)]
    for k in range(6):
        for zero in ((0, 0, 0), (-0.0, 0, -0.0)):
            bad = CUBE.copy()
            bad[k, 1] = zero
            hit, inside, h, poly = _pair(bad, tri)
            assert not hit and not inside and (h == 0).all(), k
    for where in ((2, 0, 1), (3, 1, 0), (0, 0, 0)):
        for v in (np.nan, np.inf, -np.inf):
            bad = CUBE.copy()
            bad[where] = v
            ro.pair(bad, tri)                                                   # unspecified, and no fault
    assert not _pair(np.full((6, 2, 3), np.nan, F32), tri)[0]
    so = _scene(orc, _cube(orc))
    try:
        whole = CUBE.copy()
        whole[:, 0] = [(-1,) * 3, (2,) * 3] * 3
        zero = CUBE.copy()
        zero[4, 1] = 0
        regions = np.stack([whole, zero, np.full((6, 2, 3), np.nan, F32), CUBE + F32([[(5, 0, 0), (0, 0, 0)]])])
        c = ro.count_in_regions(so, regions)
        assert c["count"].tolist() == [12, 0, 0, 0] and c["inside"].tolist() == [12, 0, 0, 0]
        r = ro.list_in_regions(so, regions, max_hits=3)
        assert r["count"].tolist() == [12, 0, 0, 0] and r["triangle"][0].tolist() == [0, 1, 2] and (r["inside"][0] == 1).all()
        assert (r["triangle"][1:] == -1).all() and (r["instance"][1:] == -1).all() and (r["inside"][1:] == 0).all() and (r["normal"][1:] == 0).all()
        # the cube's own faces touch the unit-cube region: closed, so all twelve are pairs, and wholly inside
        c = ro.count_in_regions(so, CUBE[None])
        assert c["count"].tolist() == [12] and c["inside"].tolist() == [12]
        # half of it: the four triangles of the far faces are out, the eight that cross x = .5 are pairs but not inside
        half = CUBE.copy()
        half[1, 0] = (.5, 0, 0)
        r = ro.list_in_regions(so, half[None])
        assert r["count"].tolist() == [10] and int(r["inside"].sum()) == 2
    finally:
        so.close()


def test_degenerate_triangles():
    assert _pair(CUBE, [(.5, .5, .5)] * 3)[:2] == (True, True) and _pair(CUBE, [(1, 1, 1)] * 3)[:2] == (True, True)
    assert not _pair(CUBE, [(2, .5, .5)] * 3)[0]
    hit, inside, _h, poly = _pair(CUBE, [(.5, .5, .5), (1.5, .5, .5), (1.5, .5, .5)])     # a segment through the face x = 1
    assert hit and not inside and [.5, .5, .5] in poly and [1, .5, .5] in poly
    assert not _pair(CUBE, [(2, .5, .5), (3, .5, .5), (3, .5, .5)])[0]
    assert _pair(CUBE, [(-1, .5, .5), (2, .5, .5), (2, .5, .5)])[:2] == (True, False)     # through the whole region, no vertex inside


def test_rooms_truncate_and_pad(orc):
    so = _scene(orc, _cube(orc))
    try:
        half = CUBE.copy()
        half[1, 0] = (.5, 0, 0)
        regions = np.stack([CUBE, CUBE + F32([[(3, 0, 0), (0, 0, 0)]]), half])
        r = ro.list_in_regions(so, regions)
        assert r["count"].tolist() == [12, 0, 10]
        for M in (1, 3, 16):
            k = ro.list_in_regions(so, regions, max_hits=M)
            assert np.array_equal(k["count"], r["count"])
            for j in range(len(regions)):
                a, b = r["offsets"][j], r["offsets"][j + 1]
                m = min(b - a, M)
                for f in ro.FIELDS:
                    assert np.array_equal(k[f][j, :m], r[f][a:a + m]), (M, j, f)
                assert (k["instance"][j, m:] == -1).all() and (k["triangle"][j, m:] == -1).all()
                assert (k["inside"][j, m:] == 0).all() and (k["normal"][j, m:] == 0).all()
    finally:
        so.close()


# ---- float64 --------------------------------------------------------------------------------------------------------------------

def _clip64(tri, p, n, off):
    """the triangle clipped by the planes h_k(X) + off_k >= 0 in float64 (python floats) -> whether anything is left"""
    poly = tri
    for k in range(len(p)):
        pk, nk = p[k], n[k]
        g = [nk[0] * (v[0] - pk[0]) + nk[1] * (v[1] - pk[1]) + nk[2] * (v[2] - pk[2]) + off[k] for v in poly]
        out, m = [], len(poly)
        for i in range(m):
            j = (i + 1) % m
            if g[i] >= 0:
                out.append(poly[i])
            if (g[i] >= 0) != (g[j] >= 0):
                t = g[i] / (g[i] - g[j])
                out.append([poly[i][c] + t * (poly[j][c] - poly[i][c]) for c in range(3)])
        poly = out
        if not poly:
            return False
    return True


def _verdict64(tri, mapped):
    """float64 on the mapped planes and the triangle as the shim saw them -> (decisive, pair, clear, inside): the region grown by delta
    still misses or shrunk by delta still hits; every |height| exceeds delta, and then whether all are above"""
    p64, n64, t64 = mapped[:, 0].astype(np.float64), mapped[:, 1].astype(np.float64), np.asarray(tri, np.float64)
    M = max(np.abs(t64).max(), np.abs(p64).max())
    delta = 1e-4 * np.abs(n64).sum(1) * M
    p, n, t = p64.tolist(), n64.tolist(), t64.tolist()
    grown, shrunk = _clip64(t, p, n, delta.tolist()), _clip64(t, p, n, (-delta).tolist())
    h = np.einsum("kc,kvc->kv", n64, t64[None] - p64[:, None])
    clear = bool((np.abs(h) > delta[:, None]).all())
    return (not grown) or shrunk, shrunk, clear, bool((h >= 0).all())


def _random_obb(rng, extent, lo=-2.0, hi=0.0):
    """an oriented box of 10^lo..10^hi of the extent somewhere in it, its six planes' normals scaled by 1e-1..1e1 -> (region, size)"""
    size = extent * 10.0 ** rng.uniform(lo, hi)
    q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
    c = rng.uniform(-0.5, 0.5, 3) * extent
    half = 0.5 * size * rng.uniform(0.5, 1.0, 3)
    planes = []
    for a in range(3):
        for sgn in (-1.0, 1.0):
            planes.append([c + sgn * half[a] * q[a], -sgn * q[a] * 10.0 ** rng.uniform(-1, 1)])
    return np.array(planes, F32), size


def test_agrees_with_float64_clip():
    """20 000 random posed oriented boxes of 1e-2 to 1 of the extent (10), normals scaled by 1e-1 to 1e1, against a triangle of like
    size nearby, in mesh space.  With p'_k and n'_k as the shim mapped them, in float64, delta_k = 1e-4 |n'_k|_1 M (M the largest
    coordinate magnitude of the case; fp32 heights err by about 4u |n'_k|_1 M with u = 2^-24, and a cut point moves by a few u M, a
    thousand times less): the pair decision agrees wherever the region grown by delta still misses or shrunk by delta still hits, and
    inside agrees wherever every |height| exceeds delta."""
    rng = np.random.default_rng(15)
    n, extent = 20000, 10.0
    undecided = pairs = insides = checked_inside = 0
    for j in range(n):
        pose = np.concatenate([rng.uniform(-2, 2, 3), rng.uniform(-np.pi, np.pi, 3)]).astype(F32)
        region, size = _random_obb(rng, extent)
        mapped = ro.pair(region, np.zeros((3, 3), F32), pose)[4]
        centre = mapped[:, 0].astype(np.float64).mean(0)
        tri = (centre + rng.normal(size=3) * size * rng.uniform(0, 1.0) + rng.normal(size=(3, 3)) * 0.4 * size).astype(F32)
        hit, inside, _h, _poly, mapped = ro.pair(region, tri, pose)
        decisive, want, clear, want_inside = _verdict64(tri, mapped)
        if decisive:
            assert hit == want, (j, hit, want)
            pairs += int(hit)
        else:
            undecided += 1
        if clear:
            assert inside == want_inside, (j, inside, want_inside)
            checked_inside += 1
            insides += int(inside)
    print("undecided %d, pairs %d, inside %d of %d clear, of %d" % (undecided, pairs, insides, checked_inside, n))
    assert undecided <= 0.02 * n, undecided
    assert pairs >= 0.05 * n and (n - undecided - pairs) >= 0.05 * n, (pairs, undecided)
    assert insides >= 100 and checked_inside >= 0.9 * n


@pytest.mark.parametrize("pose,scale", [((0.3, -0.2, 0.5, 0.4, -0.3, 0.2), (1.5, 0.7, 1.2)),
                                        ((-0.1, 0.4, 0.0, -0.6, 0.1, 0.9), (1.0, -1.3, 0.8))])
def test_posed_scaled_mirrored_instance_matches_world_copy(orc, pose, scale):
    """A posed, non-uniformly scaled (and mirrored) instance of a mesh and the same triangles placed in world space as an identity
    instance: the same pairs and the same inside flags wherever the float64 clip of the world triangle by the world planes is
    decisive (delta = 1e-4 |N_k|_1 times the largest coordinate, 3)."""
    tris = sd.random_triangles(60, seed=3, spread=1.0, size=0.4)
    a = _scene(orc, tris, [(0, 0, tuple(pose), tuple(scale))])
    b = _scene(orc, _world_copy(orc, tris, pose, scale))
    try:
        world = _verts(orc, _world_copy(orc, tris, pose, scale))
        rng = np.random.default_rng(9)
        regions = np.stack([_random_obb(rng, 3.0, -1.0, 0.0)[0] for _ in range(200)])
        ra, rb = ro.list_in_regions(a, regions), ro.list_in_regions(b, regions)
        agreed = agreed_inside = 0
        for j in range(len(regions)):
            got = []
            for r in (ra, rb):
                s0, s1 = r["offsets"][j], r["offsets"][j + 1]
                flag = np.full(len(world), -1)
                flag[r["triangle"][s0:s1]] = r["inside"][s0:s1]
                got.append(flag)
            for t in range(len(world)):
                decisive, want, clear, want_inside = _verdict64(world[t], regions[j])
                if decisive:
                    assert (got[0][t] >= 0) == (got[1][t] >= 0) == want, (j, t)
                    agreed += int(want)
                if clear:
                    assert (got[0][t] == 1) == (got[1][t] == 1) == want_inside, (j, t)
                    agreed_inside += int(want_inside)
        assert agreed > 200 and agreed_inside > 20, (agreed, agreed_inside)
    finally:
        a.close()
        b.close()


# ---- helpers --------------------------------------------------------------------------------------------------------------------

def _heights64(region, x):
    r = np.asarray(region, np.float64)
    return np.einsum("...kc,...kc->...k", r[..., 1, :], np.asarray(x, np.float64)[..., None, :] - r[..., 0, :])


def test_helpers_make_regions_with_inward_normals(rt):
    rng = np.random.default_rng(4)
    n = 200
    lo = rng.uniform(-5, 5, (n, 3)).astype(F32)
    ext = rng.uniform(0.1, 3, (n, 3)).astype(F32)
    boxes = np.stack([lo, lo + ext], 1)
    rb = rt.regions_from_boxes(boxes)
    assert rb.shape == (n, 6, 2, 3) and rb.dtype == F32
    assert np.array_equal(rb[:, 0::2, 0], np.repeat(lo[:, None], 3, 1)) and np.array_equal(rb[:, 1::2, 0], np.repeat(boxes[:, 1, None], 3, 1))
    assert (_heights64(rb, lo + 0.5 * ext) > 0).all()
    for a in range(3):
        for s in (-0.25, 1.25):
            x = lo + 0.5 * ext
            x[:, a] = lo[:, a] + s * ext[:, a]
            assert ((_heights64(rb, x) < 0).sum(1) == 1).all()
    # oriented boxes
    q = np.stack([np.linalg.qr(rng.normal(size=(3, 3)))[0] for _ in range(n)]).astype(F32)
    c = rng.uniform(-5, 5, (n, 3)).astype(F32)
    half = rng.uniform(0.1, 2, (n, 3)).astype(F32)
    rob = rt.regions_from_obbs(c, q, half)
    assert rob.shape == (n, 6, 2, 3) and rob.dtype == F32
    local = rng.uniform(-0.9, 0.9, (n, 3))
    assert (_heights64(rob, c + np.einsum("na,nac->nc", local * half, q)) > 0).all()
    for a in range(3):
        out = local.copy()
        out[:, a] = rng.choice([-1.2, 1.2], n)
        assert ((_heights64(rob, c + np.einsum("na,nac->nc", out * half, q)) < 0).sum(1) == 1).all()
    # frusta: a camera at `eye` looking along -z of its own frame, corners counter-clockwise seen from the eye
    eye = rng.uniform(-5, 5, (n, 3)).astype(F32)
    tan = rng.uniform(0.2, 1.0, (n, 2))
    cam = np.stack([(tan[:, 0], -tan[:, 1], -np.ones(n)), (tan[:, 0], tan[:, 1], -np.ones(n)), (-tan[:, 0], tan[:, 1], -np.ones(n)),
                    (-tan[:, 0], -tan[:, 1], -np.ones(n))], 0).transpose(2, 0, 1)                   # [n, 4, 3]
    corners = (eye[:, None] + np.einsum("nkc,ncd->nkd", cam, q)).astype(F32)
    near, far = F32(0.5), rng.uniform(2, 9, n).astype(F32)
    rf = rt.regions_from_frusta(eye, corners, near, far)
    assert rf.shape == (n, 6, 2, 3) and rf.dtype == F32
    axis = -q[:, 2].astype(np.float64)                                          # the mean direction
    uv = rng.uniform(-0.9, 0.9, (n, 2)) * tan
    depth = rng.uniform(0.6, 0.95, n) * (far - 0.5) + 0.5                        # (between the caps)
    ray = np.einsum("nc,ncd->nd", np.stack([uv[:, 0], uv[:, 1], -np.ones(n)], 1), q)
    assert (_heights64(rf, eye + ray * depth[:, None]) > 0).all()
    assert (_heights64(rf, eye + ray * 0.4)[:, 4] < 0).all() and (_heights64(rf, eye + ray * (far * 1.1)[:, None])[:, 5] < 0).all()
    assert (_heights64(rf, eye - axis) < 0).any(1).all()
    wide = np.einsum("nc,ncd->nd", np.stack([1.5 * tan[:, 0], uv[:, 1], -np.ones(n)], 1), q)
    h = _heights64(rf, eye + wide * depth[:, None])
    assert (h[:, 0] < 0).all() and (np.delete(h, 0, 1)[:, :3] > 0).all()        # past the side between corners 0 and 1 alone
    assert np.array_equal(rt.regions_from_frusta(eye, corners, np.full(n, near), far), rf)
    assert np.array_equal(rt.regions_from_frusta(eye, corners, 0.5, far), rf)
    # torch in, torch out, the same numbers
    torch = pytest.importorskip("torch")
    tb = rt.regions_from_boxes(torch.from_numpy(boxes))
    assert isinstance(tb, torch.Tensor) and np.array_equal(tb.numpy(), rb)
    to = rt.regions_from_obbs(torch.from_numpy(c), torch.from_numpy(q), torch.from_numpy(half))
    assert isinstance(to, torch.Tensor) and to.dtype == torch.float32 and np.allclose(to.numpy(), rob, rtol=0, atol=1e-6)
    tf = rt.regions_from_frusta(torch.from_numpy(eye), torch.from_numpy(corners), 0.5, torch.from_numpy(far))
    assert isinstance(tf, torch.Tensor) and tf.dtype == torch.float32 and np.allclose(tf.numpy(), rf, rtol=1e-5, atol=1e-5)


def test_box_regions_agree_with_the_box_rule(rt, orc):
    """Triangles and boxes with small integer coordinates: regions_from_boxes through this shim and rule 11 through box_oracle name the
    same pairs wherever the float64 clip calls the pair decisive (touching pairs are not: both rules are closed, and they are
    compared there too, as a count that is printed)."""
    o = orc.oracle()
    rng = np.random.default_rng(21)
    v = rng.integers(-4, 5, (300, 3, 3)).astype(F32)
    tris = np.stack([np.asarray(o.tri_from_vertices(x.ravel()), F32) for x in v])
    so = _scene(orc, tris)
    try:
        lo = rng.integers(-4, 3, (150, 3))
        boxes = np.stack([lo, lo + rng.integers(1, 4, (150, 3))], 1).astype(F32)
        regions = rt.regions_from_boxes(boxes)
        rr, rb = ro.list_in_regions(so, regions), box_oracle.list_in_boxes(so, boxes)
        decisive_pairs = differing = 0
        for j in range(len(boxes)):
            a = set(rr["triangle"][rr["offsets"][j]:rr["offsets"][j + 1]].tolist())
            b = set(rb["triangle"][rb["offsets"][j]:rb["offsets"][j + 1]].tolist())
            for t in range(len(v)):
                decisive, want, _c, _i = _verdict64(v[t], regions[j])
                if decisive:
                    assert (t in a) == (t in b) == want, (j, t)
                    decisive_pairs += int(want)
                else:
                    differing += int((t in a) != (t in b))
        print("decisive pairs %d, touching pairs on which the two rules differ %d" % (decisive_pairs, differing))
        assert decisive_pairs > 1000
    finally:
        so.close()
