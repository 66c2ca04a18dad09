"""Segment queries without a GPU: the brute-force shim (tests/segment_oracle.c) that the GPU tests compare with is pinned on hand-made
cases with exact answers, on degenerate input, against the same triangles placed in world space and against float64; the C-ABI and
the Python wrapper reject bad arguments before they touch a device (the GPU side: test_gpu_segments.py)."""
import ctypes as C

import numpy as np
import pytest

import crossing_oracle
import point_oracle
import scene_defs as sd
import segment_oracle

F32 = np.float32
FLT_MAX = np.finfo(F32).max
A, AB, AC = np.zeros(3, F32), np.array([2, 0, 0], F32), np.array([0, 2, 0], F32)
# The shim's worst distance error against float64 over the 20 000 cases of test_shim_against_float64, relative to the largest
# coordinate magnitude of the case, as measured with this seed; the test asserts four times that: the margin
# is for other seeds, since near-parallel pairs lose digits in den.
MEASURED_REL_ERROR = 2.27e-7


def _scene(orc, tris, instances):
    return sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", tris)], instances).build_oracle(orc)


def _tris(orc, verts):
    o = orc.oracle()
    out = np.stack([o.tri_from_vertices(np.asarray(v, F32).ravel()) for v in verts])
    out[:, 12:18] = [0, 0, 1, 0, 0, 1]
    return out


def test_five_candidates_and_the_tie_order(orc):
    """Power-of-two cases with exact answers on the triangle (0,0,0) (2,0,0) (0,2,0): each of the five candidates wins where it
    should, with its s, weights and d2; among equal candidates the first in the order (a)..(e) wins."""
    cases = [
        # q0, q1 -> which, s, b1, b2, d2
        ((0.5, 0.5, 1), (0.5, 0.5, 3), 0, 0.0, 0.25, 0.25, 1.0),          # (a): the end Q0 above the face
        ((0.5, 0.5, 3), (0.5, 0.5, 1), 1, 1.0, 0.25, 0.25, 1.0),          # (b): the end Q1
        ((1, -1, -1), (1, -1, 1), 2, 0.5, 0.5, 0.0, 1.0),                 # (c): passing the edge AB's line outside the triangle
        ((-1, 1, -1), (-1, 1, 1), 3, 0.5, 0.0, 0.5, 1.0),                 # (d): the edge AC
        ((2, 2, -1), (2, 2, 1), 4, 0.5, 0.5, 0.5, 2.0),                   # (e): the edge BC
        ((1, -1, -1), (1, 1, 1), 2, 0.5, 0.5, 0.0, 0.0),                  # crossing the edge AB's line in projection: touches it
        ((0.5, -1, 0), (1.5, -1, 0), 0, 0.0, 0.25, 0.0, 1.0),             # parallel to the edge AB: (a), (b), (c) tie, (a) wins
        ((1.5, -1, 0), (0.5, -1, 0), 0, 0.0, 0.75, 0.0, 1.0),             # the same, reversed
        ((0.5, 0.5, 1), (1, 0.5, 1), 0, 0.0, 0.25, 0.25, 1.0),            # parallel to the face above it: (a) and (b) tie
        ((-1, -1, 0), (-1, -1, 0), 0, 0.0, 0.0, 0.0, 2.0),                # zero length: the point query
    ]
    for q0, q1, which, s, b1, b2, d2 in cases:
        got = segment_oracle.on_triangle(np.array(q0, F32), np.array(q1, F32), A, AB, AC)
        assert got == (F32(s), F32(b1), F32(b2), F32(d2), which), (q0, q1, got)
    # step 4 alone: parallel segments (den = 0) start from s = 0 and clamp from there
    assert segment_oracle.segment_segment((0, 1, 0), (4, 0, 0), (1, 0, 0), (2, 0, 0)) == (F32(0.25), F32(0.0))
    assert segment_oracle.segment_segment((2, 1, 0), (4, 0, 0), (1, 0, 0), (2, 0, 0)) == (F32(0.0), F32(0.5))
    assert segment_oracle.segment_segment((8, 1, 0), (4, 0, 0), (1, 0, 0), (2, 0, 0)) == (F32(0.0), F32(1.0))
    assert segment_oracle.segment_segment((0, -2, 1), (0, 4, 0), (-1, 0, 0), (4, 0, 0)) == (F32(0.5), F32(0.25))
    assert segment_oracle.segment_segment((0, -2, 1), (0, 4, 0), (1, 0, 0), (4, 0, 0)) == (F32(0.5), F32(0.0))     # u < 0 -> 0
    assert segment_oracle.segment_segment((0, -2, 1), (0, 4, 0), (-8, 0, 0), (4, 0, 0)) == (F32(0.5), F32(1.0))    # u > 1 -> 1
    assert segment_oracle.segment_segment((0, 0, 0), (0, 0, 0), (-1, 1, 0), (4, 0, 0)) == (F32(0.0), F32(0.25))    # a point
    assert segment_oracle.segment_segment((0, -2, 1), (0, 4, 0), (0, 0, 0), (0, 0, 0)) == (F32(0.5), F32(0.0))     # a point edge
    assert segment_oracle.segment_segment((1, 1, 1), (0, 0, 0), (0, 0, 0), (0, 0, 0)) == (F32(0.0), F32(0.0))


def test_zero_length_segment_is_the_point_query(orc):
    """P0 == P1: every field the two shims share is the same bits, over posed, scaled and mirrored instances and under a bound."""
    tris = sd.random_triangles(60, seed=11, spread=1.0, size=0.5)
    instances = [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (0, 0, (0.3, -0.2, 0.5, 0.4, -0.7, 1.1), (1.5, -0.5, 2.0)),
                 (0, 0, (-1.0, 0.5, 0.0, 0.0, 3.0, -0.2), (-1.0, -1.0, 0.25))]
    so = _scene(orc, tris, instances)
    try:
        rng = np.random.default_rng(3)
        pts = rng.uniform(-3, 3, (300, 3)).astype(F32)
        segs = np.ascontiguousarray(np.stack([pts, pts], axis=1))
        for md in (None, rng.uniform(0.1, 1.5, 300).astype(F32)):
            got, ref = segment_oracle.closest_to_segments(so, segs, md), point_oracle.closest_points(so, pts, md)
            for k in point_oracle.OUTPUTS:
                assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
            assert (got["parameter"] == 0).all() and (got["crossings"] == 0).all()
            assert (got["which"][got["instance"] >= 0] == 0).all()
            assert np.array_equal(got["clearance"], got["distance"]) and np.array_equal(got["within"], got["instance"] >= 0)
    finally:
        so.close()


def test_degenerate_triangles_are_finite(orc):
    """Zero-area, collinear, repeated-vertex, single-point and needle triangles never divide by zero: s and the weights finite and in
    [0, 1], and the distance within 1e-5 of the float64 distance between the segment and the triangle's (degenerate) edges."""
    rng = np.random.default_rng(1)
    for _ in range(300):
        a, b = rng.uniform(-1, 1, (2, 3)).astype(F32)
        kind = int(rng.integers(5))
        c = {0: a, 1: (a + F32(rng.choice([2.0, 0.5, -1.0])) * (b - a)).astype(F32), 2: b,
             3: (a + F32(0.4) * (b - a) + rng.uniform(-1, 1, 3).astype(F32) * F32(1e-6)).astype(F32), 4: a}[kind]
        if kind in (0, 4):
            b = a if kind == 4 else b
        q0, q1 = rng.uniform(-2, 2, (2, 3)).astype(F32)
        if rng.random() < 0.2:
            q1 = q0
        s, b1, b2, d2, which = segment_oracle.on_triangle(q0, q1, a, (b - a).astype(F32), (c - a).astype(F32))
        assert np.isfinite([s, b1, b2, d2]).all() and 0 <= s <= 1 and 0 <= b1 <= 1 and 0 <= b2 <= 1 and b1 + b2 <= 1 + 1e-6
        want = _segment_triangle64(*(np.asarray(v, np.float64)[None] for v in (q0, q1, a, b, c)))[0]
        assert abs(np.sqrt(np.float64(d2)) - want) <= 1e-5 * max(1.0, want), (a, b, c, q0, q1)


def test_piercing_is_reported_by_the_crossing_half(orc):
    """A segment through the middle of a large triangle: every candidate of the minimum is far away, so under a small radius the
    distance is a miss, and the crossing half says crossings == 1, clearance == 0, within == 1."""
    so = _scene(orc, _tris(orc, [[-8, -8, 0, 8, -8, 0, 0, 8, 0]]), [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    try:
        segs = np.array([[[0, 0, -1], [0, 0, 1]], [[0, 0, 1], [0, 0, 3]], [[0, 0, 1], [0, 0, 0]]], F32)
        got = segment_oracle.closest_to_segments(so, segs, np.full(3, 0.25, F32))
        assert got["distance"].tolist() == [FLT_MAX, FLT_MAX, 0.0] and got["instance"].tolist() == [-1, -1, 0]
        assert got["crossings"].tolist() == [1, 0, 1] and got["clearance"].tolist() == [0.0, FLT_MAX, 0.0]
        assert got["within"].tolist() == [1, 0, 1]
        assert not got["point"][:2].any() and not got["segment_point"][:2].any() and got["parameter"].tolist() == [0.0, 0.0, 1.0]
        free = segment_oracle.closest_to_segments(so, segs)
        assert free["distance"].tolist() == [1.0, 1.0, 0.0] and free["clearance"].tolist() == [0.0, 1.0, 0.0]
        assert free["within"].tolist() == [1, 1, 1] and free["which"].tolist() == [0, 0, 1]
        cc = crossing_oracle.count_crossings(so, segs[:, 0], segs[:, 1] - segs[:, 0], np.ones(3, F32))["count"]
        assert np.array_equal(cc, got["crossings"])
    finally:
        so.close()


def test_posed_instances_against_world_space_triangles(orc):
    """Rotated, translated, non-uniformly scaled and mirrored instances against the same triangles placed in world space under an
    identity instance: the same distances and nearest pairs to rounding, the same winners away from ties, the same crossings."""
    o = orc.oracle()
    tris = sd.random_triangles(40, seed=5, spread=1.0, size=0.5)
    instances = [(0, 0, (0.3, -0.2, 0.5, 0.4, -0.7, 1.1), (1.5, -0.5, 2.0)), (0, 0, (-1.0, 0.5, 0.0, 0.0, 3.0, -0.2), (-1.0, -1.0, 0.25)),
                 (0, 0, (0.5, 0.5, -0.5, 1.0, 0.2, 0.3), (0.5, 2.0, 1.0))]
    posed = _scene(orc, tris, instances)
    world = []
    for _m, _mat, pose, scale in instances:
        inv = o.invert_lre(np.asarray(pose, F32))
        v = tris[:, :9].reshape(-1, 3) * np.asarray(scale, F32)
        world.append(np.stack([o.apply_lre(inv, x.astype(F32)) for x in v]).reshape(-1, 9))
    flat = _scene(orc, _tris(orc, np.concatenate(world)), [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    try:
        rng = np.random.default_rng(8)
        p0 = rng.uniform(-3, 3, (400, 3))
        segs = np.ascontiguousarray(np.stack([p0, p0 + rng.normal(size=(400, 3)) * rng.choice([0.01, 0.3, 2.0], (400, 1))], axis=1), F32)
        a, b = segment_oracle.closest_to_segments(posed, segs), segment_oracle.closest_to_segments(flat, segs)
        assert np.abs(a["distance"] - b["distance"]).max() <= 2e-5
        assert np.array_equal(a["crossings"], b["crossings"]) and (a["crossings"] > 0).sum() >= 10
        same = a["instance"] * 40 + a["triangle"] == b["triangle"]
        assert same.mean() > 0.95
        assert np.abs(a["segment_point"] - b["segment_point"])[same].max() <= 1e-3
        assert np.abs(a["point"] - b["point"])[same].max() <= 1e-3
        # the nearest pair is at the distance, in world space
        gap = np.linalg.norm(a["segment_point"].astype(np.float64) - a["point"], axis=1)
        assert np.abs(gap - a["distance"]).max() <= 2e-5
    finally:
        posed.close()
        flat.close()


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(axis=-1)


def _point_segment64(p, x, d):
    """distance of points p to the segments x + t d, t in [0, 1] (float64, [..., 3])"""
    dd = _dot(d, d)
    t = np.clip(np.where(dd > 0, _dot(p - x, d) / np.where(dd > 0, dd, 1.0), 0.0), 0.0, 1.0)
    return np.linalg.norm(p - (x + t[..., None] * d), axis=-1)


def _point_triangle64(p, a, b, c):
    """distance of points p to the triangles (a, b, c): the face where the projection falls inside it, else the nearest edge"""
    best = np.minimum(np.minimum(_point_segment64(p, a, b - a), _point_segment64(p, a, c - a)), _point_segment64(p, b, c - b))
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    ok = nn > 0
    h = _dot(p - a, n) / np.where(ok, nn, 1.0)
    f = p - h[..., None] * n
    inside = ok
    for x, y in ((a, b), (b, c), (c, a)):
        inside = inside & (_dot(np.cross(y - x, f - x), n) >= 0)
    return np.where(inside, np.minimum(best, np.abs(h) * np.sqrt(nn)), best)


def _segment_segment64(p, d, x, f):
    """distance between the segments p + s d and x + u f, solved exactly: the interior stationary point where there is one in
    (0, 1)^2, else one of the four end-to-segment distances"""
    best = np.minimum(np.minimum(_point_segment64(p, x, f), _point_segment64(p + d, x, f)),
                      np.minimum(_point_segment64(x, p, d), _point_segment64(x + f, p, d)))
    r = p - x
    a, e, b, c, ff = _dot(d, d), _dot(f, f), _dot(d, f), _dot(d, r), _dot(f, r)
    den = a * e - b * b
    ok = den > 1e-30 * a * e
    s = np.where(ok, (b * ff - c * e) / np.where(ok, den, 1.0), -1.0)
    u = np.where(ok, (a * ff - b * c) / np.where(ok, den, 1.0), -1.0)
    inner = ok & (s > 0) & (s < 1) & (u > 0) & (u < 1)
    gap = np.linalg.norm((p + s[..., None] * d) - (x + u[..., None] * f), axis=-1)
    return np.where(inner, np.minimum(best, gap), best)


def _segment_triangle64(q0, q1, a, b, c):
    """the float64 minimum over rule 13's five candidates: both ends against the triangle, the segment against each edge"""
    d = q1 - q0
    ends = np.minimum(_point_triangle64(q0, a, b, c), _point_triangle64(q1, a, b, c))
    edges = np.minimum(np.minimum(_segment_segment64(q0, d, a, b - a), _segment_segment64(q0, d, a, c - a)),
                       _segment_segment64(q0, d, b, c - b))
    return np.minimum(ends, edges)


def _float64_cases(orc, n=20000, seed=13):
    """n random posed (segment, triangle) cases in scaled mesh space, as the rule sees them (fp32), a tenth of them with the segment
    nearly parallel to an edge: q0, q1, a, ab, ac [n, 3] float32"""
    o = orc.oracle()
    rng = np.random.default_rng(seed)
    poses = [np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-3.1, 3.1, 3)]).astype(F32) for _ in range(8)]
    scales = np.array([(1, 1, 1), (1.5, -0.5, 2.0), (-1, -1, 0.25), (0.5, 2, 1), (1, 1, 1), (3, 3, 3), (-2, 1, 1), (0.1, 0.1, 0.1)], F32)
    v = (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3)) * rng.choice([0.05, 0.5, 1.0], (n, 1, 1))).astype(F32)
    which = rng.integers(0, 8, n)
    sc = scales[which]
    a, ab, ac = v[:, 0] * sc, (v[:, 1] - v[:, 0]) * sc, (v[:, 2] - v[:, 0]) * sc
    p0 = rng.uniform(-2, 2, (n, 3))
    p1 = p0 + rng.normal(size=(n, 3)) * rng.choice([1e-3, 0.05, 0.5, 3.0], (n, 1))
    q = np.zeros((n, 2, 3), F32)
    # world segments through the instance map; the nearly parallel ones are made in mesh space, beside the edge AB
    for j in range(n):
        q[j, 0] = o.apply_lre(poses[which[j]], p0[j].astype(F32))
        q[j, 1] = o.apply_lre(poses[which[j]], p1[j].astype(F32))
    par = rng.random(n) < 0.1
    off = rng.normal(size=(n, 3)) * 0.3
    q[par, 0] = (a + ab * rng.uniform(-0.5, 1.0, (n, 1)) + off)[par]
    q[par, 1] = (q[:, 0] + ab * rng.uniform(0.2, 2.0, (n, 1)) + rng.normal(size=(n, 3)) * rng.choice([0, 1e-6, 1e-4], (n, 1)))[par]
    return q[:, 0].copy(), q[:, 1].copy(), a.astype(F32), ab.astype(F32), ac.astype(F32)


def _shim_on_cases(cases):
    out = np.array([segment_oracle.on_triangle(*(c[j] for c in cases))[:4] for j in range(len(cases[0]))], F32)
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3]


def test_shim_against_float64(orc):
    """20 000 random posed cases: the shim's distance against (1) the float64 minimum over the same five candidates, solved exactly,
    within 4 x MEASURED_REL_ERROR of the largest coordinate magnitude involved, and (2) independently, a dense float64 sampling of
    the segment against the triangle, which is never closer than the shim by more than that error, nor farther than half a sampling
    step along the segment.  The winner's s and weights reproduce the distance."""
    cases = _float64_cases(orc)
    s, b1, b2, d2 = _shim_on_cases(cases)
    q0, q1, a, ab, ac = (c.astype(np.float64) for c in cases)
    b, c = a + ab, a + ac
    dist = np.sqrt(d2.astype(np.float64))
    assert np.isfinite(dist).all() and (s >= 0).all() and (s <= 1).all()
    mag = np.max(np.abs(np.concatenate([q0, q1, a, b, c], axis=1)), axis=1)
    exact = _segment_triangle64(q0, q1, a, b, c)
    rel = np.abs(dist - exact) / mag
    print("worst relative error %.3g (asserted: %.3g), mean %.3g" % (rel.max(), 4 * MEASURED_REL_ERROR, rel.mean()))
    assert rel.max() <= 4 * MEASURED_REL_ERROR, (rel.max(), int(rel.argmax()))
    # the pair the shim names is at the shim's distance
    x = q0 + s[:, None].astype(np.float64) * (q1 - q0)
    y = a + b1[:, None].astype(np.float64) * ab + b2[:, None].astype(np.float64) * ac
    assert (np.abs(np.linalg.norm(x - y, axis=1) - dist) / mag).max() <= 4 * MEASURED_REL_ERROR
    # dense sampling: 129 points of the segment against the triangle
    K = 128
    t = np.linspace(0.0, 1.0, K + 1)[None, :, None]
    sampled = np.full(len(dist), np.inf)
    for lo in range(0, len(dist), 2000):
        sl = slice(lo, lo + 2000)
        p = q0[sl, None] + t * (q1 - q0)[sl, None]
        sampled[sl] = _point_triangle64(p, a[sl, None], b[sl, None], c[sl, None]).min(axis=1)
    step = np.linalg.norm(q1 - q0, axis=1) / K
    tol = 4 * MEASURED_REL_ERROR * mag
    # where the segment pierces the face the five candidates are not the minimum (rule 13 step 6 leaves that to the crossing half):
    # those cases are told apart in float64 and only bounded from above
    n = np.cross(ab, ac)
    h0, h1 = _dot(q0 - a, n), _dot(q1 - a, n)
    cut = (h0 * h1 < 0)
    w = q0 + (h0 / np.where(cut, h0 - h1, 1.0))[:, None] * (q1 - q0)
    pierce = cut
    for x, y in ((a, b), (b, c), (c, a)):
        pierce = pierce & (_dot(np.cross(y - x, w - x), n) > 0)
    assert 10 <= pierce.sum() < len(dist) // 2
    assert (sampled <= dist + step / 2 + tol).all(), "no sample of the segment is as close as the shim's answer"
    assert (sampled >= dist - tol)[~pierce].all(), "a sample of the segment is closer than the shim's answer"


def test_max_distance_is_inclusive(orc):
    """The capsule's radius: the exact distance is within, its float predecessor is not (unless the segment pierces); +inf is; NaN
    and negative radii are not (the distance then FLT_MAX), and crossings do not depend on the radius."""
    so = _scene(orc, sd.random_triangles(30, seed=6, spread=1.0, size=0.4), [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))])
    try:
        rng = np.random.default_rng(7)
        p0 = rng.uniform(-2, 2, (100, 3))
        segs = np.ascontiguousarray(np.stack([p0, p0 + rng.normal(size=(100, 3)) * 0.4], axis=1), F32)
        free = segment_oracle.closest_to_segments(so, segs)
        d = free["distance"]
        assert (d > 0).all()
        for md, want in ((d, True), (np.nextafter(d, F32(0)), False), (np.full(100, np.inf, F32), True),
                         (np.full(100, np.nan, F32), False), (np.full(100, -1.0, F32), False), (np.zeros(100, F32), False)):
            got = segment_oracle.closest_to_segments(so, segs, np.asarray(md, F32))
            assert ((got["instance"] >= 0) == want).all()
            assert np.array_equal(got["crossings"], free["crossings"])
            assert np.array_equal(got["within"], ((got["instance"] >= 0) | (got["crossings"] > 0)).astype(np.int32))
            assert np.array_equal(got["clearance"], np.where(got["crossings"] > 0, F32(0), got["distance"]))
            if not want:
                assert (got["distance"] == FLT_MAX).all() and (got["triangle"] == -1).all() and not got["point"].any()
    finally:
        so.close()


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    """librt_hip.so exports rt_closest_to_segments; it refuses a NULL scene, n < 0, NULL segments and no output before touching the
    scene, and n == 0 returns at once."""
    h = rt.libs()[0]
    assert hasattr(h, "rt_closest_to_segments") and "rt_closest_to_segments" in rt.RT_HIP_SYMBOLS
    hits = rt.RtSegmentHits()
    out = C.c_void_p(64)
    with_out = rt.RtSegmentHits(within=out)
    assert h.rt_closest_to_segments(None, C.c_void_p(64), None, 3, C.byref(with_out), None, 0) == -1
    bogus = C.c_void_p(16)                                        # a handle that is never dereferenced
    assert h.rt_closest_to_segments(bogus, C.c_void_p(64), None, -1, C.byref(with_out), None, 0) == -1
    assert h.rt_closest_to_segments(bogus, None, None, 3, C.byref(with_out), None, 0) == -1
    assert h.rt_closest_to_segments(bogus, C.c_void_p(64), None, 3, C.byref(hits), None, 0) == -1
    assert h.rt_closest_to_segments(bogus, C.c_void_p(64), None, 3, None, None, 0) == -1
    assert h.rt_closest_to_segments(bogus, None, None, 0, None, None, 0) == 0
    assert [f[0] for f in rt.RtSegmentHits._fields_] == list(rt.Scene.SEGMENT_OUTPUTS)
    assert h.rt_abi_version() == 2


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    p = np.zeros((10, 2, 3), F32)
    for bad in (p.astype(np.float64), p[:, :, :2].copy(), p[:, :1].copy(), np.zeros((10, 3), F32), np.zeros((3, 2, 10), F32).T,
                p.reshape(-1), [[[0, 0, 0]] * 2] * 10):
        with pytest.raises(ValueError):
            s.closest_to_segments(bad)
    for md in (np.zeros(9, F32), np.zeros(10, np.float64), np.zeros((10, 1), F32), np.zeros((10, 2), F32)):
        with pytest.raises(ValueError):
            s.closest_to_segments(p, md)
    for outs in (("distance", "colour"), (), ("t",), ("count",)):
        with pytest.raises(ValueError):
            s.closest_to_segments(p, outputs=outs)
    torch = pytest.importorskip("torch")
    t = torch.zeros((10, 2, 3), dtype=torch.float32)
    for a, md in ((t, None), (t, np.zeros(10, F32)), (t.double(), None)):
        with pytest.raises(ValueError):
            s.closest_to_segments(a, md)
    assert not touched
    assert rt.Scene.SEGMENT_OUTPUTS == ("distance", "instance", "triangle", "parameter", "segment_point", "point", "normal", "barycentric",
                                        "uv", "crossings", "clearance", "within", "pops")
    s.close()
