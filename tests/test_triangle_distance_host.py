"""Triangle distance queries without a GPU: the brute-force shim (tests/triangle_distance_oracle.c) that the GPU tests compare with is
pinned on hand-made cases with exact answers, on the guards, on degenerate input, against the same triangles placed in world space and
against float64; the C-ABI and the Python wrapper reject bad arguments before they touch a device (the GPU side:
test_gpu_triangle_distance.py)."""
import ctypes as C

import numpy as np
import pytest

import point_oracle
import scene_defs as sd
import segment_oracle
import tri_intersect_oracle
import triangle_distance_oracle as tdo
from test_segment_host import _dot, _point_triangle64, _scene, _segment_segment64, _tris

F32 = np.float32
FLT_MAX = np.finfo(F32).max
A, AB, AC = np.zeros(3, F32), np.array([2, 0, 0], F32), np.array([0, 2, 0], F32)
# The shim's worst distance error against float64 over 20 000 cases of test_shim_against_float64's kind, relative to the largest
# coordinate magnitude of the case, as measured over this seed (1.72e-7) and three others (1.69e-7, 1.64e-7, 2.06e-7): the worst of the
# four.  The test asserts four times that, section 18's margin, there because near-parallel edge pairs lose
# digits in den.
MEASURED_REL_ERROR = 2.07e-7
IDENTITY = [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))]


def _on(q):
    return tdo.on_triangle(np.array(q, F32), A, AB, AC)


def test_three_kinds_of_candidate_and_the_tie_order():
    """Power-of-two cases with exact answers on the triangle (0,0,0) (2,0,0) (0,2,0): a candidate of each kind wins where it should,
    with its weights on both triangles and d2; among equal candidates the first in the order 0..14 wins."""
    cases = [
        # the query's three vertices -> which, q1, q2, b1, b2, d2
        (((0.5, 0.5, 1), (0.5, 0.5, 3), (1, 0.5, 3)), 0, 0.0, 0.0, 0.25, 0.25, 1.0),       # (a): V0 above the face
        (((0.5, 0.5, 3), (0.5, 0.5, 1), (1, 0.5, 3)), 1, 1.0, 0.0, 0.25, 0.25, 1.0),       # (a): V1
        (((0.5, 0.5, 3), (1, 0.5, 3), (0.5, 0.5, 1)), 2, 0.0, 1.0, 0.25, 0.25, 1.0),       # (a): V2
        (((3, -2, -2), (3, 6, -2), (3, -2, 6)), 4, 0.25, 0.25, 1.0, 0.0, 1.0),             # (b): W1 under the query's interior
        (((-2, 3, -2), (6, 3, -2), (-2, 3, 6)), 5, 0.25, 0.25, 0.0, 1.0, 1.0),             # (b): W2
        (((-1, -2, -2), (-1, 6, -2), (-1, -2, 6)), 3, 0.25, 0.25, 0.0, 0.0, 1.0),          # (b): W0; W2 and the edge AC tie, 3 is first
        (((1, -1, -1), (1, -1, 1), (1, -3, 0)), 6, 0.5, 0.0, 0.5, 0.0, 1.0),               # (c): query edge 0 beside the edge AB
        (((-1, 1, -1), (-3, 1, 0), (-1, 1, 1)), 10, 0.0, 0.5, 0.0, 0.5, 1.0),              # (c): query edge 1 beside the edge AC
        (((4, 4, 0), (2, 2, -1), (2, 2, 1)), 14, 0.5, 0.5, 0.5, 0.5, 2.0),                 # (c): query edge 2 beside the edge BC
        (((1, 0, 1), (1, 0, 3), (1, 1, 3)), 0, 0.0, 0.0, 0.5, 0.0, 1.0),                   # a vertex exactly over an edge: (a) before (c)
        (((0.5, -1, 0), (1.5, -1, 0), (1, -3, 0)), 0, 0.0, 0.0, 0.25, 0.0, 1.0),           # parallel edges: V0, V1 and the pair tie
        (((0, 0, 1), (2, 0, 1), (0, 2, 1)), 0, 0.0, 0.0, 0.0, 0.0, 1.0),                   # parallel faces: all fifteen are 1
        (((-1, -1, 0), (-1, -1, 0), (-1, -1, 0)), 0, 0.0, 0.0, 0.0, 0.0, 2.0),             # all vertices equal: the point query
        (((-1, -1, 0), (-1, -1, 0), (-1, -3, 0)), 0, 0.0, 0.0, 0.0, 0.0, 2.0),             # two equal vertices: edge 0 is not taken
        (((1, -1, 0), (1, 1, 0), (3, 0, 0)), 1, 1.0, 0.0, 0.5, 0.5, 0.0),                  # coplanar and overlapping: V1 lies on BC
    ]
    for q, which, q1, q2, b1, b2, d2 in cases:
        got = _on(q)
        assert got == (F32(q1), F32(q2), F32(b1), F32(b2), F32(d2), which), (q, got)
    # in the parallel-face case every one of the fifteen is 1: each kind alone, reached by reordering, gives the same d2
    for q in (((0, 0, 1), (2, 0, 1), (0, 2, 1)), ((2, 0, 1), (0, 2, 1), (0, 0, 1)), ((0, 2, 1), (0, 0, 1), (2, 0, 1))):
        assert _on(q)[4:] == (F32(1.0), 0)


def test_point_triangle_is_the_point_query(orc):
    """P0 == P1 == P2: every field the two shims share is the same bits, over posed, scaled and mirrored instances and under a bound;
    the winner is candidate 0."""
    tris = sd.random_triangles(60, seed=11, spread=1.0, size=0.5)
    instances = [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (0, 0, (0.3, -0.2, 0.5, 0.4, -0.7, 1.1), (1.5, -0.5, 2.0)),
                 (0, 0, (-1.0, 0.5, 0.0, 0.0, 3.0, -0.2), (-1.0, -1.0, 0.25))]
    so = _scene(orc, tris, instances)
    try:
        rng = np.random.default_rng(3)
        pts = rng.uniform(-3, 3, (300, 3)).astype(F32)
        pts[:8] = 0.0
        pts[:4] *= F32(-1.0)                                    # (-0 too)
        q = np.ascontiguousarray(np.stack([pts, pts, pts], axis=1))
        for md in (None, rng.uniform(0.1, 1.5, 300).astype(F32)):
            got, ref = tdo.closest_to_triangles(so, q, md), point_oracle.closest_points(so, pts, md)
            for k in point_oracle.OUTPUTS:
                assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
            assert not got["query_barycentric"].any() and (got["intersections"] == 0).all()
            assert (got["which"][got["instance"] >= 0] == 0).all()
            assert np.array_equal(got["clearance"], got["distance"]) and np.array_equal(got["within"], got["instance"] >= 0)
    finally:
        so.close()


def test_two_equal_vertices_stay_close_to_the_segment_query(orc):
    """A triangle with two equal vertices is a segment; rule 14 promises no bit equality with rule 13 there (the reversed third edge
    and the (b) candidates may undercut in the last bits), only the same distance to rounding, and never a larger one by more."""
    so = _scene(orc, sd.random_triangles(60, seed=11, spread=1.0, size=0.5), [(0, 0, (0.3, -0.2, 0.5, 0.4, -0.7, 1.1), (1.5, -0.5, 2.0))])
    try:
        rng = np.random.default_rng(4)
        p = rng.uniform(-3, 3, (200, 3)).astype(F32)
        q = (p + rng.normal(size=(200, 3)) * rng.choice([0.01, 0.3, 2.0], (200, 1))).astype(F32)
        seg = segment_oracle.closest_to_segments(so, np.ascontiguousarray(np.stack([p, q], axis=1)))
        for form in ((p, p, q), (p, q, q), (q, p, q)):
            got = tdo.closest_to_triangles(so, np.ascontiguousarray(np.stack(form, axis=1)))
            assert np.isfinite(got["distance"]).all() and (got["instance"] >= 0).all()
            assert np.abs(got["distance"].astype(np.float64) - seg["distance"]).max() <= 4e-6       # (coordinates up to about 8)
            assert ((got["query_barycentric"] >= 0) & (got["query_barycentric"] <= 1)).all()
    finally:
        so.close()


def _triangle_triangle64(q, a, b, c):
    """the float64 minimum over rule 14's fifteen candidates, solved exactly: q [n, 3, 3], a / b / c [n, 3]"""
    best = np.full(len(a), np.inf)
    for k in range(3):
        best = np.minimum(best, _point_triangle64(q[:, k], a, b, c))
    for v in (a, b, c):
        best = np.minimum(best, _point_triangle64(v, q[:, 0], q[:, 1], q[:, 2]))
    for m in range(3):
        g0, g1 = q[:, m], q[:, (m + 1) % 3]
        for x, y in ((a, b), (b, c), (c, a)):
            best = np.minimum(best, _segment_segment64(g0, g1 - g0, x, y - x))
    return best


def _pierces64(p0, p1, a, b, c):
    """whether the segments p0 -> p1 meet the triangles (a, b, c), in float64 (touching counts)"""
    n = np.cross(b - a, c - a)
    h0, h1 = _dot(p0 - a, n), _dot(p1 - a, n)
    cut = (h0 * h1 <= 0) & (h0 != h1)
    w = p0 + (h0 / np.where(cut, h0 - h1, 1.0))[..., None] * (p1 - p0)
    for x, y in ((a, b), (b, c), (c, a)):
        cut = cut & (_dot(np.cross(y - x, w - x), n) >= 0)
    return cut


def _intersect64(q, a, b, c):
    hit = np.zeros(len(a), bool)
    t = (a, b, c)
    for m in range(3):
        hit |= _pierces64(q[:, m], q[:, (m + 1) % 3], a, b, c)
        hit |= _pierces64(t[m], t[(m + 1) % 3], q[:, 0], q[:, 1], q[:, 2])
    return hit


def test_degenerate_scene_triangles_are_finite():
    """Zero-area, collinear, repeated-vertex, single-point and needle scene triangles, against query triangles that are degenerate a
    fifth of the time: nothing divides by zero, every weight finite and in [0, 1], and the distance within 1e-5 of float64's."""
    rng = np.random.default_rng(1)
    for _ in range(300):
        a, b = rng.uniform(-1, 1, (2, 3)).astype(F32)
        kind = int(rng.integers(5))
        c = {0: a, 1: (a + F32(rng.choice([2.0, 0.5, -1.0])) * (b - a)).astype(F32), 2: b,
             3: (a + F32(0.4) * (b - a) + rng.uniform(-1, 1, 3).astype(F32) * F32(1e-6)).astype(F32), 4: a}[kind]
        if kind == 4:
            b = a
        q = rng.uniform(-2, 2, (3, 3)).astype(F32)
        r = rng.random()
        if r < 0.1:
            q[1] = q[0]
        elif r < 0.2:
            q[2] = q[1] = q[0]
        q1, q2, b1, b2, d2, which = tdo.on_triangle(q, a, (b - a).astype(F32), (c - a).astype(F32))
        assert np.isfinite([q1, q2, b1, b2, d2]).all() and min(q1, q2, b1, b2) >= 0 and max(q1, q2, b1, b2) <= 1
        assert b1 + b2 <= 1 + 1e-6 and q1 + q2 <= 1 + 1e-6 and 0 <= which <= 14
        want = _triangle_triangle64(q.astype(np.float64)[None], *(np.asarray(v, np.float64)[None] for v in (a, b, c)))[0]
        assert abs(np.sqrt(np.float64(d2)) - want) <= 1e-5 * max(1.0, want), (a, b, c, q)


def test_piercing_and_coplanar_overlap(orc):
    """A triangle through the middle of a large one: every candidate of the minimum is far away (distance > 0, a miss under a small
    radius) and the intersection half says intersections > 0, clearance == 0, within == 1.  Coplanar overlapping triangles, which
    rule 10 does not report, reach distance 0 through the vertex and edge candidates."""
    so = _scene(orc, _tris(orc, [[-8, -8, 0, 8, -8, 0, 0, 8, 0]]), IDENTITY)
    try:
        q = np.array([[[0, 0, -1], [0.5, 0, 1], [-0.5, 0, 1]], [[0, 0, 1], [0.5, 0, 3], [-0.5, 0, 3]],
                      [[1, -1, 0], [1, 1, 0], [3, 0, 0]]], F32)
        free = tdo.closest_to_triangles(so, q)
        assert free["distance"].tolist() == [1.0, 1.0, 0.0] and free["intersections"].tolist() == [1, 0, 0]
        assert free["clearance"].tolist() == [0.0, 1.0, 0.0] and free["within"].tolist() == [1, 1, 1]
        got = tdo.closest_to_triangles(so, q, np.full(3, 0.25, F32))
        assert got["distance"].tolist() == [FLT_MAX, FLT_MAX, 0.0] and got["instance"].tolist() == [-1, -1, 0]
        assert got["intersections"].tolist() == [1, 0, 0] and got["clearance"].tolist() == [0.0, FLT_MAX, 0.0]
        assert got["within"].tolist() == [1, 0, 1]
        assert not got["point"][:2].any() and not got["query_point"][:2].any() and not got["query_barycentric"][:2].any()
        assert np.array_equal(tri_intersect_oracle.count_intersecting(so, q), got["intersections"])
        # skip_instance takes the only instance out of both halves
        none = tdo.closest_to_triangles(so, q, None, np.zeros(3, np.int32))
        assert (none["instance"] == -1).all() and not none["intersections"].any() and not none["within"].any()
    finally:
        so.close()


def test_posed_instances_against_world_space_triangles(orc):
    """Rotated, translated, non-uniformly scaled and mirrored instances against the same triangles placed in world space under an
    identity instance: the same distances and nearest pairs to rounding, the same winners away from ties, the same intersections."""
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
    flat = _scene(orc, _tris(orc, np.concatenate(world)), IDENTITY)
    try:
        rng = np.random.default_rng(8)
        p0 = rng.uniform(-3, 3, (400, 1, 3))
        q = np.ascontiguousarray(p0 + rng.normal(size=(400, 3, 3)) * rng.choice([0.01, 0.3, 1.0], (400, 1, 1)), F32)
        a, b = tdo.closest_to_triangles(posed, q), tdo.closest_to_triangles(flat, q)
        assert np.abs(a["distance"] - b["distance"]).max() <= 2e-5
        assert np.array_equal(a["intersections"], b["intersections"]) and (a["intersections"] > 0).sum() >= 10
        same = a["instance"] * 40 + a["triangle"] == b["triangle"]
        assert same.mean() > 0.95
        assert np.abs(a["query_point"] - b["query_point"])[same].max() <= 1e-3
        assert np.abs(a["point"] - b["point"])[same].max() <= 1e-3
        # the nearest pair is at the distance, in world space, and the query's point has the query's weights
        gap = np.linalg.norm(a["query_point"].astype(np.float64) - a["point"], axis=1)
        assert np.abs(gap - a["distance"]).max() <= 2e-5
        w = a["query_barycentric"].astype(np.float64)
        x = q[:, 0] + w[:, :1] * (q[:, 1].astype(np.float64) - q[:, 0]) + w[:, 1:] * (q[:, 2].astype(np.float64) - q[:, 0])
        assert np.abs(x - a["query_point"]).max() <= 2e-5
        # skipping an instance: the result is the scene without it
        sk = rng.integers(-1, 3, 400).astype(np.int32)
        c = tdo.closest_to_triangles(posed, q, None, sk)
        assert (c["instance"] != sk).all() and (c["distance"] >= a["distance"]).all()
        keep = a["instance"] != sk
        assert np.array_equal(c["distance"][keep], a["distance"][keep]) and np.array_equal(c["triangle"][keep], a["triangle"][keep])
    finally:
        posed.close()
        flat.close()


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def _float64_cases(orc, n=20000, seed=13):
    """n random posed (query triangle, scene triangle) pairs in scaled mesh space, as the rule sees them (fp32), a tenth of them with a
    query edge nearly parallel to the scene edge AB: q [n, 3, 3], a, ab, ac [n, 3] float32"""
    o = orc.oracle()
    rng = np.random.default_rng(seed)
    poses = [np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-3.1, 3.1, 3)]).astype(F32) for _ in range(8)]
    scales = np.array([(1, 1, 1), (1.5, -0.5, 2.0), (-1, -1, 0.25), (0.5, 2, 1), (1, 1, 1), (3, 3, 3), (-2, 1, 1), (0.1, 0.1, 0.1)], F32)
    v = (rng.uniform(-1, 1, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3)) * rng.choice([0.05, 0.5, 1.0], (n, 1, 1))).astype(F32)
    which = rng.integers(0, 8, n)
    sc = scales[which]
    a, ab, ac = v[:, 0] * sc, (v[:, 1] - v[:, 0]) * sc, (v[:, 2] - v[:, 0]) * sc
    p = (rng.uniform(-2, 2, (n, 1, 3)) + rng.normal(size=(n, 3, 3)) * rng.choice([1e-3, 0.05, 0.5, 3.0], (n, 1, 1))).astype(F32)
    q = np.zeros((n, 3, 3), F32)
    for j in range(n):                                          # world triangles through the instance map
        for k in range(3):
            q[j, k] = o.apply_lre(poses[which[j]], p[j, k])
    par = rng.random(n) < 0.1                                   # made in mesh space, an edge beside the edge AB
    off = rng.normal(size=(n, 3)) * 0.3
    q[par, 0] = (a + ab * rng.uniform(-0.5, 1.0, (n, 1)) + off)[par]
    q[par, 1] = (q[:, 0] + ab * rng.uniform(0.2, 2.0, (n, 1)) + rng.normal(size=(n, 3)) * rng.choice([0, 1e-6, 1e-4], (n, 1)))[par]
    return q, a.astype(F32), ab.astype(F32), ac.astype(F32)


def _shim_on_cases(cases):
    return np.array([tdo.on_triangle(*(c[j] for c in cases))[:5] for j in range(len(cases[0]))], F32)


def _rel_error(cases):
    out = _shim_on_cases(cases)
    q, a, ab, ac = (c.astype(np.float64) for c in cases)
    b, c = a + ab, a + ac
    dist = np.sqrt(out[:, 4].astype(np.float64))
    mag = np.max(np.abs(np.concatenate([q.reshape(-1, 9), a, b, c], axis=1)), axis=1)
    return out, dist, mag, np.abs(dist - _triangle_triangle64(q, a, b, c)) / mag


def test_shim_against_float64(orc):
    """20 000 random posed pairs: the shim's distance against (1) the float64 minimum over the same fifteen candidates, solved
    exactly, within 4 x MEASURED_REL_ERROR of the largest coordinate magnitude involved, and (2) independently, a barycentric
    sampling of the query triangle against the scene triangle in float64.  Outside the pairs that intersect, told apart in float64,
    no sample is closer than the shim by more than that error; and in every pair some sample is within half a sampling step of the
    shim's answer.  The step is an eighth of the query's longest edge; the samples are the barycentric grid of 16 subdivisions,
    whose cells have sides of at most half a step, so every point of the query triangle is within step / (2 sqrt 3) of a sample and
    the distance, being 1-Lipschitz, is within that of a sample's.  The winner's weights reproduce the distance."""
    cases = _float64_cases(orc)
    out, dist, mag, rel = _rel_error(cases)
    q, a, ab, ac = (c.astype(np.float64) for c in cases)
    b, c = a + ab, a + ac
    assert np.isfinite(dist).all() and (out[:, :4] >= 0).all() and (out[:, :4] <= 1).all()
    print("worst relative error %.3g (asserted: %.3g), mean %.3g" % (rel.max(), 4 * MEASURED_REL_ERROR, rel.mean()))
    assert rel.max() <= 4 * MEASURED_REL_ERROR, (rel.max(), int(rel.argmax()))
    # the pair the shim names is at the shim's distance
    w = out.astype(np.float64)
    x = q[:, 0] + w[:, :1] * (q[:, 1] - q[:, 0]) + w[:, 1:2] * (q[:, 2] - q[:, 0])
    y = a + w[:, 2:3] * ab + w[:, 3:4] * ac
    assert (np.abs(np.linalg.norm(x - y, axis=1) - dist) / mag).max() <= 4 * MEASURED_REL_ERROR
    K = 16
    i, j = np.meshgrid(np.arange(K + 1), np.arange(K + 1), indexing="ij")
    keep = i + j <= K
    w1, w2 = (i[keep] / K)[None, :, None], (j[keep] / K)[None, :, None]
    sampled = np.full(len(dist), np.inf)
    for lo in range(0, len(dist), 1000):
        sl = slice(lo, lo + 1000)
        p = q[sl, 0, None] + w1 * (q[sl, 1] - q[sl, 0])[:, None] + w2 * (q[sl, 2] - q[sl, 0])[:, None]
        sampled[sl] = _point_triangle64(p, a[sl, None], b[sl, None], c[sl, None]).min(axis=1)
    longest = np.max([np.linalg.norm(q[:, (m + 1) % 3] - q[:, m], axis=1) for m in range(3)], axis=0)
    step = longest / 8
    tol = 4 * MEASURED_REL_ERROR * mag
    meet = _intersect64(q, a, b, c)
    assert 10 <= meet.sum() < len(dist) // 2
    assert (sampled <= dist + step / 2 + tol).all(), "no sample of the query triangle is as close as the shim's answer"
    assert (sampled >= dist - tol)[~meet].all(), "a sample of the query triangle is closer than the shim's answer"


def test_max_distance_is_inclusive(orc):
    """The exact distance is within, its float predecessor is not (unless the triangles intersect); +inf is; NaN and negative bounds
    are not (the distance then FLT_MAX), and the intersections do not depend on the bound."""
    so = _scene(orc, sd.random_triangles(30, seed=6, spread=1.0, size=0.4), IDENTITY)
    try:
        rng = np.random.default_rng(7)
        q = np.ascontiguousarray(rng.uniform(-2, 2, (100, 1, 3)) + rng.normal(size=(100, 3, 3)) * 0.3, F32)
        free = tdo.closest_to_triangles(so, q)
        d = free["distance"]
        assert (d > 0).all() and (free["intersections"] > 0).any()
        for md, want in ((d, True), (np.nextafter(d, F32(0)), False), (np.full(100, np.inf, F32), True),
                         (np.full(100, np.nan, F32), False), (np.full(100, -1.0, F32), False), (np.zeros(100, F32), False)):
            got = tdo.closest_to_triangles(so, q, np.asarray(md, F32))
            assert ((got["instance"] >= 0) == want).all()
            assert np.array_equal(got["intersections"], free["intersections"])
            assert np.array_equal(got["within"], ((got["instance"] >= 0) | (got["intersections"] > 0)).astype(np.int32))
            assert np.array_equal(got["clearance"], np.where(got["intersections"] > 0, F32(0), got["distance"]))
            if not want:
                assert (got["distance"] == FLT_MAX).all() and (got["triangle"] == -1).all() and not got["point"].any()
    finally:
        so.close()


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    """librt_hip.so exports rt_closest_to_triangles; it refuses a NULL scene, n < 0, NULL triangles and no output before touching the
    scene, and n == 0 returns at once."""
    h = rt.libs()[0]
    assert hasattr(h, "rt_closest_to_triangles") and "rt_closest_to_triangles" in rt.RT_HIP_SYMBOLS
    hits = rt.RtTriangleHits()
    out = C.c_void_p(64)
    with_out = rt.RtTriangleHits(within=out)
    assert h.rt_closest_to_triangles(None, C.c_void_p(64), None, None, 3, C.byref(with_out), None, 0) == -1
    bogus = C.c_void_p(16)                                        # a handle that is never dereferenced
    assert h.rt_closest_to_triangles(bogus, C.c_void_p(64), None, None, -1, C.byref(with_out), None, 0) == -1
    assert h.rt_closest_to_triangles(bogus, None, None, None, 3, C.byref(with_out), None, 0) == -1
    assert h.rt_closest_to_triangles(bogus, C.c_void_p(64), None, None, 3, C.byref(hits), None, 0) == -1
    assert h.rt_closest_to_triangles(bogus, C.c_void_p(64), None, None, 3, None, None, 0) == -1
    assert h.rt_closest_to_triangles(bogus, None, None, None, 0, None, None, 0) == 0
    assert [f[0] for f in rt.RtTriangleHits._fields_] == list(rt.Scene.TRIANGLE_HIT_OUTPUTS)
    assert h.rt_abi_version() == 2


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    p = np.zeros((10, 3, 3), F32)
    for bad in (p.astype(np.float64), p[:, :, :2].copy(), p[:, :2].copy(), np.zeros((10, 3), F32), np.zeros((3, 3, 10), F32).T,
                p.reshape(-1), [[[0, 0, 0]] * 3] * 10):
        with pytest.raises(ValueError):
            s.closest_to_triangles(bad)
    for md in (np.zeros(9, F32), np.zeros(10, np.float64), np.zeros((10, 1), F32), np.zeros((10, 3), F32)):
        with pytest.raises(ValueError):
            s.closest_to_triangles(p, md)
    for sk in (np.zeros(9, np.int32), np.zeros(10, np.int64), np.zeros(10, F32), np.zeros((10, 1), np.int32)):
        with pytest.raises(ValueError):
            s.closest_to_triangles(p, None, sk)
    for outs in (("distance", "colour"), (), ("t",), ("crossings",), ("parameter",)):
        with pytest.raises(ValueError):
            s.closest_to_triangles(p, outputs=outs)
    torch = pytest.importorskip("torch")
    t = torch.zeros((10, 3, 3), dtype=torch.float32)
    for a, md in ((t, None), (t, np.zeros(10, F32)), (t.double(), None)):
        with pytest.raises(ValueError):
            s.closest_to_triangles(a, md)
    assert not touched
    assert rt.Scene.TRIANGLE_HIT_OUTPUTS == ("distance", "instance", "triangle", "query_barycentric", "query_point", "point", "normal",
                                             "barycentric", "uv", "intersections", "clearance", "within", "pops")
    s.close()
