"""Sphere sweeps without a GPU: the brute-force shim (tests/sweep_oracle.c) that the GPU tests compare with is pinned on hand-made
power-of-two cases with exact answers for each of the eight candidates and the tie order, against the point shim where the sphere
starts in contact, on degenerate input, against the same triangles placed in world space and against float64 (the study that fixes
rule 16's constants); the C-ABI and the Python wrapper reject bad arguments before they touch a device (the GPU side:
test_gpu_sweeps.py)."""
import ctypes as C

import numpy as np
import pytest

import point_oracle
import scene_defs as sd
import sweep_oracle

F32 = np.float32
FLT_MAX = np.finfo(F32).max
A, AB, AC = np.zeros(3, F32), np.array([4, 0, 0], F32), np.array([0, 4, 0], F32)
# The float64 study, measured with seeds 1..12 of _cases, 20 000 cases each.
# The constants of rule 16 step 3 are the smallest powers of two with which no case whose float64 minimum distance along the path is
# below r (1 - DELTA) was reported as a miss: 2^-21 lost one contact in seed 13 and one in seed 14 (2^-22 one in nearly every seed).
KR = KM = 2.0 ** -20
# the worst |distance64(centre at the reported time) - r| / r of a moving contact (seed 10), and four times that: the margin is for
# other seeds.  The error is a few ulps of r + M (worst 8.3 ulps), so relative to r it rises with M / r, which reaches 3e4 here.
MEASURED_REL_CONTACT_ERROR = 6.47e-3
DELTA = 4 * MEASURED_REL_CONTACT_ERROR
# the worst |time - time64| |D| / (r + M) (seed 12), asserted at four times that
MEASURED_TIME_ERROR = 8.69e-6


def _scene(orc, tris, instances):
    return sd.SceneDesc([((1.0, 1.0, 1.0), None)], [("tris", tris)], instances).build_oracle(orc)


def _tris(orc, verts):
    o = orc.oracle()
    out = np.stack([o.tri_from_vertices(np.asarray(v, F32).ravel()) for v in verts])
    out[:, 12:18] = [0, 0, 1, 0, 0, 1]
    return out


def test_the_constants_are_the_studys():
    assert sweep_oracle.KR == KR and sweep_oracle.KM == KM
    q0, q1 = np.array([1, -8, 2], F32), np.array([3, 4, -5], F32)
    for r in (0.0, 0.5, 3.0):
        rw = F32(F32(F32(r) + F32(F32(r) * F32(KR))) + F32(F32(8) * F32(KM)))
        assert sweep_oracle.reach2(q0, q1, r) == F32(rw * rw)
    assert sweep_oracle.reach2(q0, q1, np.inf) == np.inf


def test_eight_candidates_and_the_tie_order():
    """Exact answers on the triangle (0,0,0), (4,0,0), (0,4,0) with r = 1: every kind of candidate wins where it should, and equal
    times go to the first in the order start, face, edges AB / AC / BC, vertices A / B / C."""
    def run(q0, q1, r=1.0, tri=(A, AB, AC)):
        return sweep_oracle.on_triangle(q0, q1, r, *tri)
    # head-on onto the face from height 4: s = (h - r) / |D|
    s, b1, b2, d2, which = run((1, 1, 4), (1, 1, 0))
    assert (s, b1, b2, d2, which) == (0.75, 0.25, 0.25, 1.0, 1)
    s, b1, b2, d2, which = run((1, 1, -4), (1, 1, 0))           # from the other side
    assert (s, d2, which) == (0.75, 1.0, 1)
    assert run((1, 1, 4), (1, 1, 8))[4] == -1                    # moving away: no face root, nothing else in reach
    # onto an edge from the side, in the triangle's plane (the face's slab holds the centre: no face root)
    assert run((2, -4, 0), (2, 0, 0)) == (0.75, 0.5, 0.0, 1.0, 2)
    assert run((-4, 2, 0), (0, 2, 0)) == (0.75, 0.0, 0.5, 1.0, 3)
    s, b1, b2, d2, which = run((6, 6, 0), (2, 2, 0))
    assert which == 4 and abs(float(s) - (1 - 2 ** 0.5 / 8)) < 1e-6       # BC is the line x + y = 4: (8 - 8 s) / sqrt(2) = 1
    assert abs(np.sqrt(d2) - 1) < 1e-6 and abs(b1 - 0.5) < 1e-6 and abs(b2 - 0.5) < 1e-6
    # onto the vertices from outside the corners
    for q0, at, kind, bary in (((-3, -3, 0), (0, 0, 0), 5, (0, 0)), ((7, -3, 0), (4, 0, 0), 6, (1, 0)), ((-3, 7, 0), (0, 4, 0), 7, (0, 1))):
        s, b1, b2, d2, which = run(q0, at)
        assert which == kind and (b1, b2) == bary and abs(float(s) - (1 - 1 / (3 * 2 ** 0.5))) < 1e-6 and abs(np.sqrt(d2) - 1) < 1e-6
    # ties: along the x axis towards A the cylinder about AC and the sphere about A are entered at once (the edge is earlier in the
    # order; AB's line is the path's own: no root); straight down onto A the face and the vertex
    assert run((-4, 0, 0), (0, 0, 0)) == (0.75, 0.0, 0.0, 1.0, 3)
    assert run((0, 0, 4), (0, 0, 0)) == (0.75, 0.0, 0.0, 1.0, 1)
    # start in contact: time 0 with the point query's weights, whatever the path; r - distance is the penetration
    assert run((1, 1, 0.5), (1, 1, -8)) == (0.0, 0.25, 0.25, 0.25, 0)
    assert run((1, 1, 1), (9, 9, 9)) == (0.0, 0.25, 0.25, 1.0, 0)       # touching counts: the radius is inclusive
    # contact exactly at s = 1 counts; a path that stops short does not
    assert run((1, 1, 4), (1, 1, 1)) == (1.0, 0.25, 0.25, 1.0, 1)
    assert run((1, 1, 4), (1, 1, 1.5))[4] == -1
    # zero length: the start alone
    assert run((1, 1, 0.5), (1, 1, 0.5)) == (0.0, 0.25, 0.25, 0.25, 0)
    assert run((1, 1, 2), (1, 1, 2))[4] == -1
    # radius: 0 is a point (it touches where the path crosses the face), +inf touches at once, NaN and negative never
    assert run((1, 1, 4), (1, 1, -4), r=0.0) == (0.5, 0.25, 0.25, 0.0, 1)
    assert run((1, 1, 4), (1, 1, 0), r=np.inf)[::4] == (0.0, 0)
    assert run((1, 1, 0.5), (1, 1, 0), r=np.nan)[4] == -1 and run((1, 1, 0.5), (1, 1, 0), r=-1.0)[4] == -1


def test_a_face_root_off_the_triangle_is_rejected():
    """The centre reaches the offset plane beside the triangle: the root is priced, lies farther than r, and is not a contact."""
    assert sweep_oracle.on_triangle((-2, -2, 4), (-2, -2, 0), 1.0, A, AB, AC)[4] == -1
    # an edge root beyond the edge's end likewise: AB's line is reached at x = 8
    assert sweep_oracle.on_triangle((8, -4, 0), (8, 0, 0), 1.0, A, AB, AC)[4] == -1
    # ... unless the vertex is in reach there
    s, b1, b2, d2, which = sweep_oracle.on_triangle((4.5, -4, 0), (4.5, 0, 0), 1.0, A, AB, AC)
    assert which == 6 and (b1, b2) == (1, 0) and abs(np.sqrt(d2) - 1) < 1e-6


def test_degenerate_triangles():
    """A triangle that is a point has its vertex candidates alone, one that is a segment its edges; nothing is NaN."""
    Z = np.zeros(3, F32)
    assert sweep_oracle.on_triangle((0, 0, 4), (0, 0, 0), 1.0, Z, Z, Z) == (0.75, 0.0, 0.0, 1.0, 5)
    s, b1, b2, d2, which = sweep_oracle.on_triangle((2, 0, 4), (2, 0, 0), 1.0, Z, np.array([4, 0, 0], F32), np.array([8, 0, 0], F32))
    assert (s, d2, which) == (0.75, 1.0, 2) and np.isfinite([b1, b2]).all()
    assert sweep_oracle.on_triangle((0, 0, 4), (0, 0, 0), 1.0, Z + np.nan, AB, AC)[4] == -1


def test_start_in_contact_and_zero_length_are_the_point_query(orc):
    """Wherever the point shim has a winner within r of P0, the sweep reports time 0 and the same bits in every field the two share;
    a zero-length sweep has nothing else."""
    tris = sd.random_triangles(60, seed=11, spread=1.0, size=0.5)
    instances = [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0)), (0, 0, (0.3, -0.2, 0.5, 0.4, -0.7, 1.1), (1.5, -0.5, 2.0)),
                 (0, 0, (-1.0, 0.5, 0.0, 0.0, 3.0, -0.2), (-1.0, -1.0, 0.25))]
    so = _scene(orc, tris, instances)
    try:
        rng = np.random.default_rng(3)
        pts = rng.uniform(-3, 3, (400, 3)).astype(F32)
        r = rng.uniform(0.05, 1.0, 400).astype(F32)
        ref = point_oracle.closest_points(so, pts, r)
        at = ref["instance"] >= 0
        assert at.sum() >= 100 and (~at).sum() >= 100
        moving = np.ascontiguousarray(np.stack([pts, pts + rng.normal(size=(400, 3)).astype(F32)], axis=1))
        still = np.ascontiguousarray(np.stack([pts, pts], axis=1))
        for segs in (moving, still):
            got = sweep_oracle.sweep_spheres(so, segs, r)
            for k in point_oracle.OUTPUTS:
                assert np.array_equal(got[k][at].view(np.uint32), ref[k][at].view(np.uint32)), k
            assert (got["time"][at] == 0).all() and (got["which"][at] == 0).all() and (got["hit"][at] == 1).all()
            assert np.abs(got["centre"][at] - pts[at]).max() <= 1e-5           # (to the instance's space and back)
        # (a zero-length sweep just beyond r may still be valid under reach2; it is then a start candidate too)
        assert (got["which"][got["hit"] == 1] == 0).all() and (got["hit"][~at].sum() <= 2)
    finally:
        so.close()


def test_posed_instances_against_world_space_triangles(orc):
    """Rotated, translated, non-uniformly scaled and mirrored instances against the same triangles placed in world space under an
    identity instance: the same times and contacts to rounding, the same winners away from ties; centre, point and contact_normal
    are consistent in world space."""
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
        p0 = rng.uniform(-3, 3, (600, 3))
        segs = np.ascontiguousarray(np.stack([p0, p0 + rng.normal(size=(600, 3)) * rng.choice([0.3, 2.0, 6.0], (600, 1))], axis=1), F32)
        r = rng.uniform(0.02, 0.3, 600).astype(F32)
        a, b = sweep_oracle.sweep_spheres(posed, segs, r), sweep_oracle.sweep_spheres(flat, segs, r)
        both = (a["hit"] == 1) & (b["hit"] == 1)
        assert (a["hit"] != b["hit"]).sum() <= 2 and both.sum() >= 100 and (a["which"][both] > 0).sum() >= 50
        same = both & (a["instance"] * 40 + a["triangle"] == b["triangle"])
        assert same.sum() > 0.95 * both.sum()
        length = np.linalg.norm((segs[:, 1] - segs[:, 0]).astype(np.float64), axis=1)
        assert (np.abs(a["time"].astype(np.float64) - b["time"])[same] * length[same]).max() <= 1e-3
        assert np.abs(a["centre"] - b["centre"])[same].max() <= 1e-3 and np.abs(a["point"] - b["point"])[same].max() <= 1e-3
        # in world space: centre is on the path, point is at `distance` from it, contact_normal points from point to centre
        h = a["hit"] == 1
        on_path = segs[:, 0].astype(np.float64) + a["time"].astype(np.float64)[:, None] * (segs[:, 1].astype(np.float64) - segs[:, 0])
        assert np.abs(on_path - a["centre"])[h].max() <= 2e-5
        gap = a["centre"].astype(np.float64) - a["point"]
        assert np.abs(np.linalg.norm(gap, axis=1) - a["distance"])[h].max() <= 2e-5
        moving = h & (a["which"] > 0)
        assert np.abs(a["distance"][moving] - r[moving]).max() <= 2e-5
        assert np.abs(gap / a["distance"][:, None] - a["contact_normal"])[moving].max() <= 1e-3
        assert np.abs(np.linalg.norm(a["contact_normal"].astype(np.float64), axis=1) - 1)[h].max() <= 1e-5
    finally:
        posed.close()
        flat.close()


# ---- float64 ------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(axis=-1)


def _distance64(x, a, b, c):
    """distance of the points x to the triangles (a, b, c) in float64: the face where the projection falls inside it, else the
    nearest edge"""
    def seg(p, q):
        e = q - p
        ee = _dot(e, e)
        t = np.clip(_dot(x - p, e) / np.where(ee > 0, ee, 1.0), 0.0, 1.0)
        v = x - (p + t[..., None] * e)
        return np.sqrt(_dot(v, v))
    d = np.minimum(np.minimum(seg(a, b), seg(a, c)), seg(b, c))
    n = np.cross(b - a, c - a)
    nn = np.sqrt(_dot(n, n))
    ok = nn > 0
    nh = n / np.where(ok, nn, 1.0)[..., None]
    inside = ok
    for p, q in ((a, b), (b, c), (c, a)):
        inside = inside & (_dot(np.cross(q - p, x - p), nh) >= 0)
    return np.where(inside, np.minimum(d, np.abs(_dot(nh, x - a))), d)


def _cases(seed, n):
    """posed cases: a triangle of size 0.1 .. 10 placed 0.1 .. 100 sizes from the origin, a radius of 0.01 .. 1 sizes, a path that
    starts 0.1 .. 5 sizes from a point of the triangle and is aimed within two radii of it, stopping short or going beyond"""
    g = np.random.default_rng(seed)
    size = 10 ** g.uniform(-1, 1, n)
    off = g.normal(size=(n, 3)) * (size * 10 ** g.uniform(-1, 2, n))[:, None]
    tri = g.uniform(-1, 1, (n, 3, 3)) * size[:, None, None] + off[:, None, :]
    r = size * 10 ** g.uniform(-2, 0, n)
    on = (tri * g.dirichlet((1, 1, 1), n)[:, :, None]).sum(1)
    p0 = on + g.normal(size=(n, 3)) * (size * 10 ** g.uniform(-1, 0.7, n))[:, None]
    aim = on + g.normal(size=(n, 3)) * (r * g.uniform(0, 2, n))[:, None]
    p1 = p0 + (aim - p0) * (10 ** g.uniform(-0.5, 0.5, n))[:, None]
    return tri.astype(F32), p0.astype(F32), p1.astype(F32), r.astype(F32)


def _truth64(a, ab, ac, p0, p1, r, samples=513):
    """-> (minimum distance along the path, whether it comes within r, the time of impact) in float64, for the triangle as the rule
    sees it (A, A + AB, A + AC in fp32) and the path Q0 + s D with D the fp32 difference: dense sampling, a ternary search for the
    minimum (the distance to a convex set is convex along a line) and a bisection of distance - r at the first crossing"""
    A_, B_, C_ = a.astype(np.float64), (a + ab).astype(np.float64), (a + ac).astype(np.float64)
    q0, d, r = p0.astype(np.float64), (p1 - p0).astype(np.float64), r.astype(np.float64)
    s = np.linspace(0, 1, samples)
    dd = _distance64(q0[:, None, :] + s[None, :, None] * d[:, None, :], A_[:, None], B_[:, None], C_[:, None])
    k = dd.argmin(1)
    lo, hi = s[np.maximum(k - 1, 0)], s[np.minimum(k + 1, samples - 1)]
    for _ in range(80):
        m1, m2 = lo + (hi - lo) / 3, hi - (hi - lo) / 3
        worse = _distance64(q0 + m1[:, None] * d, A_, B_, C_) > _distance64(q0 + m2[:, None] * d, A_, B_, C_)
        lo, hi = np.where(worse, m1, lo), np.where(worse, hi, m2)
    dmin = np.minimum(dd.min(1), _distance64(q0 + (0.5 * (lo + hi))[:, None] * d, A_, B_, C_))
    inside = dd <= r[:, None]
    first = inside.argmax(1)
    lo, hi = s[np.maximum(first - 1, 0)], s[first]
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        ins = _distance64(q0 + mid[:, None] * d, A_, B_, C_) <= r
        lo, hi = np.where(ins, lo, mid), np.where(ins, mid, hi)
    return dmin, inside.any(1), np.where(first == 0, 0.0, hi)


def test_shim_against_float64():
    """20 000 posed cases against float64, with a seed the study did not use: no path that comes within r (1 - DELTA) of the
    triangle is reported as a miss, none that stays beyond r (1 + DELTA) as a hit; the centre at the reported time is at r to DELTA;
    the time is the float64 time of impact to four times the study's worst error."""
    n, step = 20000, 2500
    tri, p0, p1, r = _cases(101, n)
    a = np.ascontiguousarray(tri[:, 0])
    ab, ac = np.ascontiguousarray(tri[:, 1] - tri[:, 0]), np.ascontiguousarray(tri[:, 2] - tri[:, 0])
    out = np.array([sweep_oracle.on_triangle(p0[j], p1[j], r[j], a[j], ab[j], ac[j]) for j in range(n)], np.float64)
    time, which = out[:, 0], out[:, 4].astype(np.int64)
    hit = which >= 0
    parts = [_truth64(a[i:i + step], ab[i:i + step], ac[i:i + step], p0[i:i + step], p1[i:i + step], r[i:i + step]) for i in range(0, n, step)]
    dmin, comes, time64 = (np.concatenate([p[k] for p in parts]) for k in range(3))
    r64 = r.astype(np.float64)
    assert hit.sum() >= 8000 and (~hit).sum() >= 4000 and all((which == k).sum() >= 100 for k in range(8))
    missed = ~hit & (dmin < r64 * (1 - DELTA))
    assert not missed.any(), (missed.sum(), np.flatnonzero(missed)[:5])
    false = hit & (dmin > r64 * (1 + DELTA))
    assert not false.any(), (false.sum(), np.flatnonzero(false)[:5])
    q0, d = p0.astype(np.float64), (p1 - p0).astype(np.float64)
    at = _distance64(q0 + time[:, None] * d, a.astype(np.float64), (a + ab).astype(np.float64), (a + ac).astype(np.float64))
    moving = hit & (which > 0)
    rel = np.abs(at - r64)[moving] / r64[moving]
    big = np.maximum(np.abs(p0).max(1), np.abs(p1).max(1)).astype(np.float64)
    ulps = (np.abs(at - r64) / (r64 + big))[moving] * 2 ** 23
    both = hit & comes
    terr = np.abs(time - time64)[both] * np.sqrt(_dot(d, d))[both] / (r64 + big)[both]
    print("contact error: worst %.3g of r, %.2f ulps of r + M; time error: worst %.3g of r + M; M / r up to %.3g"
          % (rel.max(), ulps.max(), terr.max(), (big / r64).max()))
    assert rel.max() <= DELTA
    assert terr.max() <= 4 * MEASURED_TIME_ERROR


def test_c_abi_exports_and_rejects_bad_arguments(rt):
    """librt_hip.so exports rt_sweep_spheres; it refuses a NULL scene, n < 0, NULL segments, a NULL radius and no output before
    touching the scene, and n == 0 returns at once.  The call is additive: the ABI version stays."""
    h = rt.libs()[0]
    assert hasattr(h, "rt_sweep_spheres") and "rt_sweep_spheres" in rt.RT_HIP_SYMBOLS
    hits = rt.RtSweepHits()
    p = C.c_void_p(64)
    with_out = rt.RtSweepHits(hit=p)
    assert h.rt_sweep_spheres(None, p, p, 3, C.byref(with_out), None, 0) == -1
    bogus = C.c_void_p(16)                                        # a handle that is never dereferenced
    assert h.rt_sweep_spheres(bogus, p, p, -1, C.byref(with_out), None, 0) == -1
    assert h.rt_sweep_spheres(bogus, None, p, 3, C.byref(with_out), None, 0) == -1
    assert h.rt_sweep_spheres(bogus, p, None, 3, C.byref(with_out), None, 0) == -1
    assert h.rt_sweep_spheres(bogus, p, p, 3, C.byref(hits), None, 0) == -1
    assert h.rt_sweep_spheres(bogus, p, p, 3, None, None, 0) == -1
    assert h.rt_sweep_spheres(bogus, None, None, 0, None, None, 0) == 0
    assert [f[0] for f in rt.RtSweepHits._fields_] == list(rt.Scene.SWEEP_OUTPUTS)
    assert h.rt_abi_version() == 2


def test_python_wrapper_checks_before_the_device(rt, monkeypatch):
    s = rt.Scene()
    touched = []
    monkeypatch.setattr(rt.Scene, "device_handle", property(lambda self: touched.append(1)))
    p, r = np.zeros((10, 2, 3), F32), np.ones(10, F32)
    for bad in (p.astype(np.float64), p[:, :, :2].copy(), p[:, :1].copy(), np.zeros((10, 3), F32), np.zeros((3, 2, 10), F32).T,
                p.reshape(-1), [[[0, 0, 0]] * 2] * 10):
        with pytest.raises(ValueError):
            s.sweep_spheres(bad, r)
    for rad in (None, np.zeros(9, F32), np.zeros(10, np.float64), np.zeros((10, 1), F32), np.zeros((10, 2), F32), 1.0):
        with pytest.raises(ValueError):
            s.sweep_spheres(p, rad)
    for outs in (("time", "colour"), (), ("t",), ("parameter",), ("within",)):
        with pytest.raises(ValueError):
            s.sweep_spheres(p, r, outputs=outs)
    torch = pytest.importorskip("torch")
    t = torch.zeros((10, 2, 3), dtype=torch.float32)
    for a, rad in ((t, torch.ones(10)), (t, r), (t.double(), torch.ones(10))):
        with pytest.raises(ValueError):
            s.sweep_spheres(a, rad)
    assert not touched
    assert rt.Scene.SWEEP_OUTPUTS == ("time", "distance", "instance", "triangle", "centre", "point", "normal", "contact_normal",
                                      "barycentric", "uv", "hit", "pops")
