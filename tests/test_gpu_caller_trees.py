"""Caller-supplied trees on the GPU: rt_scene_upload takes any valid tree in RtMeshDesc, and until this file every tree a kernel had
traversed came from one of the library's two builders, which make the same tree and stop at 32 levels.  Here the same triangles go
up under the trees of tests/caller_trees.py -- chains of 64 levels in both child orders, exact and with every box the mesh's bounds,
median splits numbered breadth first with padded boxes, leaves of 0, 1, 2, 30, 31, 32 and more triangles and inverted empty boxes, a
root that is a leaf, triangles that two leaves reference -- and every output that the families' own GPU tests compare exactly is
held to the same brute-force shims (tests/*_oracle.c, which know nothing of trees), through those tests' own _check functions.
`pops` depends on the tree and is compared with no shim; on the loosest chains it is predicted from the tree instead.

The ray shim alone is no brute force: it is the oracle's cast over the oracle's tree.  caller_trees.ray_pool keeps to rays whose
answer no tree changes (directions of length >= 1), and tests/test_caller_trees_host.py shows on the reference that none of them has
two equal smallest crossings.  That file also holds every tree used here valid in float64."""

import numpy as np
import pytest

import box_oracle as bo
import caller_trees as ct
import crossing_oracle as xo
import point_oracle
import query_points as qp
import query_segments as qs
import query_triangles as qt
import ray_oracle
import region_oracle as ro
import section_oracle as sc
import segment_oracle
import tri_intersect_oracle as ti
import triangle_distance_oracle as tdo
import test_gpu_boxes as t_box
import test_gpu_crossing_list as t_xl
import test_gpu_crossings as t_x
import test_gpu_nearby as t_nb
import test_gpu_point_query as t_pt
import test_gpu_regions as t_rg
import test_gpu_sections as t_sc
import test_gpu_segments as t_sg
import test_gpu_tri_intersect as t_ti
import test_gpu_triangle_distance as t_td
from test_gpu_crossings import _eq

pytestmark = pytest.mark.gpu
F32 = np.float32
FLT_MAX = np.finfo(F32).max
N = 129                                                         # two full waves and a one-lane wave
RAY_EXACT = ("t", "instance", "triangle", "location", "normal", "uv")
MIN_KEYS = ("distance", "instance", "triangle", "point")


class _World:
    pass


def _toward(so, centers):
    """how deep a query goes, for the ordering alone: the oracle's node pops of the ray from the camera through the query's centre"""
    eye = np.asarray(ct.CAMERA["pose"][:3], F32)
    c = np.ascontiguousarray(centers, F32)
    return ray_oracle.cast_rays(so, np.tile(eye, (len(c), 1)), np.ascontiguousarray(c - eye, F32))["pops"]


def _pools(rt, orc, scenes, desc, so):
    """129 queries per family from the families' own builders, the deepest last"""
    o, cam = orc.oracle(), ct.camera_rays(scenes)
    rng = np.random.default_rng(41)

    def pick(q, centers):
        return ct.hardest_last((q,), _toward(so, centers), N, rng)[0]
    p = dict(rays=ct.ray_pool(scenes, so, N))
    pts = qp.flatten(qp.families(rng, o, desc, so, cam, n=60))
    p["points"] = pick(pts, pts)
    segs = qs.flatten(qs.families(rng, o, desc, so, cam, n=200)[0])
    p["segments"] = pick(segs, segs.mean(axis=1))
    tris = qt.flatten(qt.families(rng, o, desc, so, cam, n=200)[0])
    p["triangles"] = pick(tris, tris.mean(axis=1))
    tris = t_ti._flat(t_ti.families(rng, o, desc, n=60))
    p["meeting"] = pick(tris, tris.mean(axis=1))
    boxes = t_box._flat(t_box.families(rng, o, desc, n=60))
    p["boxes"] = pick(boxes, boxes.mean(axis=1))
    planes = t_sc._flat(t_sc.families(rng, o, desc, n=60))
    p["planes"] = pick(planes, planes[:, 0])
    reg = t_rg._flat(t_rg.families(rt, rng, o, desc, n=160)[8])
    p["regions8"] = pick(reg, reg[:, :, 0].mean(axis=1))
    p["regions4"] = np.ascontiguousarray(p["regions8"][:, :4])  # four faces of the oriented box: an unbounded prism
    assert all(len(v[0] if isinstance(v, tuple) else v) == N for v in p.values())
    return p


@pytest.fixture(scope="module")
def world(rt, orc, scenes, blob5k):
    """the scene on the oracle, as uploaded and deformed; its triangles; the pools and the radii; tree 1's render"""
    w = _World()
    w.rt, w.orc, w.o = rt, orc, orc.oracle()
    w.desc = ct.scene(blob5k)
    w.so = w.desc.build_oracle(orc)
    w.tris = ct.mesh_triangles(rt, w.desc)
    for k, h in enumerate(w.desc.oracle_meshes):                # the oracle and the library number the triangles alike
        assert np.array_equal(w.o.mesh_dump(h)["tris"][:, :9], w.tris[k][:, :9])
    w.pools = _pools(rt, orc, scenes, w.desc, w.so)
    rng = np.random.default_rng(43)
    w.diag = t_nb._diag(orc, w.desc)
    dist = point_oracle.closest_points(w.so, w.pools["points"])["distance"]
    w.point_md, w.nearby_md = qp.special_bounds(rng, dist), t_nb._bounds(rng, dist, w.diag)
    w.segment_md = t_sg._bounds(rng, segment_oracle.closest_to_segments(w.so, w.pools["segments"]), w.diag)
    w.triangle_md = t_td._bounds(rng, tdo.closest_to_triangles(w.so, w.pools["triangles"]), w.diag)
    lo, hi = qp.scene_box(w.o, w.desc, w.desc.oracle_meshes)
    span = np.maximum(hi - lo, F32(1e-3)).astype(F32)
    w.grid = ((lo - F32(0.05) * span).astype(F32), (F32(1.1) * span / np.asarray((5, 3, 2), F32)).astype(F32), (5, 3, 2))
    w.whole = np.ascontiguousarray(np.stack([lo - span, hi + span])[None], F32)
    # the deformed scene of the refit tests, on an oracle scene of its own
    w.desc2 = ct.scene(blob5k)
    w.so2 = w.desc2.build_oracle(orc)
    w.tris2 = [ct.deformed(w.o, t) for t in w.tris]
    for h, t in zip(w.desc2.oracle_meshes, w.tris2):
        w.o.mesh_refit(h, t)
    # tree 1: the library's own scene, for the render
    w.cam = rt.Camera(ct.CAMERA["width"], ct.CAMERA["height"], scenes.scaled_K(ct.CAMERA["width"]), scenes.D_REF)
    w.cam.set_pose(ct.CAMERA["pose"])
    sp = w.desc.build_product(rt)
    sp.upload_to_device()
    w.render = rt.render_ids(sp, w.cam)
    w.library_depth = sp.info()["max_stack"]
    sp.close()
    assert (w.render["hit_inst"] >= 0).mean() > 0.1
    # mesh A alone at the identity: one tree's pops
    w.desc_a = ct.identity_scene()
    w.so_a = w.desc_a.build_oracle(orc)
    yield w
    for so in (w.so, w.so2, w.so_a):
        so.close()


def _raw(w, name, desc=None, tris=None):
    desc = desc or w.desc
    tris = tris or w.tris
    if name == "library":
        trees = [ct.library_tree(w.rt.Mesh.from_triangles(t).dump()) for t in tris]
    else:
        trees = [ct.variant(w.rt, name, t, k) for k, t in enumerate(tris)]
    return ct.RawScene(w.rt, list(zip(tris, trees)), desc.materials, desc.instances), trees


def _rays(sp, so, o, d, where):
    """trace_rays, binned and not, and occluded with tmax at the hit and at its float successor, against the oracle's cast"""
    ref = ray_oracle.cast_rays(so, o, d)
    hit = ref["instance"] >= 0
    assert hit.sum() > 40, where
    for binning in (False, True):
        got = sp.trace_rays(o, d, outputs=RAY_EXACT, binning=binning)
        for k in RAY_EXACT:
            _eq(got[k], ref[k], "%s trace_rays binning=%s %s" % (where, binning, k))
    with np.errstate(over="ignore"):
        bounds = ((ref["t"], 0), (np.nextafter(ref["t"], F32(np.inf)), 1))
    for tmax, want in bounds:
        occ = ray_oracle.cast_rays(so, o, d, lighting_pass=1, tmax=tmax)["occluded"]
        assert (occ[hit] == want).all() and not occ[~hit].any(), where      # (the bound is exclusive: on the reference)
        for binning in (False, True):
            got = sp.occluded(o, d, np.ascontiguousarray(tmax, F32), binning=binning)
            assert np.array_equal(got, occ), (where, "occluded", want, binning, np.flatnonzero(got != occ)[:5])
    return ref


def _every_family(w, sp, where, so=None):
    """every family on its pool against its shim, through the family's own comparison"""
    so = so or w.so
    p = w.pools
    o, d = p["rays"]
    _rays(sp, so, o, d, where)
    t_pt._check(sp, so, p["points"], where=where)
    t_pt._check(sp, so, p["points"], w.point_md, where=where + " bounded")
    t_x._check_rays(sp, so, o, d, where=where)
    t_x._check_points(sp, so, p["points"], where=where)
    t_x._check_points(sp, so, p["points"], w.point_md, where=where + " bounded")
    t_xl._check(sp, so, o, d, where=where, ks=(3,))
    t_nb._check(sp, so, p["points"], w.nearby_md, w.point_md, where=where, ks=(3,))
    t_ti._check(sp, so, p["meeting"], where=where, ks=(3,))
    t_box._check(sp, so, p["boxes"], where=where, ks=(3,))
    origin, spacing, dims = w.grid
    g = sp.occupancy_grid(origin, spacing, dims, outputs=("occupied", "count"), as_numpy=True)
    ref = bo.count_in_boxes(so, bo.grid_boxes(origin, spacing, dims)).reshape(dims[::-1])
    _eq(g["count"], ref, where + " grid count")
    assert np.array_equal(g["occupied"], ref > 0) and ref.sum() > 0, where
    assert np.array_equal(sp.occupancy_grid(origin, spacing, dims, as_numpy=True)["occupied"], ref > 0), where + " occupied alone"
    t_sc._check(sp, so, p["planes"], where=where, ks=(3,))
    for K in (4, 8):
        t_rg._check(sp, so, p["regions%d" % K], where="%s K=%d" % (where, K), ms=(3,))
    t_sg._check(sp, so, p["segments"], where=where)
    t_sg._check(sp, so, p["segments"], w.segment_md, where=where + " bounded")
    t_td._check(sp, so, p["triangles"], where=where)
    t_td._check(sp, so, p["triangles"], w.triangle_md, where=where + " bounded")


def _render(w, sp, where):
    got = w.rt.render_ids(sp, w.cam)
    for k in ("img", "hit_inst", "hit_tri"):
        assert np.array_equal(got[k], w.render[k]), (where, k, int((got[k] != w.render[k]).sum()))


@pytest.mark.parametrize("name", ("library",) + ct.VARIANTS[:-1])
def test_whatever_the_tree(world, name):
    """Trees 1 to 6 over the same triangles, two meshes in three instances (rotated with a non-uniform scale, mirrored, identity):
    every exact output of every query family equals its shim bit for bit (NaN equals NaN), and the production render equals the
    render under the library's own tree.  The tree with empty leaves carries the unordered-box flag and so takes every family down
    its no-prune path; the same split without them does not."""
    w = world
    sp, trees = _raw(w, name)
    try:
        depth = max(t["levels"] for t in trees)
        assert sp.info()["max_stack"] == depth and (depth == 64) == name.startswith("chain"), (name, depth)
        flags = [sp.mesh_flags(k) & 1 for k in range(2)]
        assert flags == ([1, 1] if name == "median_empty" else [0, 0]), (name, flags)
        _every_family(w, sp, name)
        _render(w, sp, name)
    finally:
        sp.close()


@pytest.mark.parametrize("deep_child", (0, 1))
def test_the_stack_reaches_its_spill_array(world, deep_child):
    """Chains of 64 levels over mesh A at the identity: rt_scene_info reports a stack of 64, and the results equal the shims.
    With every box the mesh's bounds no predicate can prune below a root it passes, so a query that passes the bounds visits all 63
    interior nodes: pops == 63 in every family that counts interior nodes, for every unbounded point (its lower bound to the
    bounds is below every triangle's distance), and for every box, plane, region, ray and triangle that the shim gives at least one
    pair (a pair lies inside the bounds); pops == 127 for rt_trace_rays, which counts the reference's pops (raycast.cu:61: the 63
    interior nodes and the 64 leaves), for every ray whose parameter at the bounds is below its final distance.
    No stack gauge exists.  The evidence that the stack left its 17 LDS rows is this equality and the reading of the walkers: by
    walk_unordered's rule (child a continues, child b is postponed when both pass) the deep_child = 0 chain holds one postponed leaf
    per level, 63 at the bottom, 47 of them in the spill array (indices up to sp - lds_depth = 46 of its 48 entries); the
    nearest-first kernels postpone child b on equal bounds (a_near = !(lb < la)), so they do the same on that chain, and the ray cast
    postpones child a on equal distances (a tie takes the else branch), so it does so on the deep_child = 1 chain."""
    w = world
    p = w.pools
    tris = [w.tris[1]]
    for loose in (False, True):
        tree = ct.chain(tris[0], 64, deep_child, 3)
        tree = ct.loosened(tree, "all_root") if loose else tree
        sp = ct.RawScene(w.rt, [(tris[0], tree)], w.desc_a.materials, w.desc_a.instances)
        where = "chain %d %s" % (deep_child, "all_root" if loose else "exact")
        try:
            assert sp.info()["max_stack"] == 64 and sp.mesh_flags(0) == 0, where
            o, d = p["rays"]
            ref = _rays(sp, w.so_a, o, d, where)
            t_pt._check(sp, w.so_a, p["points"], where=where)
            t_x._check_rays(sp, w.so_a, o, d, where=where)
            t_box._check(sp, w.so_a, p["boxes"], where=where, ks=(3,))
            t_sc._check(sp, w.so_a, p["planes"], where=where, ks=(3,))
            t_rg._check(sp, w.so_a, p["regions8"], where=where, ms=(3,))
            t_ti._check(sp, w.so_a, p["meeting"], where=where, ks=(3,))
            if not loose:
                continue
            got = sp.closest_points(p["points"], outputs=("distance", "pops"))["pops"]
            assert (got == 63).all(), (where, "closest_points", np.unique(got))
            counted = (("count_in_boxes", sp.count_in_boxes(p["boxes"], outputs=("count", "pops")), bo.count_in_boxes(w.so_a, p["boxes"])),
                       ("count_sections", sp.count_sections(p["planes"], outputs=("count", "pops")), sc.count_sections(w.so_a, p["planes"])),
                       ("count_in_regions", sp.count_in_regions(p["regions8"], outputs=("count", "pops")), ro.count_in_regions(w.so_a, p["regions8"])["count"]),
                       ("count_crossings", sp.count_crossings(o, d, outputs=("count", "pops")), xo.count_crossings(w.so_a, o, d)["count"]),
                       ("count_intersecting", sp.count_intersecting(p["meeting"], outputs=("count", "pops")), ti.count_intersecting(w.so_a, p["meeting"])))
            for what, g, cnt in counted:
                cnt = np.asarray(cnt["count"] if isinstance(cnt, dict) else cnt)
                print(where, what, "queries with a pair:", int((cnt > 0).sum()), "pops:", np.unique(g["pops"]))
                assert (cnt > 0).sum() >= 5, (where, what)
                assert (g["pops"][cnt > 0] == 63).all() and g["pops"].max() == 63, (where, what, np.unique(g["pops"]))
            at_bounds = np.array([w.o.aabb(tree["node_bounds"][0, :3], tree["node_bounds"][0, 3:], oo, dd) for oo, dd in zip(o, d)], F32)
            sel = at_bounds < ref["t"]
            pops = sp.trace_rays(o, d, outputs=("t", "pops"), binning=False)["pops"]
            print(where, "trace_rays: rays through the bounds:", int(sel.sum()), "pops:", np.unique(pops))
            assert sel.sum() >= 20 and (pops[sel] == 127).all() and pops.max() == 127, (where, np.unique(pops[sel]))
        finally:
            sp.close()


@pytest.mark.parametrize("levels", ct.SEAM_LEVELS)
def test_queries_at_the_lds_spill_seam(world, levels):
    """The query-side counterpart of test_stack_depth_at_the_lds_boundary: chains of 16, 17, 18 and 19 levels with every box the
    mesh's bounds, in both child orders, straddle lds_rows() = 17; one call each of closest_points, count_in_boxes, count_sections
    and list_crossings against the shims, and the unbounded points' pops say that every level was visited."""
    w = world
    p = w.pools
    a = w.tris[1]
    o, d = p["rays"]
    for deep_child in (0, 1):
        sp = ct.RawScene(w.rt, [(a, ct.seam_chain(a, levels, deep_child))], w.desc_a.materials, w.desc_a.instances)
        where = "seam %d / %d" % (levels, deep_child)
        try:
            assert sp.info()["max_stack"] == levels
            got, _ref = t_pt._check(sp, w.so_a, p["points"], where=where)
            assert (got["pops"] == levels - 1).all(), (where, np.unique(got["pops"]))
            _eq(sp.count_in_boxes(p["boxes"])["count"], bo.count_in_boxes(w.so_a, p["boxes"]), where + " count_in_boxes")
            _eq(sp.count_sections(p["planes"])["count"], sc.count_sections(w.so_a, p["planes"]), where + " count_sections")
            t_xl._check(sp, w.so_a, o, d, where=where, ks=())
        finally:
            sp.close()


def _interior_records(trees, tris):
    """Where rt_scene_upload lays the interior records (include/rt_hip.h, DESIGN.md "Data layout in HBM"): per mesh its interior
    nodes in node order, room for max(interior nodes, triangles - 1) of them, then its triangle slots, room for max(sum of the leaf
    counts, triangles).  -> list per mesh of (record index [k], child a node [k], child b node [k])"""
    out, base = [], 0
    for tree, t in zip(trees, tris):
        child = tree["node_children"]
        inner = np.flatnonzero(child[:, 0] > 0)
        out.append((base + np.arange(len(inner)), child[inner, 0], child[inner, 1]))
        slots = int(tree["node_leaf_count"][child[:, 0] <= 0].sum())
        base += max(len(inner), len(t) - 1) + max(slots, len(t))
    return out


@pytest.mark.parametrize("name", ("chain0", "median_empty", "shared"))
def test_refit_on_caller_trees(world, name):
    """rt_scene_refit_mesh on trees the library did not build, vertices moved by a smooth deformation.  The 64-level chain has 63
    levels of one interior node each: the run kernel's batch of 32 levels fills and is flushed (the branch no builder's tree
    reaches).  The padded boxes become exact and the empty leaves stay empty (the flag stays).  With shared references the mesh has
    more slots than triangles, and every reference moves.  Afterwards every interior record holds the exact bounds of the triangles
    below its two children, computed here from the tree, and the queries equal the shims on the deformed oracle scene; on the chain's
    scene rt_scene_rebuild_mesh_device then replaces the tree by the library's own, and rt_scene_info still reports a stack that
    holds it."""
    w = world
    p = w.pools
    sp, trees = _raw(w, name)
    try:
        for k, t in enumerate(w.tris2):
            sp.refit(k, t)
        rec = sp.debug_read(0, np.float32).reshape(-1, 16)
        for k, (index, a, b) in enumerate(_interior_records(trees, w.tris)):
            want = ct.exact_bounds(trees[k], w.tris2[k])
            # (as values: a bound that is a zero is the same bound with either sign, and which of two zeros a minimum returns is
            # left open, in numpy as in fminf; no bound is a NaN)
            for words, side, what in ((slice(0, 6), a, "a"), (slice(6, 12), b, "b")):
                bad = np.flatnonzero((rec[index, words] != want[side]).any(axis=1))
                assert bad.size == 0, "%s mesh %d: %d child %s boxes are not exact after the refit, first record %d: got %s want %s" % (
                    name, k, bad.size, what, index[bad[0]], rec[index[bad[0]], words], want[side[bad[0]]])
        assert [sp.mesh_flags(k) & 1 for k in range(2)] == ([1, 1] if name == "median_empty" else [0, 0])
        o, d = p["rays"]
        where = name + " refitted"
        _rays(sp, w.so2, o, d, where)
        t_pt._check(sp, w.so2, p["points"], where=where)
        if name == "shared":
            _shared_counts(w, sp, trees, where)
        else:
            t_box._check(sp, w.so2, p["boxes"], where=where, ks=(3,))
            t_sc._check(sp, w.so2, p["planes"], where=where, ks=(3,))
        if name == "chain0":
            for k, t in enumerate(w.tris2):
                sp.rebuild_on_device(k, t)
            own = max(ct.depth(ct.library_tree(w.rt.Mesh.from_triangles(t).dump())) for t in w.tris2)
            assert own <= sp.info()["max_stack"] <= 64, (own, sp.info())
            _every_family(w, sp, name + " rebuilt", so=w.so2)
    finally:
        sp.close()


def _shared_counts(w, sp, trees, where):
    """a box around the whole scene: every instance's triangles, each once per leaf that references it (include/rt_hip.h, RtMeshDesc)"""
    want = sum(int(trees[mesh]["node_leaf_count"].sum()) for mesh, _m, _p, _s in w.desc.instances)
    assert want == sum(len(w.tris[mesh]) + ct.SHARED_K for mesh, _m, _p, _s in w.desc.instances)
    c = sp.count_in_boxes(w.whole, outputs=("count",))["count"]
    assert int(c[0]) == want, (where, int(c[0]), want)
    g = sp.list_in_boxes(w.whole, outputs=("instance", "triangle"))
    assert int(g["count"][0]) == want
    for i, (mesh, _m, _p, _s) in enumerate(w.desc.instances):
        _eq(np.bincount(g["triangle"][g["instance"] == i], minlength=len(w.tris[mesh])).astype(np.int32), trees[mesh]["refs"], "%s instance %d references" % (where, i))


def test_shared_references(world):
    """Tree 7: 24 triangles of each mesh stand in two leaves, through overlapping leaf ranges and through repeats in leaf_indices.
    The minimum-type answers are those of the mesh without the repeats; a counting or listing query reports a triangle once per leaf
    that references it (what include/rt_hip.h promises next to RtMeshDesc)."""
    w = world
    p = w.pools
    sp, trees = _raw(w, "shared")
    try:
        for k, t in enumerate(trees):
            assert int(t["node_leaf_count"].sum()) == len(w.tris[k]) + ct.SHARED_K
        o, d = p["rays"]
        _rays(sp, w.so, o, d, "shared")
        t_pt._check(sp, w.so, p["points"], where="shared")
        t_pt._check(sp, w.so, p["points"], w.point_md, where="shared bounded")
        got, ref = sp.closest_to_segments(p["segments"], outputs=MIN_KEYS), segment_oracle.closest_to_segments(w.so, p["segments"])
        for k in MIN_KEYS:
            _eq(got[k], ref[k], "shared closest_to_segments " + k)
        got, ref = sp.closest_to_triangles(p["triangles"], outputs=MIN_KEYS), tdo.closest_to_triangles(w.so, p["triangles"])
        for k in MIN_KEYS:
            _eq(got[k], ref[k], "shared closest_to_triangles " + k)
        _shared_counts(w, sp, trees, "shared")
        _render(w, sp, "shared")
    finally:
        sp.close()
