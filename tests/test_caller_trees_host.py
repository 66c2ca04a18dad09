"""The caller-supplied trees of tests/caller_trees.py, without a GPU: every generator and every variant that tests/test_gpu_caller_trees.py
puts on the device is a valid tree in float64 (so a mismatch on the GPU is the kernels' and not the generator's), rt_scene_upload's
validation -- which runs before the device is touched -- accepts them all and answers RT_E_DEPTH to 65 levels, and the ray pool of the
GPU tests has no two equal smallest crossings (the cast's answer is then the same under every tree)."""
import numpy as np
import pytest

import caller_trees as ct
import crossing_list_oracle as xl

RT_E_INVALID, RT_E_DEPTH = -1, -3
MATERIAL = [((1.0, 1.0, 1.0), None)]
IDENTITY = [(0, 0, (0.0,) * 6, (1.0, 1.0, 1.0))]


@pytest.fixture(scope="module")
def meshes(rt, blob5k):
    return ct.mesh_triangles(rt, ct.scene(blob5k))            # [mesh B, mesh A]


def _valid(tree, tris, levels=None, shared=0, where=""):
    """Float64: boxes contain what is below them (declared empty leaves apart), children after parents, one parent each, every node
    reachable, ranges inside leaf_indices, every triangle in as many leaves as the tree states (one, but for `shared` more in all),
    the depth the tree states (and the one asked for)."""
    child, first, count = tree["node_children"], tree["node_leaf_first"], tree["node_leaf_count"]
    m, n = len(child), len(tris)
    v = np.asarray(tris, np.float32)[:, :9].reshape(n, 3, 3).astype(np.float64)
    seen, level = np.zeros(m, int), np.zeros(m, int)
    level[0] = 1
    refs = np.zeros(n, int)
    for i in range(m):
        assert level[i] > 0, (where, i, "unreachable, or a child in front of its parent")
        a, b = int(child[i, 0]), int(child[i, 1])
        if a > 0:
            assert i < a < m and i < b < m and a != b, (where, i, a, b)
            seen[a] += 1
            seen[b] += 1
            level[a] = level[b] = level[i] + 1
            assert count[i] == 0, (where, i)
        else:
            assert (a, b) == (-1, -1) and 0 <= first[i] and first[i] + count[i] <= len(tree["leaf_indices"]), (where, i)
            idx = tree["leaf_indices"][first[i]:first[i] + count[i]]
            assert len(set(idx.tolist())) == len(idx) and (idx >= 0).all() and (idx < n).all(), (where, i, "a leaf lists a triangle twice")
            refs[idx] += 1
            assert (count[i] == 0) == (i in tree["empty"]), (where, i)
    assert (seen[1:] == 1).all() and seen[0] == 0, where
    assert int(level.max()) == tree["levels"] == ct.depth(tree) and (levels is None or tree["levels"] == levels), (where, level.max(), tree["levels"], levels)
    assert np.array_equal(refs, tree["refs"]) and refs.min() >= 1 and int((refs - 1).sum()) == shared, (where, refs.min(), (refs - 1).sum())
    under = ct.below(tree)
    for i in range(m):
        box = tree["node_bounds"][i].astype(np.float64)
        if i in tree["empty"]:
            assert (tree["node_bounds"][i] == ct.EMPTY_BOX).all() and len(under[i]) == 0, (where, i)
            continue
        p = v[under[i]].reshape(-1, 3)
        assert len(p) and (box[:3] <= p.min(axis=0)).all() and (box[3:] >= p.max(axis=0)).all(), (where, i, "the box does not hold what is below it")
    return level


def _interior_boxes_exact(tree, tris):
    return np.array_equal(tree["node_bounds"], ct.exact_bounds(tree, tris))


def test_generators(meshes):
    """every generator on its own, at the parameters the issue names"""
    a = meshes[1]
    rng = np.random.default_rng(1)
    for dc in (0, 1):
        t = ct.chain(a, 64, dc, 3)
        _valid(t, a, levels=64, where="chain 64 / %d" % dc)
        inner = [i for i in range(len(t["node_children"])) if not ct.is_leaf(t, i)]
        assert len(inner) == 63 and len(t["node_children"]) == 127 and (t["node_leaf_count"][t["node_children"][:, 0] <= 0] == 3).all()
        assert all(t["node_children"][i, dc] == i + 2 and ct.is_leaf(t, t["node_children"][i, 1 - dc]) for i in inner)
        assert _interior_boxes_exact(t, a)
        r = ct.loosened(t, "all_root")
        _valid(r, a, levels=64, where="all_root")
        assert (r["node_bounds"] == t["node_bounds"][0]).all()
        p = ct.loosened(t, "padded", rng)
        _valid(p, a, levels=64, where="padded")
        assert (p["node_bounds"][:, :3] <= t["node_bounds"][:, :3]).all() and (p["node_bounds"][:, 3:] >= t["node_bounds"][:, 3:]).all()
        assert (p["node_bounds"] != t["node_bounds"]).mean() > 0.5
    _valid(ct.chain(a, 65, 0, 2), a, levels=65, where="chain 65")
    _valid(ct.chain(a, 1, 0, 3), a, levels=1, where="chain 1")
    _valid(ct.root_leaf(a), a, levels=1, where="root_leaf")
    for order in ("bfs", "pre"):
        t = ct.median(a, ct.LEAF_SIZES, order, np.random.default_rng(3))
        level = _valid(t, a, where="median " + order)
        assert _interior_boxes_exact(t, a) and len(t["empty"]) >= 1
        if order == "bfs":
            assert (np.diff(level) >= 0).all()                  # numbered level by level
        else:
            assert (np.diff(level) < 0).any() and all(t["node_children"][i, 0] == i + 1 or t["node_children"][i, 1] == i + 1
                                                       for i in range(len(level)) if not ct.is_leaf(t, i))
    t = ct.median(meshes[0], [s for s in ct.LEAF_SIZES if s], "pre", np.random.default_rng(4))
    _valid(t, meshes[0], where="median on mesh B")
    s = ct.shared(t, 10, np.random.default_rng(5), meshes[0])
    _valid(s, meshes[0], shared=10, where="shared")
    assert len(s["leaf_indices"]) < int(s["node_leaf_count"].sum())            # some ranges overlap ...
    assert len(s["leaf_indices"]) > len(meshes[0])                              # ... and some triangles are listed twice


def test_the_gpu_tests_trees_are_valid(rt, meshes):
    """every variant of tests/test_gpu_caller_trees.py, on both meshes, and the chains at the LDS / spill seam"""
    for k, tris in enumerate(meshes):
        for name in ct.VARIANTS:
            t = ct.variant(rt, name, tris, k)
            _valid(t, tris, levels=64 if name.startswith("chain") else None, shared=ct.SHARED_K if name == "shared" else 0, where=(name, k))
            sizes = set(t["node_leaf_count"][t["node_children"][:, 0] <= 0].tolist())
            if name == "median_empty":
                assert {0, 31, 32} <= sizes and max(sizes) > 32 and len(t["empty"]) >= 1, (k, sorted(sizes))
            if name in ("median", "shared"):
                assert 0 not in sizes and not t["empty"] and (t["node_bounds"][:, :3] <= t["node_bounds"][:, 3:]).all(), (k, sorted(sizes))
            if name == "median":
                assert {31, 32} <= sizes and max(sizes) > 32, (k, sorted(sizes))
            if name == "shared":
                assert np.array_equal(t["node_children"], ct.variant(rt, "median", tris, k)["node_children"])     # (tree 5's topology)
    assert ct.variant(rt, "root_leaf", meshes[1], 1)["levels"] == 1
    for levels in ct.SEAM_LEVELS:
        for dc in (0, 1):
            _valid(ct.seam_chain(meshes[1], levels, dc), meshes[1], levels=levels, where=("seam", levels, dc))


def test_upload_validation_and_depth(rt, meshes, blob5k):
    """rt_scene_upload validates before it touches the device: 65 levels are RT_E_DEPTH, 64 levels and every other tree here pass
    (without a device the call then ends with the no-device error, as test_scene_upload_validates_its_input expects)"""
    a = meshes[1]
    no_gpu = rt.device_count() == 0
    assert ct.upload_rc(rt, [(a, ct.chain(a, 65, 0, 2))], MATERIAL, IDENTITY) == RT_E_DEPTH
    assert ct.upload_rc(rt, [(a, ct.chain(a, 65, 1, 2))], MATERIAL, IDENTITY) == RT_E_DEPTH
    for dc in (0, 1):
        rc = ct.upload_rc(rt, [(a, ct.chain(a, 64, dc, 3))], MATERIAL, IDENTITY)
        assert rc not in (RT_E_DEPTH, RT_E_INVALID) and (rc != 0) == no_gpu, rc
    desc = ct.scene(blob5k)
    for name in ct.VARIANTS:
        rc = ct.upload_rc(rt, [(t, ct.variant(rt, name, t, k)) for k, t in enumerate(meshes)], desc.materials, desc.instances)
        assert rc not in (RT_E_DEPTH, RT_E_INVALID) and (rc != 0) == no_gpu, (name, rc)
    for levels in ct.SEAM_LEVELS:
        rc = ct.upload_rc(rt, [(a, ct.seam_chain(a, levels, 0))], MATERIAL, IDENTITY)
        assert rc not in (RT_E_DEPTH, RT_E_INVALID) and (rc != 0) == no_gpu, (levels, rc)
    # a tree one level too deep beside a valid mesh, and a depth that only the second mesh has
    lib = ct.library_tree(rt.Mesh.from_triangles(a).dump())
    assert ct.upload_rc(rt, [(a, lib), (a, ct.chain(a, 65, 0, 2))], MATERIAL, IDENTITY) == RT_E_DEPTH


def test_the_ray_pool_has_no_ties(orc, scenes, blob5k):
    """The ray shim is the oracle's cast over ITS tree: it agrees with a cast over any other tree when no ray has two equal smallest
    crossings.  The crossing-list shim (brute force, sorted by t) says so for the pool of the GPU tests, on the scene as uploaded and
    on the deformed scene of the refit test.  A seed that gives a tie is replaced here (caller_trees.RAY_SEED), never masked there."""
    desc = ct.scene(blob5k)
    so = desc.build_oracle(orc)
    try:
        o, d = ct.ray_pool(scenes, so)
        assert len(o) == 129
        for state in ("uploaded", "deformed"):
            if state == "deformed":
                for k, h in enumerate(desc.oracle_meshes):
                    orc.oracle().mesh_refit(h, ct.deformed(orc.oracle(), orc.oracle().mesh_dump(h)["tris"]))
            ref = xl.list_crossings(so, o, d)
            off, t = ref["offsets"], ref["t"]
            two = np.flatnonzero(ref["count"] >= 2)
            ties = two[t[off[two]] == t[off[two] + 1]]
            assert ties.size == 0, (state, ties, t[off[ties]])
            assert (ref["count"] > 0).sum() > 40, state
    finally:
        so.close()
