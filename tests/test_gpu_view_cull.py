"""Back-facing leaves (view_records_kernel, ViewJob::cull): in the views of primary and G-buffer launches a leaf
child of one to four triangles none of which can be accepted from the frame's origin -- (v0 - origin) . n >= 2^-20 for each, in the
traversal's own fp32 operations -- gets a box that no ray passes.  Frames, hit ids and distances must stay bit for bit what they were:
every case renders a batch of four frames, each with a pose of its own (the smallest launch that gets views), and holds

  - the batch's frames (render_kernel<.., VIEW>) and the G-buffer's images (gbuffer_kernel) to the instrumented kernel's frames, which
    reads no view,
  - the G-buffer's t, instance and triangle planes to those of a child process that runs with RT_VIEW_CULL=0 (read once per process:
    one child renders every case),
  - on two cases the same planes to the CPU oracle,

and asserts through rt_scene_view_cull_stats that the cull really fired -- on the scenes whose tree this file knows, with the count a
numpy evaluation of the rule gives.  Frames are 64 x 48 or smaller (tests/conftest.py lifts the rays-per-record condition)."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import caller_trees as ct
import scene_defs as sd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
F32 = np.float32
K_CULL = F32(2.0 ** -20)                                            # kCullMin
IDENTITY = ((0.0,) * 6, (1.0, 1.0, 1.0))
MATS = [((0.9, 0.5, 0.2), None), ((1.0, 1.0, 1.0), sd.checker_texture())]
# four cameras in front of a scene around the origin, each with its own position and orientation
OUTSIDE = [(0.1, -4.2, 0.4, 0.15, -0.05, 0.1), (-0.6, -3.6, 0.1, -0.1, 0.05, 0.0), (0.7, -4.8, 0.9, 0.2, -0.15, -0.2), (0.0, -3.9, -0.3, 0.0, 0.1, 0.3)]
# ... inside the room
INSIDE = [(0.3, -0.5, 0.2, 0.0, 0.0, 0.0), (-0.4, 0.1, 0.6, 1.2, 0.1, 0.0), (0.0, 0.0, 0.0, -2.0, -0.3, 0.2), (1.1, 0.9, -0.8, 3.0, 0.4, -0.1)]
# ... all at z = 0: the plane of the N = 0 triangle, 1e-40 below the plane of the denormal one
IN_PLANE = [(0.1, -4.2, 0.0, 0.15, -0.05, 0.1), (-0.6, -3.6, 0.0, -0.1, 0.05, 0.0), (0.7, -4.8, 0.0, 0.2, 0.0, -0.2), (0.0, -3.9, 0.0, 0.0, 0.1, 0.3)]
# ... on the axis of sd.deep_stack_scene
AXIS = [(0.0, -1.0, 0.0, 0.0, 0.0, 0.0), (0.01, -1.0, 0.0, 0.01, 0.0, 0.0), (0.0, -1.2, 0.01, 0.0, 0.01, 0.0), (-0.01, -0.9, 0.0, 0.0, 0.0, 0.02)]


# ---- triangles ----------------------------------------------------------------------------------------------------------------------

def _tri(a, b, c, towards):
    """[18] triangle a, b, c wound so that its normal has a positive component along `towards`"""
    import orc
    o = orc.oracle()
    t = o.tri_from_vertices(np.array([a, b, c], F32).ravel())
    if float(np.dot(t[9:12].astype(np.float64), np.asarray(towards, np.float64))) < 0:
        t = o.tri_from_vertices(np.array([a, c, b], F32).ravel())
    t[12:18] = [0, 0, 1, 0, 0, 1]
    return t


def sphere_tris():
    """a closed sphere of radius 1: the icosahedron subdivided twice, 320 triangles, normals outwards"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], np.float64)
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    unit = lambda p: p / np.linalg.norm(p)
    faces = [tuple(unit(v[i]) for i in t) for t in f]
    for _ in range(2):
        nxt = []
        for a, b, c in faces:
            ab, bc, ca = unit(a + b), unit(b + c), unit(c + a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = nxt
    out = np.stack([_tri(a, b, c, a + b + c) for a, b, c in faces])
    assert out.shape == (320, 18)
    return out


def _box_faces(r, sign):
    """the twelve triangles of the cube [-r, r]^3, normals outwards (sign = 1) or inwards (-1)"""
    out = []
    for axis in range(3):
        for side in (-1.0, 1.0):
            u, w = (axis + 1) % 3, (axis + 2) % 3
            p = []
            for su, sw in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                q = [0.0, 0.0, 0.0]
                q[axis], q[u], q[w] = side * r, su * r, sw * r
                p.append(q)
            n = [0.0, 0.0, 0.0]
            n[axis] = side * sign
            out += [_tri(p[0], p[1], p[2], n), _tri(p[0], p[2], p[3], n)]
    return np.stack(out)


def room_tris():
    """a box room seen from inside: walls that face the camera, and the outer faces of the same walls behind them, which never can"""
    return np.concatenate([_box_faces(2.0, -1.0), _box_faces(2.125, 1.0)])


def special_tris():
    """two coincident triangles with opposite normals; a triangle in the plane z = 0 of the IN_PLANE cameras (N = 0) and one 1e-40 above
    it with its normal upwards (N = 1e-40, a denormal); a pair behind them, facing away; random triangles around"""
    a, b, c = (-0.5, 1.0, -0.5), (0.5, 1.0, -0.5), (0.0, 1.0, 0.6)
    tiny = float(F32(1e-40))
    out = [_tri(a, b, c, (0, -1, 0)), _tri(a, b, c, (0, 1, 0)),
           _tri((1.5, 0.5, 0.0), (2.5, 0.5, 0.0), (2.0, 1.5, 0.0), (0, 0, 1)),
           _tri((-2.5, 0.5, tiny), (-1.5, 0.5, tiny), (-2.0, 1.5, tiny), (0, 0, 1)),
           _tri((-0.4, 3.0, 1.0), (0.4, 3.0, 1.0), (0.0, 3.0, 1.8), (0, 1, 0)), _tri((-0.4, 3.2, -1.0), (0.4, 3.2, -1.0), (0.0, 3.2, -1.8), (0, 1, 0))]
    more = sd.random_triangles(40, seed=23, spread=1.2, size=0.3)
    more[:, [1, 4, 7]] += F32(2.0)                                  # (moved along y as a whole: the normals stand)
    return np.concatenate([np.stack(out), more]).astype(F32)


def leaves_tree(tris):
    """a caller's tree over `tris` with leaves of 1, 2, 4, 5 and more than 30 triangles: the first seed that has them all"""
    for seed in range(200):
        t = ct.median(tris, [1, 2, 4, 5, 40], "pre", np.random.default_rng([41, seed]))
        sizes = set(t["node_leaf_count"][t["node_children"][:, 0] <= 0].tolist())
        if {1, 4, 5} <= sizes and max(sizes) > 30:
            return t
    raise AssertionError("no seed gives leaves of 1, 4, 5 and more than 30 triangles")


# ---- the cases: name -> (scene, poses, (triangles, tree) of mesh 0 where the instance is the identity and the count is asserted) --------

def _library(rt, tris, instances=None):
    desc = sd.SceneDesc(MATS, [("tris", tris)], instances or [(0, 1) + IDENTITY])
    sp = desc.build_product(rt)
    sp.upload_to_device()
    return desc, sp, ct.library_tree(desc.product_meshes[0].dump())


def case_sphere(rt):
    tris = sphere_tris()
    desc, sp, tree = _library(rt, tris)
    return dict(sp=sp, desc=desc, poses=OUTSIDE, known=(tris, tree))


def case_room(rt):
    tris = room_tris()
    desc, sp, tree = _library(rt, tris)
    return dict(sp=sp, desc=desc, poses=INSIDE, known=(tris, tree))


def case_specials(rt):
    tris = special_tris()
    desc, sp, tree = _library(rt, tris)
    return dict(sp=sp, desc=desc, poses=IN_PLANE, known=(tris, tree))


def case_leaves(rt):
    tris = ct.mesh_a()
    tree = leaves_tree(tris)
    sp = ct.RawScene(rt, [(tris, tree)], MATS, [(0, 1) + IDENTITY])
    return dict(sp=sp, desc=None, poses=OUTSIDE, known=(tris, tree))


POSED = [(0, 1, (1.3, 0.5, 0.2, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), (0, 0, (-1.2, 0.8, 0.3, 0.7, 0.3, -0.4), (0.6, 1.1, 0.8))]


def case_posed(rt):
    """a translated instance, and a rotated and non-uniformly scaled one"""
    tris = sphere_tris()
    desc, sp, tree = _library(rt, tris, POSED)
    return dict(sp=sp, desc=desc, poses=OUTSIDE, known=(tris, tree))


def case_deep(rt):
    """a tree deeper than the LDS stack: lanes that outgrow it are traced again, on the general stack, through the same views --
    with a sphere beside the chain, whose far half is culled in those views"""
    deep = sd.deep_stack_scene(28)
    desc = sd.SceneDesc(MATS, [deep.meshes[0], ("tris", sphere_tris())], [(0, 0) + IDENTITY, (1, 1, (3.0, 6.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    sp = desc.build_product(rt)
    sp.upload_to_device()
    assert sp.info()["max_stack"] > 17
    return dict(sp=sp, desc=desc, poses=AXIS, known=None)


def unordered_tree(tris):
    """a caller's tree with empty leaves (inverted boxes: the mesh is flagged unordered and every wave takes the generic slab loop)
    beside leaves of 1, 2 and 4 triangles"""
    for seed in range(200):
        t = ct.median(tris, [0, 1, 2, 4], "pre", np.random.default_rng([43, seed]))
        sizes = set(t["node_leaf_count"][t["node_children"][:, 0] <= 0].tolist())
        if {0, 1, 4} <= sizes:
            return t
    raise AssertionError("no seed gives empty leaves beside leaves of 1 and 4 triangles")


def case_unordered(rt):
    tris = ct.mesh_a()
    tree = unordered_tree(tris)
    sp = ct.RawScene(rt, [(tris, tree)], MATS, [(0, 1) + IDENTITY])
    assert sp.mesh_flags(0) & 1
    return dict(sp=sp, desc=None, poses=OUTSIDE, known=(tris, tree))


CASES = dict(sphere=case_sphere, room=case_room, specials=case_specials, leaves=case_leaves, posed=case_posed, deep=case_deep,
             unordered=case_unordered)


# ---- rendering ------------------------------------------------------------------------------------------------------------------------

def _handle(sp):
    h = sp.device_handle
    return h if isinstance(h, C.c_void_p) else C.c_void_p(h)


def _cams(rt, scenes, poses):
    cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
    out = (rt.RtCameraParams * len(poses))()
    for i, ps in enumerate(poses):
        cam.set_pose(ps)
        out[i] = cam.params()
    return cam, out


def gbuffer(rt, scenes, sp, poses):
    """rt_render_gbuffer itself: dict of t, instance, triangle [n, H, W] and image [n, H, W, 3]; asserts that the launch took a view slot"""
    import torch
    n = len(poses)
    cam, cams = _cams(rt, scenes, poses)
    cam.close()
    t = torch.zeros((n, H, W), dtype=torch.float32, device="cuda")
    inst, tri = (torch.full((n, H, W), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    img = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * n)(*[img[i].data_ptr() for i in range(n)])
    planes = rt.RtGBuffer(t=t.data_ptr(), instance=inst.data_ptr(), triangle=tri.data_ptr())
    before = sp.view_stats()
    rt.check(rt.libs()[0].rt_render_gbuffer(_handle(sp), cams, n, ptrs, W * 3, C.byref(planes), None, 1), "rt_render_gbuffer")
    after = sp.view_stats()
    assert after["launches"] == before["launches"] + 1 and after["fallbacks"] == before["fallbacks"], (before, after)
    return dict(t=t.cpu().numpy(), instance=inst.cpu().numpy(), triangle=tri.cpu().numpy(), image=img.cpu().numpy())


def batch(rt, scenes, sp, poses):
    """rt_render_batch itself: [n, H, W, 3]; asserts that the launch took a view slot"""
    import torch
    n = len(poses)
    cam, cams = _cams(rt, scenes, poses)
    cam.close()
    img = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
    ptrs = (C.c_void_p * n)(*[img[i].data_ptr() for i in range(n)])
    before = sp.view_stats()
    rt.check(rt.libs()[0].rt_render_batch(_handle(sp), cams, ptrs, C.c_size_t(W * 3), C.c_int32(n), None, C.c_int(1)), "rt_render_batch")
    after = sp.view_stats()
    assert after["launches"] == before["launches"] + 1 and after["fallbacks"] == before["fallbacks"], (before, after)
    return img.cpu().numpy()


def loop_stats(rt, scenes, sp, poses):
    """rt_scene_loop_stats of the batch: the instrumented copy of the production kernel, same launch decisions, same views"""
    import torch
    cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
    img = torch.zeros((len(poses), H, W, 3), dtype=torch.uint8, device="cuda")
    st = rt.Scene.loop_stats(sp, cam, poses, [img[i].data_ptr() for i in range(len(poses))], W * 3)
    cam.close()
    return st


def mesh_origin(pose, scale, camera_xyz):
    """the camera's position in an instance's mesh space: to_mesh_space's operations on float32 -- subtract the instance's position,
    rotate by euler2quat(pose ypr), multiply by 1 / scale"""
    import orc
    o = orc.oracle()
    q = o.euler2quat(np.array(pose[3:6], F32))
    v = o.apply_quat(q, np.array(camera_xyz, F32) - np.array(pose[:3], F32))
    return (np.asarray(v, F32) * (F32(1.0) / np.array(scale, F32))).astype(F32)


def planes_hash(g):
    return hashlib.sha256(b"".join(np.ascontiguousarray(g[k]).tobytes() for k in ("t", "instance", "triangle"))).hexdigest()


def expected_culled(tris, tree, origin):
    """the leaf children the rule culls for an identity instance seen from `origin`: leaves of one to four triangles with
    N = ((v0 - o).x * n.x + (v0 - o).y * n.y) + (v0 - o).z * n.z >= 2^-20 for every triangle, in float32 throughout"""
    o = np.asarray(origin, F32)
    d = tris[:, 0:3].astype(F32) - o
    n = tris[:, 9:12].astype(F32)
    N = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    assert N.dtype == F32
    count = 0
    for node in range(1, len(tree["node_children"])):                # (node 0 is the root: nobody's child)
        if ct.is_leaf(tree, node):
            idx = ct.leaf_triangles(tree, node)
            count += 1 <= len(idx) <= 4 and bool((N[idx] >= K_CULL).all())
    return count, N


CHILD = """
import importlib, sys
sys.path.insert(0, 'tests')
import test_gpu_view_cull as t
rt = importlib.import_module('cuda-raytracing_amd'); scenes = importlib.import_module('cuda-raytracing_amd.scenes'); rt.build()
for name, make in t.CASES.items():
    c = make(rt)
    g = t.gbuffer(rt, scenes, c['sp'], c['poses'])
    print('PLANES', name, t.planes_hash(g), len(c['sp'].view_cull_stats()), t.loop_stats(rt, scenes, c['sp'], c['poses'])['cpp_iters'])
"""


@pytest.fixture(scope="module")
def unculled(rt):
    """{case: sha256 of its t, instance and triangle planes} from one child process with RT_VIEW_CULL=0, whose views held no culled box"""
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=dict(os.environ, RT_VIEW_CULL="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("PLANES")]
    assert sorted(ln[1] for ln in lines) == sorted(CASES) and all(ln[3] == "0" for ln in lines), lines
    return {ln[1]: (ln[2], int(ln[4])) for ln in lines}


@pytest.fixture(scope="module")
def built(rt):
    """every case's scene, built once"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = CASES[name](rt)
        return made[name]
    yield get
    for c in made.values():
        c["sp"].close()


def _check(rt, scenes, c, name, unculled):
    sp, poses = c["sp"], c["poses"]
    cam = rt.Camera(W, H, scenes.scaled_K(W), scenes.D_REF)
    want = []
    for ps in poses:
        cam.set_pose(ps)
        want.append(rt.render_debug(sp, cam))
    cam.close()
    frames = batch(rt, scenes, sp, poses)
    culled_batch = sp.view_cull_stats()
    g = gbuffer(rt, scenes, sp, poses)
    culled = sp.view_cull_stats()
    assert len(culled) == len(poses) and culled == culled_batch, (culled, culled_batch)
    for k, ref in enumerate(want):
        assert np.array_equal(frames[k], ref["img"]), "%s: frame %d of the batch differs in %d pixels" % (name, k, int((frames[k] != ref["img"]).any(axis=2).sum()))
        assert np.array_equal(g["image"][k], ref["img"]), "%s: image %d of the G-buffer differs" % (name, k)
        assert np.array_equal(g["instance"][k], ref["hit_inst"]) and np.array_equal(g["triangle"][k], ref["hit_tri"]), "%s: hit ids of frame %d" % (name, k)
    assert len({f.tobytes() for f in frames}) == len(poses)            # (every pose shows something of its own)
    assert planes_hash(g) == unculled[name][0], "%s: t / instance / triangle differ from the RT_VIEW_CULL=0 process" % name
    if c["known"] is not None:
        tris, tree = c["known"]
        expect = [expected_culled(tris, tree, ps[:3])[0] for ps in poses]
        print(name, "culled leaf children per frame", culled, "numpy", expect)
        assert culled == expect, (name, culled, expect)
    return g, culled


def _oracle_planes(orc, scenes, desc, poses):
    import gbuffer_oracle
    so = desc.build_oracle(orc)
    ref = gbuffer_oracle.frames(so, W, H, scenes.scaled_K(W), scenes.D_REF, poses)
    so.close()
    return ref


def test_sphere_from_outside(rt, orc, scenes, built, unculled):
    """The far half of a closed sphere faces away from every camera outside it: those leaves are culled, in the number the rule gives;
    the planes are the oracle's."""
    c = built("sphere")
    g, culled = _check(rt, scenes, c, "sphere", unculled)
    assert all(n > 20 for n in culled), culled
    ref = _oracle_planes(orc, scenes, c["desc"], c["poses"])
    for k in ("t", "instance", "triangle"):
        assert np.array_equal(g[k].view(np.int32), ref[k].view(np.int32)), k
    assert (g["instance"] >= 0).any() and (g["instance"] < 0).any()


def test_camera_inside_a_room(rt, scenes, built, unculled):
    """The walls face the camera and stay; the outer faces of the same walls can never be accepted and go."""
    _, culled = _check(rt, scenes, built("room"), "room", unculled)
    assert all(n > 0 for n in culled), culled


def test_coincident_in_plane_and_denormal(rt, orc, scenes, built, unculled):
    """Two coincident triangles with opposite normals (one is hit, its twin's leaf may go); a triangle whose plane holds the camera
    (N = 0) and one with N = 1e-40: below 2^-20, so neither counts as facing away.  The planes are the oracle's."""
    c = built("specials")
    tris, tree = c["known"]
    for ps in c["poses"]:
        N = expected_culled(tris, tree, ps[:3])[1]
        assert N[0] < 0 < N[1] and N[1] >= K_CULL                      # the twins
        assert N[2] == 0 and 0 < N[3] < F32(1e-38) and N[4] >= K_CULL and N[5] >= K_CULL, N[:6]
    g, culled = _check(rt, scenes, c, "specials", unculled)
    assert all(n > 0 for n in culled), culled
    ref = _oracle_planes(orc, scenes, c["desc"], c["poses"])
    for k in ("t", "instance", "triangle"):
        assert np.array_equal(g[k].view(np.int32), ref[k].view(np.int32)), k
    assert (g["triangle"] == 0).any() and not (g["triangle"] == 1).any()   # the twin that faces the camera is seen, the other never


def test_leaves_of_five_and_of_more_than_thirty(rt, scenes, built, unculled):
    """A caller's tree with leaves of 1, 2, 4, 5 and 31 and more triangles: the rule looks at one to four coded triangles and leaves
    every other leaf alone, whatever its triangles face."""
    c = built("leaves")
    tris, tree = c["known"]
    sizes = tree["node_leaf_count"][tree["node_children"][:, 0] <= 0]
    _, culled = _check(rt, scenes, c, "leaves", unculled)
    assert all(0 < n < int((sizes <= 4).sum()) for n in culled), (culled, sizes)


def test_translated_and_posed_instances(rt, scenes, built, unculled):
    """The rule is evaluated in mesh space, with the origin the ray header holds: a translation, a rotation with a non-uniform scale.
    The count is the rule's at the camera's position in each instance's mesh space (no N of these spheres is near 2^-20: the last bit
    of that origin does not decide a leaf)."""
    c = dict(built("posed"))
    tris, tree = c["known"]
    c["known"] = None
    _, culled = _check(rt, scenes, c, "posed", unculled)
    expect = []
    for ps in c["poses"]:
        per = [expected_culled(tris, tree, mesh_origin(pose, scale, ps[:3])) for _, _, pose, scale in POSED]
        assert all(float(np.abs(N).min()) > 1e-5 for _, N in per)
        expect.append(sum(n for n, _ in per))
    print("posed culled leaf children per frame", culled, "numpy", expect)
    assert culled == expect and all(n > 200 for n in culled), (culled, expect)


def test_tree_deeper_than_the_lds_stack(rt, scenes, built, unculled):
    """Lanes that outgrow the LDS stack are traced again through the same, culled, views."""
    c = built("deep")
    _, culled = _check(rt, scenes, c, "deep", unculled)
    assert all(n > 100 for n in culled), culled                        # (the far half of the sphere beside the chain)
    st = loop_stats(rt, scenes, c["sp"], c["poses"])
    assert st["deep"] > 0 and st["retraced_lanes"] > 0, st


@pytest.mark.parametrize("name", ["unordered", "sphere"])
def test_generic_slab_loop_skips_culled_children(rt, scenes, built, unculled, name):
    """The compiler's generic loop sorts the two plane products of an axis, so a box of +inf / -inf planes would pass it for every
    ray and every culled leaf would be visited by rays that miss its real box; pixels cannot show that.  Two kinds of waves take that
    loop through view records: every wave of a mesh flagged unordered (a caller's tree with empty leaves), and, on any mesh, the
    waves whose rays straddle a sign change of the direction.  Their lanes' iterations, counted by the instrumented copy of the
    production kernel, must fall below those of a process that culls nothing."""
    c = built(name)
    if name == "unordered":
        _check(rt, scenes, c, name, unculled)
    st = loop_stats(rt, scenes, c["sp"], c["poses"])
    assert len(c["sp"].view_cull_stats()) == len(c["poses"])          # (the stats launch read culled views)
    print(name, "iterations on the compiler's loops", st["cpp_iters"], "without the cull", unculled[name][1], st)
    assert st["cpp_generic"] > 0 and (name != "unordered" or st["asm"] == 0), st
    assert 0 < st["cpp_iters"] < unculled[name][1], (st, unculled[name])


def test_samples_only_extension_kernel_reads_unculled_views(rt, orc, scenes, built):
    """The samples-only extension kernel reports node pops, pinned to the oracle's: its launch takes views (4 spp of one frame) and they
    hold every box as it is -- the pops plane is the oracle's, and the scene's last pre-pass wrote no culled view."""
    c = built("sphere")
    sp, pose = c["sp"], OUTSIDE[0]
    K = scenes.scaled_K(W)
    so = c["desc"].build_oracle(orc)
    ref = so.render_ex(W, H, K, scenes.D_REF, pose, 4, 0, 0, threads=8)
    so.close()
    batch(rt, scenes, sp, OUTSIDE)
    assert len(sp.view_cull_stats()) == 4
    cam = rt.Camera(W, H, K, scenes.D_REF)
    cam.set_pose(pose)
    cam.set_options(4, 0, 0)
    before = sp.view_stats()
    got = rt.render_ex(sp, cam)
    cam.close()
    after = sp.view_stats()
    assert after["launches"] == before["launches"] + 1 and after["fallbacks"] == before["fallbacks"], (before, after)
    assert sp.view_cull_stats() == []
    assert np.array_equal(got["img"], ref["img"]) and np.array_equal(got["total_pops"], ref["total_pops"])
    assert int(got["total_pops"].max()) > 4 * 5
