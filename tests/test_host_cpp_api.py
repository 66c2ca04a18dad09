"""The host C++ mirror (cuda-raytracing_amd/csrc/host/) as a C++ user sees it, compiled with plain g++ in the CPU suite:

* the per-node BVHTree queries of the reference (cost / evaluate_split / grow_to_include, BVHTree.hpp:175-201, :294-361),
  to_device_compatible (:364-383) and transforms::test_all (transforms.hpp:238-290)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "cuda-raytracing_amd")


def _gxx(src, exe, extra=()):
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(PKG, "csrc", "host"), src, "-L" + PKG, "-lrt_host", "-lrt_hip", "-Wl,-rpath," + PKG, "-o", exe] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


BVH_PROGRAM = r"""
#include <cstdio>
#include <iostream>
#include <random>
#include "Material.hpp"
#include "MeshPrimitive.h"
#include "rt_hip.h"
#include "transforms.hpp"
int main(int argc, char** argv)
{
    if (argc > 1) { transforms::test_all(); return 0; }
    std::mt19937 gen(7);
    std::uniform_real_distribution<float> u(-1.0f, 1.0f);
    std::vector<TrianglePrimitive> tris;
    for (int i = 0; i < 700; i++) {
        float3 c = make_float3(u(gen) * 3, u(gen) * 2, u(gen));
        tris.push_back(TrianglePrimitive(make_float3(c.x + 0.2f * u(gen), c.y + 0.2f * u(gen), c.z + 0.2f * u(gen)),
                                         make_float3(c.x + 0.2f * u(gen), c.y + 0.2f * u(gen), c.z + 0.2f * u(gen)),
                                         make_float3(c.x + 0.2f * u(gen), c.y + 0.2f * u(gen), c.z + 0.2f * u(gen))));
    }
    for (int i = 0; i < 9; i++) tris.push_back(tris[3]);                 // duplicates: a leaf that cannot be split
    MeshPrimitive mesh(tris);
    const BVHTree& t = mesh.bvh_top;
    const TrianglePrimitive* T = mesh.triangle_array().data();
    int interior = 0, leaves = 0;
    for (int k = 0; k < (int)t.nodes.size(); k++) {
        const BVHNode& n = t.nodes[k];
        // the node's box is what grow_to_include gives over its triangles (BVHTree.hpp:206-209)
        BVHTree probe; probe.nodes.resize(1);
        probe.nodes[0].min = make_float3(FLT_MAX, FLT_MAX, FLT_MAX); probe.nodes[0].max = make_float3(-FLT_MAX, -FLT_MAX, -FLT_MAX);
        for (int i = 0; i < n.count; i++) probe.grow_to_include(0, T[t.order[n.first + i]]);
        if (memcmp(&probe.nodes[0].min, &n.min, 12) || memcmp(&probe.nodes[0].max, &n.max, 12)) { printf("bounds differ at node %d\n", k); return 1; }
        if (n.count <= 1) { leaves++; continue; }
        // the decision of BVHTree::fill (:218-246) from the reference's own per-axis evaluation
        std::pair<float, float> ex = t.evaluate_split(k, "x", T), ey = t.evaluate_split(k, "y", T), ez = t.evaluate_split(k, "z", T);
        int axis; float pos, best;
        if (ex.first < ey.first && ex.first < ez.first) { axis = 0; pos = ex.second; best = ex.first; }
        else if (ey.first < ex.first && ey.first < ez.first) { axis = 1; pos = ey.second; best = ey.first; }
        else { axis = 2; pos = ez.second; best = ez.first; }
        const bool is_leaf = n.child_index_a == -1 && n.child_index_b == -1;
        int nl = 0;
        for (int i = 0; i < n.count; i++) { float3 c = T[t.order[n.first + i]].center(); nl += (axis == 0 ? c.x : axis == 1 ? c.y : c.z) <= pos; }
        const bool splits = best < t.cost(k) && nl > 0 && nl < n.count;
        if (is_leaf) {
            leaves++;
            // (a leaf deeper than one triangle: the depth limit, or no plane that pays, or a one-sided partition)
            if (splits && t.max_level() < 32) { printf("node %d is a leaf but the evaluation splits it\n", k); return 1; }
            continue;
        }
        interior++;
        if (!splits) { printf("node %d is split but the evaluation would not\n", k); return 1; }
        const BVHNode& a = t.nodes[n.child_index_a]; const BVHNode& b = t.nodes[n.child_index_b];
        if (a.count != nl || b.count != n.count - nl || a.first != n.first || b.first != n.first + nl) { printf("partition differs at node %d\n", k); return 1; }
        for (int i = 0; i < a.count; i++) { float3 c = T[t.order[a.first + i]].center(); if (!((axis == 0 ? c.x : axis == 1 ? c.y : c.z) <= pos)) { printf("left side wrong at %d\n", k); return 1; } }
        for (int i = 0; i < b.count; i++) { float3 c = T[t.order[b.first + i]].center(); if ((axis == 0 ? c.x : axis == 1 ? c.y : c.z) <= pos) { printf("right side wrong at %d\n", k); return 1; } }
    }
    BVHTree::DeviceCompatible d = t.to_device_compatible();
    BVHTree::DeviceCompatible d2 = BVHTree::compile_tree(mesh.bvh_top);                 // BVHTree.hpp:364, the reference's name for it
    if (d2.node_bounds != d.node_bounds || d2.node_children != d.node_children || d2.leaf_indices != d.leaf_indices) { printf("compile_tree differs\n"); return 1; }
    // MeshPrimitive::to_device / Material::to_device (MeshPrimitive.h:36, Material.hpp:21) exist with the reference's names; without
    // a GPU the uploads fail cleanly (a null device scene / a null pointer), with one they succeed -- either way no crash
    d_MeshPrimitive* dm = mesh.to_device();
    if (!dm || dm->num_triangles != mesh.num_triangles) { printf("to_device gave no object\n"); return 1; }
    Material mat;
    Material* dmat = mat.to_device();
    int have_gpu = 0;
    rt_device_count(&have_gpu);
    if ((have_gpu > 0) != (dm->device != nullptr) || (have_gpu > 0) != (dmat != nullptr)) { printf("to_device and the device count disagree\n"); return 1; }
    if (dm->device) rt_scene_destroy(dm->device);
    if (dmat) rt_free(dmat);
    delete dm;
    if (d.node_bounds.size() != t.nodes.size() * 6 || d.node_children.size() != t.nodes.size() * 2 || d.leaf_indices.size() != tris.size()) return 1;
    long leaf_total = 0;
    for (size_t k = 0; k < t.nodes.size(); k++) leaf_total += d.node_leaf_count[k];
    if (leaf_total != (long)tris.size()) { printf("leaf counts do not add up\n"); return 1; }
    printf("OK nodes %d interior %d leaves %d\n", (int)t.nodes.size(), interior, leaves);
    return 0;
}
"""


def test_bvhtree_per_node_queries_and_transforms_self_check(rt, tmp_path):
    src = tmp_path / "bvh_queries.cpp"
    src.write_text("#include <cfloat>\n#include <cstring>\n" + BVH_PROGRAM)
    exe = str(tmp_path / "bvh_queries")
    _gxx(str(src), exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK nodes"), r.stdout + r.stderr
    interior, leaves = int(r.stdout.split()[4]), int(r.stdout.split()[6])
    assert interior > 300 and leaves == interior + 1
    # transforms::test_all prints the pose round trip of transforms.hpp:257-289; its "lre inv" line is invert_lre of the input pose
    r = subprocess.run([exe, "selftest"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0
    text = r.stdout
    for label in ("lre in:", "homo:", "inverted:", "lre inv:", "subtracted:", "Quat:", "vec out:"):
        assert label in text, label
    inv = np.zeros(6, np.float32)
    pose = np.array([0, 10, 0, 0, 0.5, 0], np.float32)
    import ctypes as C
    s = rt.libs()[1]
    s.rth_invert_lre(pose.ctypes.data_as(C.POINTER(C.c_float)), inv.ctypes.data_as(C.POINTER(C.c_float)))
    printed = [float(v) for v in text.split("lre inv:")[1].strip().splitlines()[0].replace(",", " ").split()]
    np.testing.assert_allclose(printed, inv, rtol=2e-5, atol=1e-6)


REFIT_PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include <hip/hip_vector_types.h>
#include "rt_hip.h"
#include "MeshPrimitive.h"
#include "Scene.h"
int main()
{
    std::vector<TrianglePrimitive> rest, moved;
    for (int i = 0; i < 50; i++) {
        const float f = 0.1f * (float)i;
        rest.push_back(TrianglePrimitive(make_float3(f, 0, 0), make_float3(f + 1, 0, 0), make_float3(f, 1, 0), make_float3(0, 0, 1),
                                         make_float2(0.01f * i, 0.2f), make_float2(0.3f, 0.02f * i), make_float2(0.5f, 0.6f)));
        moved.push_back(TrianglePrimitive(make_float3(f, 0, 2), make_float3(f + 1, 0, 2), make_float3(f, 1, 2.5f), make_float3(0, 0, 1),
                                          make_float2(9, 9), make_float2(8, 8), make_float2(7, 7)));   // other uvs: a refit must not take them
    }
    MeshPrimitive m(rest);
    if (!m.refit(moved)) { printf("refit refused\n"); return 1; }
    for (int i = 0; i < 50; i++) {
        const TrianglePrimitive& t = m.triangle_array()[(size_t)i];
        if (memcmp(t.vertices, moved[(size_t)i].vertices, sizeof t.vertices)) { printf("vertices of %d did not move\n", i); return 1; }
        if (memcmp(t.uv_coords, rest[(size_t)i].uv_coords, sizeof t.uv_coords)) { printf("uv of %d changed\n", i); return 1; }
    }
    // (the tree follows: the root's box now spans z = 2 .. 2.5)
    if (m.bvh_top.nodes[0].max.z != 2.5f || m.bvh_top.nodes[0].min.z != 2.0f) { printf("bounds were not refitted\n"); return 1; }
    std::vector<TrianglePrimitive> fewer(moved.begin(), moved.begin() + 10);
    if (m.refit(fewer)) { printf("a refit with another count was accepted\n"); return 1; }
    // A mesh made for a device build (no host tree yet), refitted before anything read its tree: the tree it gets at last is the one
    // built from the triangles it was made with, refitted -- what its device copy is rendered with -- not a new one over the moved
    // triangles.  (`moved` piles the triangles up differently: a builder run over it splits elsewhere.)
    for (int i = 0; i < 50; i++) for (int k = 0; k < 3; k++) moved[(size_t)i].vertices[k].x = 5.0f - moved[(size_t)i].vertices[k].x * (i % 7);
    MeshPrimitive late = MeshPrimitive::for_device_build(rest), early(rest), fresh(moved);
    if (!late.builds_at_upload()) { printf("a mesh made for a device build does not build at upload\n"); return 1; }
    late.refit(moved, true);
    if (late.builds_at_upload()) { printf("refitted since: it must go through sync_tree\n"); return 1; }
    late.sync_tree();
    early.refit(moved);
    const BVHTree &a = late.bvh_top, &b = early.bvh_top, &c = fresh.bvh_top;
    if (a.nodes.size() != b.nodes.size() || a.order != b.order) { printf("the late tree is not the early tree\n"); return 1; }
    for (size_t k = 0; k < a.nodes.size(); k++)
        if (a.nodes[k].child_index_a != b.nodes[k].child_index_a || a.nodes[k].child_index_b != b.nodes[k].child_index_b || a.nodes[k].first != b.nodes[k].first ||
            a.nodes[k].count != b.nodes[k].count || memcmp(&a.nodes[k].min, &b.nodes[k].min, 12) || memcmp(&a.nodes[k].max, &b.nodes[k].max, 12)) { printf("node %d differs\n", (int)k); return 1; }
    if (c.order == a.order && c.nodes.size() == a.nodes.size()) { printf("the probe does not tell the two trees apart\n"); return 1; }
    printf("OK\n");
    return 0;
}
"""


def test_refit_moves_vertices_and_keeps_texture_coordinates(rt, tmp_path):
    """Scene::refit_mesh / MeshPrimitive::refit: vertices and normals of the moved triangles are taken, texture coordinates stay -- the
    contract of rt_scene_refit_mesh ("uvs and the tree's topology stay", rt_hip.h), so that the host copy a later upload_to_device()
    sends is the mesh the refitted device copy renders (the GPU side: test_fuzz_adversarial_refit_and_rebuild)."""
    src = tmp_path / "refit.cpp"
    src.write_text(REFIT_PROGRAM)
    exe = str(tmp_path / "refit")
    _gxx(str(src), exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


def test_cmake_project_configures_and_builds(tmp_path):
    """CMakeLists.txt at the repository root (for C++ users; the reference is a CMake project too): configure with hipcc as the
    compiler and build both libraries and the two examples -- hipcc cross-compiles for gfx950, so this runs without a GPU."""
    import shutil
    if not shutil.which("cmake") or not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("cmake or hipcc not installed")
    b = str(tmp_path / "build")
    r = subprocess.run(["cmake", "-S", ROOT, "-B", b, "-DCMAKE_CXX_COMPILER=/opt/rocm/bin/hipcc"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    r = subprocess.run(["cmake", "--build", b, "-j", "4"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    for f in ("librt_hip.so", "librt_host.so", "demo_main", "tiled_main"):
        assert os.path.exists(os.path.join(b, f)), f
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(b, "librt_hip.so")], capture_output=True, text=True).stdout
    assert " rt_render\n" in syms and " rt_scene_rebuild_mesh_device\n" in syms
