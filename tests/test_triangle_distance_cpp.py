"""Scene::closest_to_triangles (cuda-raytracing_amd/csrc/host/) compiles and links against the two libraries as a C++ user sees them,
and refuses what the C ABI refuses: no device scene, and through rt_closest_to_triangles itself a NULL scene, n < 0, NULL triangles
and no output at all (no GPU is touched)."""
import os
import subprocess

from test_host_cpp_api import _gxx

PROGRAM = r"""
#include <cstdio>
#include "Scene.h"
#include "rt_hip.h"
int main()
{
    Scene scene;                                   // never uploaded: no device scene
    RtTriangleHits out = {};
    float distance[4], clearance[4], query_point[4 * 3], query_barycentric[4 * 2];
    int32_t within[4], intersections[4], skip[4] = {-1, -1, -1, -1};
    out.distance = distance; out.clearance = clearance; out.query_point = query_point; out.query_barycentric = query_barycentric;
    out.within = within; out.intersections = intersections;
    float triangles[4 * 9] = {};
    const int a = scene.closest_to_triangles(triangles, nullptr, skip, 4, out);
    const int b = scene.last_error;
    RtScene* bogus = reinterpret_cast<RtScene*>(16);        // a handle that is never dereferenced
    RtTriangleHits none = {};
    const int c = rt_closest_to_triangles(nullptr, triangles, nullptr, nullptr, 4, &out, nullptr, 0);
    const int d = rt_closest_to_triangles(bogus, triangles, nullptr, nullptr, -1, &out, nullptr, 0);
    const int e = rt_closest_to_triangles(bogus, nullptr, nullptr, nullptr, 4, &out, nullptr, 0);
    const int f = rt_closest_to_triangles(bogus, triangles, nullptr, skip, 4, &none, nullptr, 0);
    const int g = rt_closest_to_triangles(bogus, triangles, nullptr, nullptr, 4, nullptr, nullptr, 0);
    const int h = rt_closest_to_triangles(bogus, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0);    // nothing to do: RT_OK
    printf("%d %d %d %d %d %d %d %d %d\n", a, b, c, d, e, f, g, h, rt_abi_version());
    return 0;
}
"""


def test_scene_member_compiles_links_and_refuses_what_the_c_abi_refuses(rt, tmp_path):
    src, exe = tmp_path / "triangle_distance.cpp", tmp_path / "triangle_distance"
    src.write_text(PROGRAM)
    _gxx(str(src), str(exe))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["-1", "-1", "-1", "-1", "-1", "-1", "-1", "0", "2"], r.stdout
