"""Scene::sweep_spheres (cuda-raytracing_amd/csrc/host/) compiles and links against the two libraries as a C++ user sees them, and
refuses what the C ABI refuses: no device scene, and through rt_sweep_spheres itself a NULL scene, n < 0, NULL segments, a NULL radius
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
    RtSweepHits out = {};
    float time[4], centre[4 * 3], contact_normal[4 * 3];
    int32_t hit[4], triangle[4];
    out.time = time; out.centre = centre; out.contact_normal = contact_normal; out.hit = hit; out.triangle = triangle;
    float segments[4 * 6] = {}, radius[4] = {1, 1, 1, 1};
    const int a = scene.sweep_spheres(segments, radius, 4, out);
    const int b = scene.last_error;
    RtScene* bogus = reinterpret_cast<RtScene*>(16);        // a handle that is never dereferenced
    RtSweepHits none = {};
    const int c = rt_sweep_spheres(nullptr, segments, radius, 4, &out, nullptr, 0);
    const int d = rt_sweep_spheres(bogus, segments, radius, -1, &out, nullptr, 0);
    const int e = rt_sweep_spheres(bogus, nullptr, radius, 4, &out, nullptr, 0);
    const int f = rt_sweep_spheres(bogus, segments, nullptr, 4, &out, nullptr, 0);
    const int g = rt_sweep_spheres(bogus, segments, radius, 4, &none, nullptr, 0);
    const int h = rt_sweep_spheres(bogus, segments, radius, 4, nullptr, nullptr, 0);
    const int i = rt_sweep_spheres(bogus, nullptr, nullptr, 0, nullptr, nullptr, 0);      // nothing to do: RT_OK
    printf("%d %d %d %d %d %d %d %d %d %d\n", a, b, c, d, e, f, g, h, i, rt_abi_version());
    return 0;
}
"""


def test_scene_member_compiles_links_and_refuses_what_the_c_abi_refuses(rt, tmp_path):
    src, exe = tmp_path / "sweeps.cpp", tmp_path / "sweeps"
    src.write_text(PROGRAM)
    _gxx(str(src), str(exe))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["-1", "-1", "-1", "-1", "-1", "-1", "-1", "-1", "0", "2"], r.stdout
