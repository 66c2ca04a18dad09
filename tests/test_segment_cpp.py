"""Scene::closest_to_segments (cuda-raytracing_amd/csrc/host/) compiles and links against the two libraries as a C++ user sees them,
and refuses what the C ABI refuses: no device scene, and through rt_closest_to_segments itself a NULL scene, n < 0, NULL segments and
no output at all (no GPU is touched)."""
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
    RtSegmentHits out = {};
    float distance[4], clearance[4], segment_point[4 * 3];
    int32_t within[4], crossings[4];
    out.distance = distance; out.clearance = clearance; out.segment_point = segment_point; out.within = within; out.crossings = crossings;
    float segments[4 * 6] = {};
    const int a = scene.closest_to_segments(segments, nullptr, 4, out);
    const int b = scene.last_error;
    RtScene* bogus = reinterpret_cast<RtScene*>(16);        // a handle that is never dereferenced
    RtSegmentHits none = {};
    const int c = rt_closest_to_segments(nullptr, segments, nullptr, 4, &out, nullptr, 0);
    const int d = rt_closest_to_segments(bogus, segments, nullptr, -1, &out, nullptr, 0);
    const int e = rt_closest_to_segments(bogus, nullptr, nullptr, 4, &out, nullptr, 0);
    const int f = rt_closest_to_segments(bogus, segments, nullptr, 4, &none, nullptr, 0);
    const int g = rt_closest_to_segments(bogus, segments, nullptr, 4, nullptr, nullptr, 0);
    const int h = rt_closest_to_segments(bogus, nullptr, nullptr, 0, nullptr, nullptr, 0);      // nothing to do: RT_OK
    printf("%d %d %d %d %d %d %d %d %d\n", a, b, c, d, e, f, g, h, rt_abi_version());
    return 0;
}
"""


def test_scene_member_compiles_links_and_refuses_what_the_c_abi_refuses(rt, tmp_path):
    src, exe = tmp_path / "segments.cpp", tmp_path / "segments"
    src.write_text(PROGRAM)
    _gxx(str(src), str(exe))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["-1", "-1", "-1", "-1", "-1", "-1", "-1", "0", "2"], r.stdout
