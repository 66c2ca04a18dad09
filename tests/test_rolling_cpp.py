"""Sensor::render_rolling_on, Sensor::point_cloud_offsets_rolling, Sensor::rolling_slices and the free point_cloud_fill_rolling
(Sensor.h) compile and link against the two libraries as a C++ user sees them -- through a const Sensor -- and refuse what the C ABI
refuses before any device call: a sensor without a table, a scene without a device scene, a wrong number of poses, a bad axis or
slice_pixels; through the C ABI itself NULL arguments, a bad count, no output; for the fill a short workspace, a pointer whose plane
was not staged, a negative capacity.  last_error stays what it was.  No GPU is touched."""
import os
import subprocess

from test_host_cpp_api import _gxx

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#include "Scene.h"
#include "Sensor.h"
#include "rt_hip.h"
int main()
{
    Scene scene;                                   // never uploaded: no device scene
    std::vector<float> dirs(40 * 24 * 3, 0.0f);
    for (size_t i = 1; i < dirs.size(); i += 3) dirs[i] = 1.0f;
    Sensor made(dirs.data(), 40, 24);              // no device in this process: the table cannot be made
    const Sensor& sensor = made;                   // (const: the calls write nothing in the sensor)
    const int sensor_error = made.last_error;
    const int s0 = sensor.rolling_slices(0, 16), s1 = sensor.rolling_slices(1, 8), s2 = sensor.rolling_slices(0, 8);      // 3, 3, 5
    const int s3 = sensor.rolling_slices(2, 8), s4 = sensor.rolling_slices(0, 12), s5 = sensor.rolling_slices(1, 0);       // 0, 0, 0
    std::vector<lre> six(6), five(5), empty;
    char* ws = reinterpret_cast<char*>(4096);      // device pointers that are never dereferenced
    int64_t* off = reinterpret_cast<int64_t*>(8192);
    const size_t bytes = rt_rolling_workspace_bytes(2, 3);
    const size_t cbytes = rt_point_cloud_rolling_workspace_bytes(40, 24, 2, RT_CLOUD_ALL, 3);
    const float inf = INFINITY;
    RtGBuffer g = {};
    g.t = reinterpret_cast<float*>(16384);
    const int a = sensor.render_rolling_on(nullptr, scene, six, 2, 0, 16, g, nullptr, ws, bytes);       // no table, no device scene
    const int b = sensor.render_rolling_on(nullptr, scene, five, 2, 0, 16, g, nullptr, ws, bytes);      // a wrong number of poses
    const int c = sensor.render_rolling_on(nullptr, scene, empty, 0, 0, 16, g, nullptr, ws, bytes);
    const int d = sensor.render_rolling_on(nullptr, scene, six, 2, 2, 16, g, nullptr, ws, bytes);       // a bad axis
    const int e = sensor.render_rolling_on(nullptr, scene, six, 2, 0, 12, g, nullptr, ws, bytes);       // a bad slice_pixels
    const int f = sensor.point_cloud_offsets_rolling(nullptr, scene, six, 2, 0, 16, 0.0f, inf, nullptr, RT_CLOUD_RANGE, off, ws, cbytes);
    const int h = sensor.point_cloud_offsets_rolling(nullptr, scene, five, 2, 0, 16, 0.0f, inf, nullptr, RT_CLOUD_RANGE, off, ws, cbytes);
    const int kept = made.last_error == sensor_error;
    RtPointCloud out = {}, none = {}, foreign = {};
    out.range = reinterpret_cast<float*>(16384);
    foreign.uv = reinterpret_cast<float*>(16384);
    const int i = point_cloud_fill_rolling(nullptr, 40, 24, 2, 0, 16, RT_CLOUD_ALL, ws, cbytes - 1, 0, out);      // a short workspace
    const int j = point_cloud_fill_rolling(nullptr, 40, 24, 2, 0, 16, RT_CLOUD_RANGE, ws, cbytes, 0, foreign);
    const int k = point_cloud_fill_rolling(nullptr, 40, 24, 2, 0, 16, RT_CLOUD_ALL, ws, cbytes, 0, none);
    const int l = point_cloud_fill_rolling(nullptr, 40, 24, 2, 0, 16, RT_CLOUD_RANGE, ws, cbytes, -1, out);
    const int m = point_cloud_fill_rolling(nullptr, 40, 24, 2, 3, 16, RT_CLOUD_RANGE, ws, cbytes, 0, out);
    const int n = point_cloud_fill_rolling(nullptr, 40, 24, 2, 0, 20, RT_CLOUD_RANGE, ws, cbytes, 0, out);
    const int ok = point_cloud_fill_rolling(nullptr, 40, 24, 2, 0, 16, RT_CLOUD_ALL, ws, cbytes, 0, out);         // capacity 0: nothing to launch
    RtScene* bogus = reinterpret_cast<RtScene*>(16);        // handles that are never dereferenced
    const RtRayTable* table = reinterpret_cast<const RtRayTable*>(32);
    RtRollingPose p[6] = {};
    const int o = rt_render_gbuffer_rolling(nullptr, table, p, 2, 0, 16, nullptr, 0, &g, nullptr, ws, bytes, nullptr, 0);
    const int q = rt_render_gbuffer_rolling(bogus, nullptr, p, 2, 0, 16, nullptr, 0, &g, nullptr, ws, bytes, nullptr, 0);
    const int r = rt_render_gbuffer_rolling(bogus, table, nullptr, 2, 0, 16, nullptr, 0, &g, nullptr, ws, bytes, nullptr, 0);
    const int s = rt_render_gbuffer_rolling(bogus, table, p, 33, 0, 16, nullptr, 0, &g, nullptr, ws, bytes, nullptr, 0);
    const int t = rt_render_gbuffer_rolling(bogus, table, p, 2, 0, 16, nullptr, 0, &g, nullptr, nullptr, bytes, nullptr, 0);
    RtGBuffer nothing = {};
    const int u = rt_render_gbuffer_rolling(bogus, table, p, 2, 0, 16, nullptr, 0, &nothing, nullptr, ws, bytes, nullptr, 0);
    const int v = rt_point_cloud_offsets_rolling(bogus, table, p, 2, 0, 16, 2.0f, 1.0f, nullptr, RT_CLOUD_RANGE, off, ws, cbytes, nullptr, 0);
    printf("%d %d %d %d %d %d\n", s0, s1, s2, s3, s4, s5);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", a, b, c, d, e, f, h, i, j, k, l, m, n, o, q, r, s, t, u, v);
    printf("%d %d %d %d\n", kept, ok, (int)(bytes >= 2 * 3 * 48), (int)(cbytes == rt_point_cloud_workspace_bytes(40, 24, 2, RT_CLOUD_ALL) + bytes));
    return 0;
}
"""


def test_rolling_compiles_links_and_refuses_what_the_c_abi_refuses(rt, tmp_path):
    src, exe = tmp_path / "rolling.cpp", tmp_path / "rolling"
    src.write_text(PROGRAM)
    _gxx(str(src), str(exe))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().split("\n")
    assert lines[0].split() == ["3", "3", "5", "0", "0", "0"], r.stdout
    assert lines[1].split() == ["-1"] * 20, r.stdout
    assert lines[2].split() == ["1", "0", "1", "1"], r.stdout
