"""Camera::point_cloud_offsets, Sensor::point_cloud_offsets and the free point_cloud_fill (Camera.h, Sensor.h) compile and link
against the two libraries as a C++ user sees them, and refuse what the C ABI refuses before any device call: no poses, more than
RT_MAX_BATCH poses, a scene without a device scene, a sensor without a table; through the C ABI itself a NULL workspace or offsets, a
short workspace, no field, unknown bits, a bad range gate, and for the fill a pointer whose plane was not staged, a negative capacity
and no output at all.  last_error stays what it was: the calls write nothing in the object.  No GPU is touched."""
import os
import subprocess

from test_host_cpp_api import _gxx

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#include "Camera.h"
#include "Scene.h"
#include "Sensor.h"
#include "rt_hip.h"
int main()
{
    Scene scene;                                   // never uploaded: no device scene
    float3x3 K = {};
    K.m[0][0] = K.m[1][1] = 20.0f; K.m[0][2] = 8.0f; K.m[1][2] = 4.0f; K.m[2][2] = 1.0f;
    Camera cam(16, 8, K, make_float4(0, 0, 0, 0));
    const Camera& shared = cam;                    // (const: the call writes nothing in the camera)
    std::vector<float> dirs(16 * 8 * 3, 0.0f);
    for (size_t i = 1; i < dirs.size(); i += 3) dirs[i] = 1.0f;
    Sensor sensor(dirs.data(), 16, 8);             // no device in this process: the table cannot be made
    const int sensor_error = sensor.last_error;
    std::vector<lre> two(2), many(RT_MAX_BATCH + 1), empty;
    char* ws = reinterpret_cast<char*>(4096);      // device pointers that are never dereferenced
    int64_t* off = reinterpret_cast<int64_t*>(8192);
    const size_t bytes = rt_point_cloud_workspace_bytes(16, 8, 2, RT_CLOUD_ALL);
    const float inf = INFINITY;
    const int a = shared.point_cloud_offsets(nullptr, scene, empty, 0.0f, inf, nullptr, RT_CLOUD_RANGE, off, ws, bytes);
    const int b = shared.point_cloud_offsets(nullptr, scene, many, 0.0f, inf, nullptr, RT_CLOUD_RANGE, off, ws, bytes);
    const int c = shared.point_cloud_offsets(nullptr, scene, two, 0.0f, inf, nullptr, RT_CLOUD_RANGE, off, ws, bytes);   // no device scene
    const int d = sensor.point_cloud_offsets(nullptr, scene, two, 0.0f, inf, nullptr, RT_CLOUD_RANGE, off, ws, bytes);   // no table
    const int kept = cam.last_error == 0 && sensor.last_error == sensor_error;
    RtPointCloud out = {}, none = {}, foreign = {};
    out.range = reinterpret_cast<float*>(16384);
    foreign.uv = reinterpret_cast<float*>(16384);
    const int e = point_cloud_fill(nullptr, 16, 8, empty, RT_CLOUD_RANGE, ws, bytes, 0, out);
    const int f = point_cloud_fill(nullptr, 16, 8, many, RT_CLOUD_RANGE, ws, bytes, 0, out);
    const int g = point_cloud_fill(nullptr, 16, 0, two, RT_CLOUD_RANGE, ws, bytes, 0, out);
    const int h = point_cloud_fill(nullptr, 16, 8, two, RT_CLOUD_RANGE, nullptr, bytes, 0, out);
    const int i = point_cloud_fill(nullptr, 16, 8, two, RT_CLOUD_RANGE, ws, 16, 0, out);
    const int j = point_cloud_fill(nullptr, 16, 8, two, 0, ws, bytes, 0, out);
    const int k = point_cloud_fill(nullptr, 16, 8, two, 0x200, ws, bytes, 0, out);
    const int l = point_cloud_fill(nullptr, 16, 8, two, RT_CLOUD_RANGE, ws, bytes, 0, foreign);
    const int m = point_cloud_fill(nullptr, 16, 8, two, RT_CLOUD_ALL, ws, bytes, 0, none);
    const int n = point_cloud_fill(nullptr, 16, 8, two, RT_CLOUD_RANGE, ws, bytes, -1, out);
    const int ok = point_cloud_fill(nullptr, 16, 8, two, RT_CLOUD_ALL, ws, bytes, 0, out);          // capacity 0: nothing to launch
    RtScene* bogus = reinterpret_cast<RtScene*>(16);        // a handle that is never dereferenced
    RtCameraParams p[2] = {};
    p[0].width = p[1].width = 16; p[0].height = p[1].height = 8;
    const int o = rt_point_cloud_offsets(bogus, p, 2, 0.0f, inf, nullptr, RT_CLOUD_RANGE, nullptr, ws, bytes, nullptr, 0);
    const int q = rt_point_cloud_offsets(bogus, p, 2, 0.0f, inf, nullptr, RT_CLOUD_RANGE, off, nullptr, bytes, nullptr, 0);
    const int r = rt_point_cloud_offsets(bogus, p, 2, 0.0f, inf, nullptr, RT_CLOUD_ALL, off, ws, bytes - 1, nullptr, 0);
    const int s = rt_point_cloud_offsets(bogus, p, 2, 0.0f, inf, nullptr, 0, off, ws, bytes, nullptr, 0);
    const int t = rt_point_cloud_offsets(bogus, p, 2, 2.0f, 1.0f, nullptr, RT_CLOUD_RANGE, off, ws, bytes, nullptr, 0);
    const int u = rt_point_cloud_offsets(bogus, p, 2, NAN, 1.0f, nullptr, RT_CLOUD_RANGE, off, ws, bytes, nullptr, 0);
    const int v = rt_point_cloud_offsets_table(bogus, nullptr, p, 2, 0.0f, inf, nullptr, RT_CLOUD_RANGE, off, ws, bytes, nullptr, 0);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", a, b, c, d, e, f, g, h, i, j, k, l, m, n, o, q, r, s, t, u, v,
           kept, ok, (int)(bytes > 2 * 16 * 8 * 40));
    return 0;
}
"""


def test_point_cloud_compiles_links_and_refuses_what_the_c_abi_refuses(rt, tmp_path):
    src, exe = tmp_path / "cloud.cpp", tmp_path / "cloud"
    src.write_text(PROGRAM)
    _gxx(str(src), str(exe))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["-1"] * 21 + ["1", "0", "1"], r.stdout
