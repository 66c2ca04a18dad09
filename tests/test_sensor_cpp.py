"""Sensor (cuda-raytracing_amd/csrc/host/Sensor.h) compiles and links against the two libraries as a C++ user sees them, and refuses
what the C ABI refuses: bad directions at construction, and -- before any device call -- no poses, more than RT_MAX_BATCH poses and a
scene without a device scene; through the ray-table calls themselves NULL arguments, bad sizes, a count out of range and no output at
all.  Camera::directions refuses a NULL buffer.  No GPU is touched: the process sees no device, so a well-formed Sensor reports the
error that kept its table from being made and refuses every call with -1."""
import os
import subprocess

from test_host_cpp_api import _gxx

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "Camera.h"
#include "Scene.h"
#include "Sensor.h"
#include "rt_hip.h"
int main()
{
    Scene scene;                                   // never uploaded: no device scene
    std::vector<float> dirs(16 * 8 * 3, 0.0f);
    for (size_t i = 1; i < dirs.size(); i += 3) dirs[i] = 1.0f;
    Sensor null_dirs(nullptr, 16, 8), no_width(dirs.data(), 0, 8), no_height(dirs.data(), 16, -1);
    Sensor sensor(dirs.data(), 16, 8);             // no device in this process: the table cannot be made
    const int made = sensor.last_error != 0 && sensor.table() == nullptr;
    lre pose;
    pose.x = 1.0f; pose.yaw = 0.5f;
    sensor.set_pose(pose);
    sensor.set_stream(nullptr);
    RtGBuffer out = {}, none = {};
    float t[2 * 16 * 8];
    out.t = t;
    std::vector<lre> two(2), many(RT_MAX_BATCH + 1), empty;
    const int a = sensor.render_gbuffer(scene, empty, out);
    const int b = sensor.render_gbuffer(scene, many, out);
    const int c = sensor.render_gbuffer(scene, two, out);
    const int d = sensor.last_error;
    const int e = sensor.rays(t, t);
    const int f = sensor.render_gbuffer_on(nullptr, scene, two, out);
    RtScene* bogus = reinterpret_cast<RtScene*>(16);        // handles that are never dereferenced
    RtRayTable* tab = reinterpret_cast<RtRayTable*>(32);
    RtRayTable* got = nullptr;
    RtCameraParams p[2] = {};
    p[0].width = p[1].width = 16; p[0].height = p[1].height = 8;
    const int g = rt_render_gbuffer_table(bogus, nullptr, p, 2, nullptr, 0, &out, nullptr, 0);
    const int h = rt_render_gbuffer_table(nullptr, tab, p, 2, nullptr, 0, &out, nullptr, 0);
    const int i = rt_render_gbuffer_table(bogus, tab, p, 0, nullptr, 0, &out, nullptr, 0);
    const int j = rt_render_gbuffer_table(bogus, tab, p, 2, nullptr, 0, &none, nullptr, 0);
    const int k = rt_ray_table_create(nullptr, 16, 8, nullptr, 0, &got);
    const int l = rt_ray_table_create(t, 16, 0, nullptr, 0, &got);
    const int m = rt_ray_table_rays(nullptr, p, t, t, nullptr, 0);
    const int n = rt_ray_table_info(nullptr, nullptr, nullptr, nullptr);
    float3x3 K = {};
    K.m[0][0] = K.m[1][1] = 20.0f; K.m[0][2] = 8.0f; K.m[1][2] = 4.0f; K.m[2][2] = 1.0f;
    Camera cam(16, 8, K, make_float4(0, 0, 0, 0));
    const int o = cam.directions(nullptr);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", null_dirs.last_error, no_width.last_error, no_height.last_error, a, b, c, d,
           e, f, g, h, i, j, k, l, m, n, o, made, rt_ray_table_destroy(nullptr), rt_abi_version());
    return got == nullptr ? 0 : 1;
}
"""


def test_sensor_compiles_links_and_refuses_what_the_c_abi_refuses(rt, tmp_path):
    src, exe = tmp_path / "sensor.cpp", tmp_path / "sensor"
    src.write_text(PROGRAM)
    _gxx(str(src), str(exe))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["-1"] * 18 + ["1", "0", "2"], r.stdout
