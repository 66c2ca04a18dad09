"""Camera::render_gbuffer (cuda-raytracing_amd/csrc/host/) compiles and links against the two libraries as a C++ user sees them, and
refuses what the C ABI refuses: no poses, more than RT_MAX_BATCH poses, a scene without a device scene, and through rt_render_gbuffer
itself NULL arguments, a count out of range, no output at all, a NULL image and a short pitch (no GPU is touched)."""
import os
import subprocess

from test_host_cpp_api import _gxx

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "Camera.h"
#include "Scene.h"
#include "rt_hip.h"
int main()
{
    Scene scene;                                   // never uploaded: no device scene
    float3x3 K = {};
    K.m[0][0] = K.m[1][1] = 20.0f; K.m[0][2] = 8.0f; K.m[1][2] = 4.0f; K.m[2][2] = 1.0f;
    Camera cam(16, 8, K, make_float4(0, 0, 0, 0));
    RtGBuffer out = {}, none = {};
    float t[2 * 16 * 8];
    out.t = t;
    std::vector<lre> two(2), many(RT_MAX_BATCH + 1), empty;
    const int a = cam.render_gbuffer(scene, empty, out);
    const int b = cam.render_gbuffer(scene, many, out);
    const int c = cam.render_gbuffer(scene, two, out);
    const int d = cam.last_error;
    RtScene* bogus = reinterpret_cast<RtScene*>(16);        // a handle that is never dereferenced
    RtCameraParams p[2] = {};
    p[0].width = p[1].width = 16; p[0].height = p[1].height = 8;
    uint8_t* imgs[2] = {reinterpret_cast<uint8_t*>(64), nullptr};
    const int e = rt_render_gbuffer(nullptr, p, 2, nullptr, 0, &out, nullptr, 0);
    const int f = rt_render_gbuffer(bogus, nullptr, 2, nullptr, 0, &out, nullptr, 0);
    const int g = rt_render_gbuffer(bogus, p, 2, nullptr, 0, nullptr, nullptr, 0);
    const int h = rt_render_gbuffer(bogus, p, 0, nullptr, 0, &out, nullptr, 0);
    const int i = rt_render_gbuffer(bogus, p, 2, nullptr, 0, &none, nullptr, 0);
    const int j = rt_render_gbuffer(bogus, p, 2, imgs, 48, &out, nullptr, 0);
    const int k = rt_render_gbuffer(bogus, p, 1, imgs, 47, &out, nullptr, 0);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", a, b, c, d, e, f, g, h, i, j, k, rt_abi_version());
    return 0;
}
"""


def test_camera_member_compiles_links_and_refuses_what_the_c_abi_refuses(rt, tmp_path):
    src, exe = tmp_path / "gbuffer.cpp", tmp_path / "gbuffer"
    src.write_text(PROGRAM)
    _gxx(str(src), str(exe))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, HIP_VISIBLE_DEVICES=""))
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["-1"] * 11 + ["2"], r.stdout
