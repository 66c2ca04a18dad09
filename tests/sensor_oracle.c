/* sensor_oracle.c -- the rays of a sensor's direction table (include/rt_hip.h, "sensor frames") on the CPU.  TEST INFRASTRUCTURE ONLY.
 * Includes oracle/rt_oracle.c unchanged and applies the last two steps of its camera_ray (rt_oracle.c:775-776) to the caller's
 * camera-space directions: normalize3(apply_euler(invert_lre(pose).ypr, c)), with the oracle's own functions.  No header is shared
 * with the kernel. */
#include "../oracle/rt_oracle.c"

/* n entries c [n][3] under pose6 -> origins [n][3] (the pose's position), directions [n][3] */
void orcx_sensor_rays(const float *pose6, long long n, const float *c, float *origins, float *directions)
{
    lre_t pose, inv;
    long long i;
    memcpy(&pose, pose6, sizeof pose);
    inv = invert_lre(pose);
    for (i = 0; i < n; i++) {
        f3 d = apply_euler(mk3(inv.yaw, inv.pitch, inv.roll), mk3(c[3 * i], c[3 * i + 1], c[3 * i + 2]));
        d = normalize3(d);
        origins[3 * i] = pose.x; origins[3 * i + 1] = pose.y; origins[3 * i + 2] = pose.z;
        directions[3 * i] = d.x; directions[3 * i + 1] = d.y; directions[3 * i + 2] = d.z;
    }
}

/* normalize3 alone, for the test that pins the shim */
void orcx_sensor_normalize(long long n, const float *c, float *out)
{
    long long i;
    for (i = 0; i < n; i++) {
        f3 d = normalize3(mk3(c[3 * i], c[3 * i + 1], c[3 * i + 2]));
        out[3 * i] = d.x; out[3 * i + 1] = d.y; out[3 * i + 2] = d.z;
    }
}
