/* point_cloud_oracle.c -- the `local` field of a point cloud (include/rt_hip.h, point clouds rule 5) on the CPU.  TEST INFRASTRUCTURE
 * ONLY.  Includes oracle/rt_oracle.c unchanged for its apply_lre (transforms.hpp:223-226) and returns all three components of
 * apply_lre(camera_pose, location).  No header is shared with the kernel. */
#include "../oracle/rt_oracle.c"

/* n points of ONE frame: location [n][3], pose6 = the frame's camera_pose -> local [n][3] */
void orcx_cloud_local(const float *pose6, long long n, const float *location, float *local)
{
    lre_t pose;
    long long i;
    memcpy(&pose, pose6, sizeof pose);
    for (i = 0; i < n; i++) {
        f3 l = apply_lre(pose, mk3(location[3 * i], location[3 * i + 1], location[3 * i + 2]));
        local[3 * i] = l.x; local[3 * i + 1] = l.y; local[3 * i + 2] = l.z;
    }
}
