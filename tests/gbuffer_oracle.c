/* gbuffer_oracle.c -- the `depth` plane of rt_render_gbuffer (include/rt_hip.h, G-buffer rule 2) on the CPU.  TEST INFRASTRUCTURE ONLY.
 * Includes oracle/rt_oracle.c unchanged for its apply_lre (transforms.hpp:223-226) and applies it to the locations the oracle's
 * cast_ray_lp returned: depth = apply_lre(camera_pose, location).z for a hit, FLT_MAX for a miss.  No header is shared with the
 * kernel. */
#include "../oracle/rt_oracle.c"

/* n pixels of ONE frame: location [n][3], instance [n] (-1 = miss), pose6 = the frame's camera_pose -> depth [n] */
void orcx_gbuffer_depth(const float *pose6, long long n, const float *location, const int *instance, float *depth)
{
    lre_t pose;
    long long i;
    memcpy(&pose, pose6, sizeof pose);
    for (i = 0; i < n; i++)
        depth[i] = instance[i] >= 0 ? apply_lre(pose, mk3(location[3 * i], location[3 * i + 1], location[3 * i + 2])).z : FLT_MAX;
}
