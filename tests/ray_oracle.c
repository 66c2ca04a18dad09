/* ray_oracle.c -- TEST INFRASTRUCTURE: the CPU oracle's cast of an ARBITRARY ray, for the ray-query tests (rt_trace_rays,
 * rt_occluded, rt_camera_rays).  oracle/rt_oracle.c exports whole frames only; its cast_ray_lp (raycast.cu:21-142) and camera_ray
 * (raycast.cu:156-188) are static, so this file includes it unchanged and exports thin loops over the two.  Built by
 * tests/ray_oracle.py with the oracle's own flags (oracle/Makefile); scenes are the oracle's OrcScene handles. */
#include "../oracle/rt_oracle.c"

/* n rays: org / dir [n][3]; lighting_pass / tmax (NULL = FLT_MAX) as cast_ray_lp takes them.  Every output may be NULL:
 * t [n] (HitInfo::min), inst / tri [n] (-1 on a miss), location / normal [n][3] (the accepted hit's, 0 on a miss), uv [n][2],
 * pops [n] (node pops). */
void orcx_cast_rays(const OrcScene *sc, int64_t n, const float *org, const float *dir, int lighting_pass, const float *tmax,
                    float *t, int32_t *inst, int32_t *tri, float *location, float *normal, float *uv, int32_t *pops)
{
    int64_t i;
    for (i = 0; i < n; i++) {
        ray_t ray = make_ray(mk3(org[3 * i], org[3 * i + 1], org[3 * i + 2]), mk3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]));
        hit_t hit = cast_ray_lp(&ray, sc, lighting_pass, tmax ? tmax[i] : FLT_MAX);
        if (t) t[i] = hit.min;
        if (inst) inst[i] = hit.hit_instance;
        if (tri) tri[i] = hit.hit_triangle;
        if (location) { location[3 * i] = hit.hit_location.x; location[3 * i + 1] = hit.hit_location.y; location[3 * i + 2] = hit.hit_location.z; }
        if (normal) { normal[3 * i] = hit.normal.x; normal[3 * i + 1] = hit.normal.y; normal[3 * i + 2] = hit.normal.z; }
        if (uv) { uv[2 * i] = hit.uv.x; uv[2 * i + 1] = hit.uv.y; }
        if (pops) pops[i] = hit.pops;
    }
}

/* the primary rays of pixel rows y0 .. y1 - 1, row-major (y * width + x) into org / dir [height * width][3] */
void orcx_camera_rays(int width, int height, const float *K9, const float *D4, const float *cam_pose6, int y0, int y1,
                      float *org, float *dir)
{
    camera_t cam; m33 K; int x, y;
    memcpy(&K, K9, sizeof K);
    cam.width = width; cam.height = height;
    cam.K_inv = invert_intrinsic(&K);                                              /* Camera.cu:12 */
    cam.D.x = D4[0]; cam.D.y = D4[1]; cam.D.z = D4[2]; cam.D.w = D4[3];
    memcpy(&cam.camera_pose, cam_pose6, sizeof(lre_t));
    cam.inv_camera_pose = invert_lre(cam.camera_pose);                             /* Camera.cu:21 */
    for (y = y0; y < y1; y++)
        for (x = 0; x < width; x++) {
            ray_t r = camera_ray(&cam, x, y);
            size_t p = 3 * ((size_t)y * (size_t)width + (size_t)x);
            org[p] = r.origin.x; org[p + 1] = r.origin.y; org[p + 2] = r.origin.z;
            dir[p] = r.direction.x; dir[p + 1] = r.direction.y; dir[p + 2] = r.direction.z;
        }
}
