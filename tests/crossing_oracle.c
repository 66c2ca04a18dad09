/* crossing_oracle.c -- TEST INFRASTRUCTURE: brute-force ray crossing counts, winding numbers and signed distance over a scene, the
 * specification of rt_count_crossings / rt_winding_numbers / rt_signed_distance (include/rt_hip.h).  It
 * includes oracle/rt_oracle.c unchanged for its scene (OrcScene) and apply_lre / apply_euler, and restates the fp32 sequence of the
 * rule on its own -- no header is shared with the kernel, so an error in either copy shows as a difference.  Every (instance,
 * triangle) is visited; there is no tree.  The signed distance's magnitude comes from tests/point_oracle.c (its own shim), passed in
 * by the caller.  Built by tests/crossing_oracle.py with the oracle's own flags (oracle/Makefile: -ffp-contract=off). */
#include "../oracle/rt_oracle.c"

static const float xo_dirs[3][3] = {{0x1.24b5dcp-1f, 0x1.3e5c92p-2f, 0x1.84c2f8p-1f},
                                    {-0x1.3f212ep-1f, 0x1.6d9e84p-1f, 0x1.46594ap-2f},
                                    {0x1.2809d4p-2f, 0x1.488ce8p-1f, -0x1.6bac72p-1f}};

/* an fp64 edge function to fp32 with its exact sign: a nonzero value that rounds to 0 becomes the smallest subnormal of that sign */
static float xo_narrow(double x)
{
    float f = (float)x;
    if (f == 0.0f && x > 0.0) return 0x1p-149f;
    if (f == 0.0f && x < 0.0) return -0x1p-149f;
    return f;
}

static float xo_c(f3 v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

/* rule 3 on the triangle (a, a + ab, a + ac) for o' / d' in scaled mesh space: 0 = not counted, else the sign; *t = the t found */
static int xo_triangle(f3 o, f3 d, f3 a, f3 ab, f3 ac, float tmax, float *tout)
{
    f3 b = mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z), c = mk3(a.x + ac.x, a.y + ac.y, a.z + ac.z);
    float adx = fabsf(d.x), ady = fabsf(d.y), adz = fabsf(d.z), big = adx, dz, sx, sy, sz;
    float pa[3], pb[3], pc[3], ax, ay, bx, by, cx, cy, U, V, W, det, T, t;
    int kz = 0, kx, ky, tmp;
    if (ady > big) { kz = 1; big = ady; }
    if (adz > big) kz = 2;
    kx = (kz + 1) % 3; ky = (kx + 1) % 3;
    dz = xo_c(d, kz);
    if (dz == 0.0f) return 0;
    if (dz < 0.0f) { tmp = kx; kx = ky; ky = tmp; }
    sx = xo_c(d, kx) / dz; sy = xo_c(d, ky) / dz; sz = 1.0f / dz;
    pa[0] = xo_c(a, kx) - xo_c(o, kx); pa[1] = xo_c(a, ky) - xo_c(o, ky); pa[2] = xo_c(a, kz) - xo_c(o, kz);
    pb[0] = xo_c(b, kx) - xo_c(o, kx); pb[1] = xo_c(b, ky) - xo_c(o, ky); pb[2] = xo_c(b, kz) - xo_c(o, kz);
    pc[0] = xo_c(c, kx) - xo_c(o, kx); pc[1] = xo_c(c, ky) - xo_c(o, ky); pc[2] = xo_c(c, kz) - xo_c(o, kz);
    ax = pa[0] - sx * pa[2]; ay = pa[1] - sy * pa[2];
    bx = pb[0] - sx * pb[2]; by = pb[1] - sy * pb[2];
    cx = pc[0] - sx * pc[2]; cy = pc[1] - sy * pc[2];
    U = cx * by - cy * bx; V = ax * cy - ay * cx; W = bx * ay - by * ax;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        U = xo_narrow((double)cx * (double)by - (double)cy * (double)bx);
        V = xo_narrow((double)ax * (double)cy - (double)ay * (double)cx);
        W = xo_narrow((double)bx * (double)ay - (double)by * (double)ax);
    }
    if (!((U >= 0.0f && V >= 0.0f && W >= 0.0f) || (U <= 0.0f && V <= 0.0f && W <= 0.0f))) return 0;
    det = (U + V) + W;
    if (det == 0.0f) return 0;
    T = (U * (sz * pa[2]) + V * (sz * pb[2])) + W * (sz * pc[2]);
    t = T / det;
    if (!(t > 0.0f && t <= tmax)) return 0;
    if (tout) *tout = t;
    return det < 0.0f ? 1 : -1;
}

static void xo_tri(const tri_t *t, f3 s, f3 *a, f3 *ab, f3 *ac)
{
    f3 e1 = mk3(t->v[1].x - t->v[0].x, t->v[1].y - t->v[0].y, t->v[1].z - t->v[0].z);
    f3 e0 = mk3(t->v[2].x - t->v[0].x, t->v[2].y - t->v[0].y, t->v[2].z - t->v[0].z);
    *a = mk3(t->v[0].x * s.x, t->v[0].y * s.y, t->v[0].z * s.z);
    *ab = mk3(e1.x * s.x, e1.y * s.y, e1.z * s.z);
    *ac = mk3(e0.x * s.x, e0.y * s.y, e0.z * s.z);
}

/* one ray: count, winding; ts (optional, room for cap values): the counted t, in (instance, triangle) order; returns the count */
static int xo_ray(const OrcScene *sc, f3 w, f3 dw, float tmax, int32_t *winding, float *ts, int cap)
{
    int i, k, count = 0, wn = 0;
    for (i = 0; i < sc->ninst; i++) {
        const instance_t *in = &sc->instances[i];
        const OrcMesh *m = sc->meshes[in->mesh_index];
        f3 o = apply_lre(in->pose, w);
        f3 d = apply_euler(mk3(in->pose.yaw, in->pose.pitch, in->pose.roll), dw);
        for (k = 0; k < m->ntris; k++) {
            f3 a, ab, ac;
            float t = 0.0f;
            int sg;
            xo_tri(&m->tris[k], in->scale, &a, &ab, &ac);
            sg = xo_triangle(o, d, a, ab, ac, tmax, &t);
            if (!sg) continue;
            if (ts && count < cap) ts[count] = t;
            count++;
            wn += sg;
        }
    }
    *winding = wn;
    return count;
}

/* n rays org / dir [n][3], tmax [n] (NULL = +inf) -> count / winding [n] (each optional) */
void orcx_count_crossings(const OrcScene *sc, int64_t n, const float *org, const float *dir, const float *tmax, int32_t *count,
                          int32_t *winding)
{
    int64_t j;
    for (j = 0; j < n; j++) {
        int32_t wn;
        int c = xo_ray(sc, mk3(org[3 * j], org[3 * j + 1], org[3 * j + 2]), mk3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]),
                       tmax ? tmax[j] : INFINITY, &wn, NULL, 0);
        if (count) count[j] = c;
        if (winding) winding[j] = wn;
    }
}

/* the counted t of one ray (unsorted, up to cap); returns the count */
int orcx_crossing_ts(const OrcScene *sc, const float *org, const float *dir, float tmax, float *ts, int cap)
{
    int32_t wn;
    return xo_ray(sc, mk3(org[0], org[1], org[2]), mk3(dir[0], dir[1], dir[2]), tmax, &wn, ts, cap);
}

/* n points [n][3] -> winding [n] (the median of the three directions' windings), per3 [n][3] (optional: each direction's) */
void orcx_winding_numbers(const OrcScene *sc, int64_t n, const float *pts, int32_t *winding, int32_t *per3)
{
    int64_t j;
    for (j = 0; j < n; j++) {
        f3 p = mk3(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]);
        int32_t w[3], lo, hi;
        int k;
        for (k = 0; k < 3; k++) xo_ray(sc, p, mk3(xo_dirs[k][0], xo_dirs[k][1], xo_dirs[k][2]), INFINITY, &w[k], NULL, 0);
        lo = w[0] < w[1] ? w[0] : w[1];
        hi = w[0] < w[1] ? w[1] : w[0];
        winding[j] = hi < w[2] ? hi : (lo > w[2] ? lo : w[2]);
        if (per3) { per3[3 * j] = w[0]; per3[3 * j + 1] = w[1]; per3[3 * j + 2] = w[2]; }
    }
}

/* the rule on one triangle given in scaled mesh space (host tests): o, d, a, ab, ac [3] -> sign (0 = not counted), *t */
int orcx_crossing_on_triangle(const float *o, const float *d, const float *a, const float *ab, const float *ac, float tmax, float *t)
{
    return xo_triangle(mk3(o[0], o[1], o[2]), mk3(d[0], d[1], d[2]), mk3(a[0], a[1], a[2]), mk3(ab[0], ab[1], ab[2]),
                       mk3(ac[0], ac[1], ac[2]), tmax, t);
}
