/* crossing_list_oracle.c -- TEST INFRASTRUCTURE: brute-force crossing lists over a scene, the specification of rt_crossing_offsets /
 * rt_list_crossings (include/rt_hip.h rule 8).  It includes tests/crossing_oracle.c unchanged (and through it
 * oracle/rt_oracle.c) for the scene, the per-instance maps and the counted set, and restates rule 3 once more so that the test also
 * returns U, V, W and det.  Every (instance, triangle) is visited, the pairs are sorted by (t, instance, triangle) and written into
 * the rooms.  Built by tests/crossing_list_oracle.py with the oracle's own flags (-ffp-contract=off). */
#include "crossing_oracle.c"

typedef struct { float t, b1, b2; int32_t inst, tri, sign; f2 uv; } xl_hit;

static f2 xl_mk2(float x, float y) { f2 r; r.x = x; r.y = y; return r; }

/* rule 3 on (a, a + ab, a + ac) as xo_triangle, also returning t, V, W and det of a counted triangle */
static int xl_triangle(f3 o, f3 d, f3 a, f3 ab, f3 ac, float tmax, float *tout, float *vout, float *wout, float *detout)
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
    *tout = t; *vout = V; *wout = W; *detout = det;
    return det < 0.0f ? 1 : -1;
}

static int xl_cmp(const void *pa, const void *pb)
{
    const xl_hit *a = (const xl_hit *)pa, *b = (const xl_hit *)pb;
    if (a->t != b->t) return a->t < b->t ? -1 : 1;
    if (a->inst != b->inst) return a->inst < b->inst ? -1 : 1;
    return a->tri < b->tri ? -1 : (a->tri > b->tri ? 1 : 0);
}

/* every counted pair of one ray, sorted; returns the count (*out malloc'd, the caller frees) */
static int xl_ray(const OrcScene *sc, f3 w, f3 dw, float tmax, xl_hit **out)
{
    int i, k, n = 0, cap = 16;
    xl_hit *h = (xl_hit *)malloc(sizeof(xl_hit) * cap);
    for (i = 0; i < sc->ninst; i++) {
        const instance_t *in = &sc->instances[i];
        const OrcMesh *m = sc->meshes[in->mesh_index];
        f3 o = apply_lre(in->pose, w);
        f3 d = apply_euler(mk3(in->pose.yaw, in->pose.pitch, in->pose.roll), dw);
        for (k = 0; k < m->ntris; k++) {
            const tri_t *tr = &m->tris[k];
            f3 a, ab, ac;
            float t = 0.0f, V = 0.0f, W = 0.0f, det = 1.0f, b1, b2, u0;
            int sg;
            xo_tri(tr, in->scale, &a, &ab, &ac);
            sg = xl_triangle(o, d, a, ab, ac, tmax, &t, &V, &W, &det);
            if (!sg) continue;
            if (n == cap) { cap *= 2; h = (xl_hit *)realloc(h, sizeof(xl_hit) * cap); }
            b1 = V / det; b2 = W / det;
            u0 = (1.0f - b2) - b1;
            h[n].t = t; h[n].b1 = b1; h[n].b2 = b2; h[n].inst = i; h[n].tri = k; h[n].sign = sg;
            h[n].uv = xl_mk2((u0 * tr->uv[0].x + b1 * tr->uv[1].x) + b2 * tr->uv[2].x, (u0 * tr->uv[0].y + b1 * tr->uv[1].y) + b2 * tr->uv[2].y);
            n++;
        }
    }
    qsort(h, (size_t)n, sizeof(xl_hit), xl_cmp);
    *out = h;
    return n;
}

/* n rays org / dir [n][3], tmax [n] (NULL = +inf); rooms: offsets [n + 1] (CSR) or, with offsets NULL, max_hits per ray.  Writes the
 * first min(count, room) pairs into each room and pads the rest; nothing outside the rooms.  count [n] = the full count. */
void orcl_list_crossings(const OrcScene *sc, int64_t n, const float *org, const float *dir, const float *tmax, const int64_t *offsets,
                         int32_t max_hits, float *t, int32_t *inst, int32_t *tri, int8_t *sign, float *bary, float *uv, float *point,
                         int32_t *count)
{
    int64_t j, s;
    for (j = 0; j < n; j++) {
        f3 w = mk3(org[3 * j], org[3 * j + 1], org[3 * j + 2]), d = mk3(dir[3 * j], dir[3 * j + 1], dir[3 * j + 2]);
        xl_hit *h;
        int c = xl_ray(sc, w, d, tmax ? tmax[j] : INFINITY, &h);
        int64_t start = offsets ? offsets[j] : j * (int64_t)max_hits;
        int64_t room = offsets ? (offsets[j + 1] > offsets[j] ? offsets[j + 1] - offsets[j] : 0) : max_hits;
        count[j] = c;
        for (s = 0; s < room; s++) {
            int64_t q = start + s;
            if (s < c) {
                t[q] = h[s].t; inst[q] = h[s].inst; tri[q] = h[s].tri; sign[q] = (int8_t)h[s].sign;
                bary[2 * q] = h[s].b1; bary[2 * q + 1] = h[s].b2;
                uv[2 * q] = h[s].uv.x; uv[2 * q + 1] = h[s].uv.y;
                point[3 * q] = w.x + h[s].t * d.x; point[3 * q + 1] = w.y + h[s].t * d.y; point[3 * q + 2] = w.z + h[s].t * d.z;
            } else {
                t[q] = INFINITY; inst[q] = -1; tri[q] = -1; sign[q] = 0;
                bary[2 * q] = bary[2 * q + 1] = 0.0f; uv[2 * q] = uv[2 * q + 1] = 0.0f;
                point[3 * q] = point[3 * q + 1] = point[3 * q + 2] = 0.0f;
            }
        }
        free(h);
    }
}

/* rule 3 on one triangle in scaled mesh space (host tests): sign (0 = not counted) and out4 = t, V, W, det */
int orcl_on_triangle(const float *o, const float *d, const float *a, const float *ab, const float *ac, float tmax, float *out4)
{
    return xl_triangle(mk3(o[0], o[1], o[2]), mk3(d[0], d[1], d[2]), mk3(a[0], a[1], a[2]), mk3(ab[0], ab[1], ab[2]),
                       mk3(ac[0], ac[1], ac[2]), tmax, &out4[0], &out4[1], &out4[2], &out4[3]);
}
