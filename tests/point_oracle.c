/* point_oracle.c -- TEST INFRASTRUCTURE: the brute-force closest point of a scene to arbitrary points, the specification of
 * rt_closest_points (include/rt_hip.h).  It includes oracle/rt_oracle.c unchanged for its scene (OrcScene)
 * and apply_lre, and restates the fp32 sequence of the rule on its own -- no header is shared with the kernel, so an error in
 * either copy shows as a difference.  Every (instance, triangle) is visited; there is no tree.  Built by tests/point_oracle.py
 * with the oracle's own flags (oracle/Makefile: -ffp-contract=off). */
#include "../oracle/rt_oracle.c"

static float pt_dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static f3 pt_sub(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static float pt_len2(f3 d) { return (d.x * d.x + d.y * d.y) + d.z * d.z; }
static f3 pt_at(f3 a, f3 ab, f3 ac, float b1, float b2)
{
    return mk3((a.x + b1 * ab.x) + b2 * ac.x, (a.y + b1 * ab.y) + b2 * ac.y, (a.z + b1 * ab.z) + b2 * ac.z);
}
/* an edge ratio: 0 unless the denominator is > 0, never above 1 */
static float pt_ratio(float a, float b)
{
    float r;
    if (!(b > 0.0f)) return 0.0f;
    r = a / b;
    return r < 1.0f ? r : 1.0f;                     /* (a NaN ratio -- inf / inf -- gives 1, as fminf does) */
}
/* clamped projection onto p0 + t * d, 0 for a zero-length d or a NaN t */
static float pt_seg(f3 q, f3 p0, f3 d)
{
    float dd = pt_dot(d, d), t = 0.0f;
    if (dd > 0.0f) t = pt_dot(pt_sub(q, p0), d) / dd;
    if (!(t > 0.0f)) return 0.0f;
    return t < 1.0f ? t : 1.0f;
}

/* Ericson, Real-Time Collision Detection 5.1.5, over A, AB, AC -> (b1, b2); the fallback where the face region is inconsistent */
static void pt_weights(f3 q, f3 a, f3 ab, f3 ac, float *b1, float *b2)
{
    f3 ap = pt_sub(q, a), bp, cp;
    float d1 = pt_dot(ab, ap), d2 = pt_dot(ac, ap), d3, d4, d5, d6, va, vb, vc, sum, e43, e56;
    if (d1 <= 0.0f && d2 <= 0.0f) { *b1 = 0.0f; *b2 = 0.0f; return; }
    bp = pt_sub(ap, ab);
    d3 = pt_dot(ab, bp); d4 = pt_dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) { *b1 = 1.0f; *b2 = 0.0f; return; }
    vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { *b1 = pt_ratio(d1, d1 - d3); *b2 = 0.0f; return; }
    cp = pt_sub(ap, ac);
    d5 = pt_dot(ab, cp); d6 = pt_dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) { *b1 = 0.0f; *b2 = 1.0f; return; }
    vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { *b1 = 0.0f; *b2 = pt_ratio(d2, d2 - d6); return; }
    va = d3 * d6 - d5 * d4;
    e43 = d4 - d3; e56 = d5 - d6;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {
        float w = pt_ratio(e43, e43 + e56);
        *b1 = 1.0f - w; *b2 = w; return;
    }
    sum = (va + vb) + vc;
    if (va >= 0.0f && vb >= 0.0f && vc >= 0.0f && sum > 0.0f) { *b1 = vb / sum; *b2 = vc / sum; return; }
    {
        float t0 = pt_seg(q, a, ab), t1 = pt_seg(q, a, ac), t2 = pt_seg(q, mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z), pt_sub(ac, ab));
        float s = 1.0f - t2;
        float e0 = pt_len2(pt_sub(q, pt_at(a, ab, ac, t0, 0.0f)));
        float e1 = pt_len2(pt_sub(q, pt_at(a, ab, ac, 0.0f, t1)));
        float e2 = pt_len2(pt_sub(q, pt_at(a, ab, ac, s, t2)));
        *b1 = t0; *b2 = 0.0f;
        if (e1 < e0) { e0 = e1; *b1 = 0.0f; *b2 = t1; }
        if (e2 < e0) { *b1 = s; *b2 = t2; }
    }
}

/* triangle t of instance `in` in scaled mesh space: the stored v0, e1 = v1 - v0, e0 = v2 - v0 (fp32), times the scale */
static void pt_tri(const tri_t *t, f3 s, f3 *a, f3 *ab, f3 *ac)
{
    f3 e1 = pt_sub(t->v[1], t->v[0]), e0 = pt_sub(t->v[2], t->v[0]);
    *a = mk3(t->v[0].x * s.x, t->v[0].y * s.y, t->v[0].z * s.z);
    *ab = mk3(e1.x * s.x, e1.y * s.y, e1.z * s.z);
    *ac = mk3(e0.x * s.x, e0.y * s.y, e0.z * s.z);
}

/* n points pts [n][3]; maxd [n] (NULL = +inf).  Outputs, each optional: dist [n] (FLT_MAX on a miss), inst / tri [n] (-1),
 * point / normal [n][3], bary / uv [n][2] (0 on a miss).  only_inst >= 0: that instance alone (the host tests' per-instance view). */
void orcx_closest_points(const OrcScene *sc, int64_t n, const float *pts, const float *maxd, int only_inst, float *dist, int32_t *inst,
                         int32_t *tri, float *point, float *normal, float *bary, float *uv)
{
    int64_t j;
    for (j = 0; j < n; j++) {
        f3 p = mk3(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]);
        float bound = maxd ? maxd[j] : INFINITY, best = 0.0f, wb1 = 0.0f, wb2 = 0.0f;
        int bi = -1, bt = -1, i, k;
        for (i = 0; i < sc->ninst; i++) {
            const instance_t *in = &sc->instances[i];
            const OrcMesh *m = sc->meshes[in->mesh_index];
            f3 q = apply_lre(in->pose, p);
            if (only_inst >= 0 && i != only_inst) continue;
            for (k = 0; k < m->ntris; k++) {
                f3 a, ab, ac;
                float b1, b2, d2;
                pt_tri(&m->tris[k], in->scale, &a, &ab, &ac);
                pt_weights(q, a, ab, ac, &b1, &b2);
                d2 = pt_len2(pt_sub(q, pt_at(a, ab, ac, b1, b2)));
                if (isnan(d2) || !(sqrtf(d2) <= bound)) continue;
                if (bi < 0 || d2 < best || (d2 == best && (i < bi || (i == bi && k < bt)))) { best = d2; bi = i; bt = k; wb1 = b1; wb2 = b2; }
            }
        }
        if (dist) dist[j] = bi >= 0 ? sqrtf(best) : FLT_MAX;
        if (inst) inst[j] = bi;
        if (tri) tri[j] = bt;
        if (bary) { bary[2 * j] = bi >= 0 ? wb1 : 0.0f; bary[2 * j + 1] = bi >= 0 ? wb2 : 0.0f; }
        if (bi < 0) {
            if (point) point[3 * j] = point[3 * j + 1] = point[3 * j + 2] = 0.0f;
            if (normal) normal[3 * j] = normal[3 * j + 1] = normal[3 * j + 2] = 0.0f;
            if (uv) uv[2 * j] = uv[2 * j + 1] = 0.0f;
            continue;
        }
        {
            const instance_t *in = &sc->instances[bi];
            const tri_t *t = &sc->meshes[in->mesh_index]->tris[bt];
            f3 a, ab, ac, c, w, nn;
            float u0 = (1.0f - wb2) - wb1;
            pt_tri(t, in->scale, &a, &ab, &ac);
            c = pt_at(a, ab, ac, wb1, wb2);
            w = apply_lre(in->inv_pose, c);                                   /* raycast.cu:98-102's map */
            if (point) { point[3 * j] = w.x; point[3 * j + 1] = w.y; point[3 * j + 2] = w.z; }
            nn = apply_euler(in->inv_rotation, t->normal);                    /* raycast.cu:115-122 */
            nn.x *= in->scale.x; nn.y *= in->scale.y; nn.z *= in->scale.z;
            nn = normalize3(nn);
            if (normal) { normal[3 * j] = nn.x; normal[3 * j + 1] = nn.y; normal[3 * j + 2] = nn.z; }
            if (uv) {
                uv[2 * j] = (u0 * t->uv[0].x + wb1 * t->uv[1].x) + wb2 * t->uv[2].x;
                uv[2 * j + 1] = (u0 * t->uv[0].y + wb1 * t->uv[1].y) + wb2 * t->uv[2].y;
            }
        }
    }
}

/* the rule on one triangle given in scaled mesh space (host tests): a / ab / ac / q [3] -> b1, b2, d2 */
void orcx_closest_on_triangle(const float *q, const float *a, const float *ab, const float *ac, float *out3)
{
    float b1, b2;
    f3 Q = mk3(q[0], q[1], q[2]), A = mk3(a[0], a[1], a[2]), AB = mk3(ab[0], ab[1], ab[2]), AC = mk3(ac[0], ac[1], ac[2]);
    pt_weights(Q, A, AB, AC, &b1, &b2);
    out3[0] = b1; out3[1] = b2; out3[2] = pt_len2(pt_sub(Q, pt_at(A, AB, AC, b1, b2)));
}
