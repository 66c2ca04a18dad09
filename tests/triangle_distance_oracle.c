/* triangle_distance_oracle.c -- TEST INFRASTRUCTURE: the brute-force nearest point of a scene to arbitrary triangles with the
 * intersection count, the specification of rt_closest_to_triangles (include/rt_hip.h rule 14).  It includes
 * tests/tri_intersect_oracle.c unchanged for step 5 (and through it tests/crossing_oracle.c and oracle/rt_oracle.c) for its scene
 * (OrcScene), apply_lre and rule 10's pairs, and restates the fp32 sequence of the rule on its own -- the weights, the
 * segment-segment routine and the fifteen candidates; no header is shared with the kernel, so an error in either copy shows as a
 * difference.  Every (instance, triangle) is visited; there is no tree.  Built by tests/triangle_distance_oracle.py with the
 * oracle's own flags (oracle/Makefile: -ffp-contract=off). */
#include "tri_intersect_oracle.c"

static float td_dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static f3 td_sub(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static f3 td_add(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
static float td_len2(f3 d) { return (d.x * d.x + d.y * d.y) + d.z * d.z; }
static f3 td_at(f3 a, f3 ab, f3 ac, float b1, float b2)
{
    return mk3((a.x + b1 * ab.x) + b2 * ac.x, (a.y + b1 * ab.y) + b2 * ac.y, (a.z + b1 * ab.z) + b2 * ac.z);
}
static float td_ratio(float a, float b)
{
    float r;
    if (!(b > 0.0f)) return 0.0f;
    r = a / b;
    return r < 1.0f ? r : 1.0f;
}
static float td_clamp01(float x)
{
    if (!(x > 0.0f)) return 0.0f;
    return x < 1.0f ? x : 1.0f;
}
/* clamped projection of the point q onto p0 + t * d (rule 2's fallback) */
static float td_proj(f3 q, f3 p0, f3 d)
{
    float dd = td_dot(d, d), t = 0.0f;
    if (dd > 0.0f) t = td_dot(td_sub(q, p0), d) / dd;
    return td_clamp01(t);
}

/* rule 2: Ericson 5.1.5 over A, AB, AC for the point q -> (b1, b2), with the nearest-edge fallback */
static void td_weights(f3 q, f3 a, f3 ab, f3 ac, float *b1, float *b2)
{
    f3 ap = td_sub(q, a), bp, cp;
    float d1 = td_dot(ab, ap), d2 = td_dot(ac, ap), d3, d4, d5, d6, va, vb, vc, sum, e43, e56;
    if (d1 <= 0.0f && d2 <= 0.0f) { *b1 = 0.0f; *b2 = 0.0f; return; }
    bp = td_sub(ap, ab);
    d3 = td_dot(ab, bp); d4 = td_dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) { *b1 = 1.0f; *b2 = 0.0f; return; }
    vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { *b1 = td_ratio(d1, d1 - d3); *b2 = 0.0f; return; }
    cp = td_sub(ap, ac);
    d5 = td_dot(ab, cp); d6 = td_dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) { *b1 = 0.0f; *b2 = 1.0f; return; }
    vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { *b1 = 0.0f; *b2 = td_ratio(d2, d2 - d6); return; }
    va = d3 * d6 - d5 * d4;
    e43 = d4 - d3; e56 = d5 - d6;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {
        float w = td_ratio(e43, e43 + e56);
        *b1 = 1.0f - w; *b2 = w; return;
    }
    sum = (va + vb) + vc;
    if (va >= 0.0f && vb >= 0.0f && vc >= 0.0f && sum > 0.0f) { *b1 = vb / sum; *b2 = vc / sum; return; }
    {
        float t0 = td_proj(q, a, ab), t1 = td_proj(q, a, ac), t2 = td_proj(q, td_add(a, ab), td_sub(ac, ab));
        float s = 1.0f - t2;
        float e0 = td_len2(td_sub(q, td_at(a, ab, ac, t0, 0.0f)));
        float e1 = td_len2(td_sub(q, td_at(a, ab, ac, 0.0f, t1)));
        float e2 = td_len2(td_sub(q, td_at(a, ab, ac, s, t2)));
        *b1 = t0; *b2 = 0.0f;
        if (e1 < e0) { e0 = e1; *b1 = 0.0f; *b2 = t1; }
        if (e2 < e0) { *b1 = s; *b2 = t2; }
    }
}

/* rule 13 step 4: the closest pair (s, u) of q0 + s * d and e0 + u * f */
static void td_segseg(f3 q0, f3 d, f3 e0, f3 f, float *s, float *u)
{
    f3 r = td_sub(q0, e0);
    float a = td_dot(d, d), e = td_dot(f, f), ff = td_dot(f, r), b, c, den;
    if (!(a > 0.0f) && !(e > 0.0f)) { *s = 0.0f; *u = 0.0f; return; }
    if (!(a > 0.0f)) { *s = 0.0f; *u = td_clamp01(ff / e); return; }
    c = td_dot(d, r);
    if (!(e > 0.0f)) { *u = 0.0f; *s = td_clamp01(-c / a); return; }
    b = td_dot(d, f);
    den = a * e - b * b;
    *s = 0.0f;
    if (den > 0.0f) *s = td_clamp01((b * ff - c * e) / den);
    *u = (b * *s + ff) / e;
    if (!(*u >= 0.0f)) { *u = 0.0f; *s = td_clamp01(-c / a); }
    else if (*u > 1.0f) { *u = 1.0f; *s = td_clamp01((b - c) / a); }
}

typedef struct { float q1, q2, b1, b2, d2; int which; } td_cand;
typedef struct { f3 o, e1, e2; } td_tri;         /* a triangle as (vertex, edge, edge): (Q0, QAB, QAC) or (A, AB, AC) */

/* step 3's common tail: X, c, d2 of one candidate, kept when it beats the pair's best so far (the first of equals stays; a NaN loses
 * to anything that is not NaN) */
static void td_try(td_cand *best, int which, const td_tri *q, const td_tri *t, float q1, float q2, float b1, float b2)
{
    f3 x = td_at(q->o, q->e1, q->e2, q1, q2);
    float d2 = td_len2(td_sub(x, td_at(t->o, t->e1, t->e2, b1, b2)));
    int wins = best->which < 0 || (isnan(best->d2) ? !isnan(d2) : d2 < best->d2);
    if (wins) { best->q1 = q1; best->q2 = q2; best->b1 = b1; best->b2 = b2; best->d2 = d2; best->which = which; }
}

static f3 td_corner(const td_tri *t, int k) { return k == 0 ? t->o : td_add(t->o, k == 1 ? t->e1 : t->e2); }
static void td_edge(const td_tri *t, int k, f3 *from, f3 *dir)
{
    *from = k == 2 ? td_add(t->o, t->e1) : t->o;
    *dir = k == 0 ? t->e1 : k == 1 ? t->e2 : td_sub(t->e2, t->e1);
}
static void td_on_edge(int k, float s, float *w1, float *w2)
{
    *w1 = k == 0 ? s : k == 1 ? 0.0f : 1.0f - s;
    *w2 = k == 0 ? 0.0f : s;
}

/* steps 1-3 on one pair in scaled mesh space: the query's mapped vertices, the scene triangle (A, AB, AC) */
static td_cand td_pair(f3 v0, f3 v1, f3 v2, f3 a, f3 ab, f3 ac)
{
    td_cand best = {0.0f, 0.0f, 0.0f, 0.0f, NAN, -1};
    td_tri q, t;
    int k, m;
    q.o = v0; q.e1 = td_sub(v1, v0); q.e2 = td_sub(v2, v0);
    t.o = a; t.e1 = ab; t.e2 = ac;
    for (k = 0; k < 3; k++) {
        float b1, b2;
        td_weights(td_corner(&q, k), a, ab, ac, &b1, &b2);
        td_try(&best, k, &q, &t, k == 1 ? 1.0f : 0.0f, k == 2 ? 1.0f : 0.0f, b1, b2);
    }
    if (td_dot(q.e1, q.e1) > 0.0f || td_dot(q.e2, q.e2) > 0.0f)
        for (k = 0; k < 3; k++) {
            float q1, q2;
            td_weights(td_corner(&t, k), q.o, q.e1, q.e2, &q1, &q2);
            td_try(&best, 3 + k, &q, &t, q1, q2, k == 1 ? 1.0f : 0.0f, k == 2 ? 1.0f : 0.0f);
        }
    for (m = 0; m < 3; m++) {
        f3 g0, d;
        td_edge(&q, m, &g0, &d);
        if (!(td_dot(d, d) > 0.0f)) continue;
        for (k = 0; k < 3; k++) {
            f3 e0, f;
            float s, u, q1, q2, b1, b2;
            td_edge(&t, k, &e0, &f);
            td_segseg(g0, d, e0, f, &s, &u);
            td_on_edge(m, s, &q1, &q2);
            td_on_edge(k, u, &b1, &b2);
            td_try(&best, 6 + 3 * m + k, &q, &t, q1, q2, b1, b2);
        }
    }
    return best;
}

/* n query triangles tris [n][3][3] (world); maxd [n] (NULL = +inf); skip [n] (NULL = none).  Outputs, each optional: dist [n] (FLT_MAX
 * on a miss), inst / tri [n] (-1), qbary [n][2], qpoint / point / normal [n][3], bary / uv [n][2] (0 on a miss), meets [n] (rule 10's
 * count), clearance [n], within [n], which [n] (the winning candidate 0..14, -1 on a miss: the tests' coverage counts). */
void orcd_closest_to_triangles(const OrcScene *sc, int64_t n, const float *tris, const float *maxd, const int32_t *skip, float *dist,
                               int32_t *inst, int32_t *tri, float *qbary, float *qpoint, float *point, float *normal, float *bary,
                               float *uv, int32_t *meets, float *clearance, int32_t *within, int32_t *which)
{
    int64_t j;
    for (j = 0; j < n; j++) {
        const float *P = tris + 9 * j;
        f3 p[3];
        float bound = maxd ? maxd[j] : INFINITY, d;
        td_cand best = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, -1};
        int bi = -1, bt = -1, i, k, meet, sk = skip ? skip[j] : -1;
        for (k = 0; k < 3; k++) p[k] = mk3(P[3 * k], P[3 * k + 1], P[3 * k + 2]);
        for (i = 0; i < sc->ninst; i++) {
            const instance_t *in = &sc->instances[i];
            const OrcMesh *m = sc->meshes[in->mesh_index];
            f3 q0, q1, q2;
            if (i == sk) continue;
            q0 = apply_lre(in->pose, p[0]); q1 = apply_lre(in->pose, p[1]); q2 = apply_lre(in->pose, p[2]);
            for (k = 0; k < m->ntris; k++) {
                f3 a, ab, ac;
                td_cand c;
                xo_tri(&m->tris[k], in->scale, &a, &ab, &ac);
                c = td_pair(q0, q1, q2, a, ab, ac);
                if (isnan(c.d2) || !(sqrtf(c.d2) <= bound)) continue;
                if (bi < 0 || c.d2 < best.d2 || (c.d2 == best.d2 && (i < bi || (i == bi && k < bt)))) { best = c; bi = i; bt = k; }
            }
        }
        meet = ti_query(sc, P, sk, NULL, NULL);
        d = bi >= 0 ? sqrtf(best.d2) : FLT_MAX;
        if (dist) dist[j] = d;
        if (inst) inst[j] = bi;
        if (tri) tri[j] = bt;
        if (qbary) { qbary[2 * j] = bi >= 0 ? best.q1 : 0.0f; qbary[2 * j + 1] = bi >= 0 ? best.q2 : 0.0f; }
        if (bary) { bary[2 * j] = bi >= 0 ? best.b1 : 0.0f; bary[2 * j + 1] = bi >= 0 ? best.b2 : 0.0f; }
        if (meets) meets[j] = meet;
        if (clearance) clearance[j] = meet > 0 ? 0.0f : d;
        if (within) within[j] = (bi >= 0 || meet > 0) ? 1 : 0;
        if (which) which[j] = bi >= 0 ? best.which : -1;
        if (bi < 0) {
            if (qpoint) qpoint[3 * j] = qpoint[3 * j + 1] = qpoint[3 * j + 2] = 0.0f;
            if (point) point[3 * j] = point[3 * j + 1] = point[3 * j + 2] = 0.0f;
            if (normal) normal[3 * j] = normal[3 * j + 1] = normal[3 * j + 2] = 0.0f;
            if (uv) uv[2 * j] = uv[2 * j + 1] = 0.0f;
            continue;
        }
        {
            const instance_t *in = &sc->instances[bi];
            const tri_t *t = &sc->meshes[in->mesh_index]->tris[bt];
            f3 q0 = apply_lre(in->pose, p[0]), q1 = apply_lre(in->pose, p[1]), q2 = apply_lre(in->pose, p[2]), a, ab, ac, x, c, w, nn;
            float u0 = (1.0f - best.b2) - best.b1;
            xo_tri(t, in->scale, &a, &ab, &ac);
            x = td_at(q0, td_sub(q1, q0), td_sub(q2, q0), best.q1, best.q2);
            c = td_at(a, ab, ac, best.b1, best.b2);
            w = apply_lre(in->inv_pose, x);
            if (qpoint) { qpoint[3 * j] = w.x; qpoint[3 * j + 1] = w.y; qpoint[3 * j + 2] = w.z; }
            w = apply_lre(in->inv_pose, c);
            if (point) { point[3 * j] = w.x; point[3 * j + 1] = w.y; point[3 * j + 2] = w.z; }
            nn = apply_euler(in->inv_rotation, t->normal);
            nn.x *= in->scale.x; nn.y *= in->scale.y; nn.z *= in->scale.z;
            nn = normalize3(nn);
            if (normal) { normal[3 * j] = nn.x; normal[3 * j + 1] = nn.y; normal[3 * j + 2] = nn.z; }
            if (uv) {
                uv[2 * j] = (u0 * t->uv[0].x + best.b1 * t->uv[1].x) + best.b2 * t->uv[2].x;
                uv[2 * j + 1] = (u0 * t->uv[0].y + best.b1 * t->uv[1].y) + best.b2 * t->uv[2].y;
            }
        }
    }
}

/* the rule on one pair given in scaled mesh space (host tests): q9 [3][3] the query's mapped vertices, a / ab / ac [3] ->
 * out6 = q1, q2, b1, b2, d2, which */
void orcd_on_triangle(const float *q9, const float *a, const float *ab, const float *ac, float *out6)
{
    td_cand c = td_pair(mk3(q9[0], q9[1], q9[2]), mk3(q9[3], q9[4], q9[5]), mk3(q9[6], q9[7], q9[8]), mk3(a[0], a[1], a[2]),
                        mk3(ab[0], ab[1], ab[2]), mk3(ac[0], ac[1], ac[2]));
    out6[0] = c.q1; out6[1] = c.q2; out6[2] = c.b1; out6[3] = c.b2; out6[4] = c.d2; out6[5] = (float)c.which;
}
