/* segment_oracle.c -- TEST INFRASTRUCTURE: the brute-force nearest point of a scene to arbitrary segments with the capsule test, the
 * specification of rt_closest_to_segments (include/rt_hip.h rule 13).  It includes tests/crossing_oracle.c
 * (and through it oracle/rt_oracle.c, unchanged) for its scene (OrcScene), apply_lre and step 6's crossing count, and restates the
 * fp32 sequence of the rule on its own -- no header is shared with the kernel, so an error in either copy shows as a difference.
 * Every (instance, triangle) is visited; there is no tree.  Built by tests/segment_oracle.py with the oracle's own flags
 * (oracle/Makefile: -ffp-contract=off). */
#include "crossing_oracle.c"

static float sg_dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static f3 sg_sub(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static f3 sg_add(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
static float sg_len2(f3 d) { return (d.x * d.x + d.y * d.y) + d.z * d.z; }
static f3 sg_at(f3 a, f3 ab, f3 ac, float b1, float b2)
{
    return mk3((a.x + b1 * ab.x) + b2 * ac.x, (a.y + b1 * ab.y) + b2 * ac.y, (a.z + b1 * ab.z) + b2 * ac.z);
}
static float sg_ratio(float a, float b)
{
    float r;
    if (!(b > 0.0f)) return 0.0f;
    r = a / b;
    return r < 1.0f ? r : 1.0f;
}
static float sg_clamp01(float x)
{
    if (!(x > 0.0f)) return 0.0f;
    return x < 1.0f ? x : 1.0f;
}
/* clamped projection of the point q onto p0 + t * d (rule 2's fallback) */
static float sg_proj(f3 q, f3 p0, f3 d)
{
    float dd = sg_dot(d, d), t = 0.0f;
    if (dd > 0.0f) t = sg_dot(sg_sub(q, p0), d) / dd;
    return sg_clamp01(t);
}

/* rule 2: Ericson 5.1.5 over A, AB, AC for the point q -> (b1, b2), with the nearest-edge fallback */
static void sg_weights(f3 q, f3 a, f3 ab, f3 ac, float *b1, float *b2)
{
    f3 ap = sg_sub(q, a), bp, cp;
    float d1 = sg_dot(ab, ap), d2 = sg_dot(ac, ap), d3, d4, d5, d6, va, vb, vc, sum, e43, e56;
    if (d1 <= 0.0f && d2 <= 0.0f) { *b1 = 0.0f; *b2 = 0.0f; return; }
    bp = sg_sub(ap, ab);
    d3 = sg_dot(ab, bp); d4 = sg_dot(ac, bp);
    if (d3 >= 0.0f && d4 <= d3) { *b1 = 1.0f; *b2 = 0.0f; return; }
    vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { *b1 = sg_ratio(d1, d1 - d3); *b2 = 0.0f; return; }
    cp = sg_sub(ap, ac);
    d5 = sg_dot(ab, cp); d6 = sg_dot(ac, cp);
    if (d6 >= 0.0f && d5 <= d6) { *b1 = 0.0f; *b2 = 1.0f; return; }
    vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { *b1 = 0.0f; *b2 = sg_ratio(d2, d2 - d6); return; }
    va = d3 * d6 - d5 * d4;
    e43 = d4 - d3; e56 = d5 - d6;
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) {
        float w = sg_ratio(e43, e43 + e56);
        *b1 = 1.0f - w; *b2 = w; return;
    }
    sum = (va + vb) + vc;
    if (va >= 0.0f && vb >= 0.0f && vc >= 0.0f && sum > 0.0f) { *b1 = vb / sum; *b2 = vc / sum; return; }
    {
        float t0 = sg_proj(q, a, ab), t1 = sg_proj(q, a, ac), t2 = sg_proj(q, sg_add(a, ab), sg_sub(ac, ab));
        float s = 1.0f - t2;
        float e0 = sg_len2(sg_sub(q, sg_at(a, ab, ac, t0, 0.0f)));
        float e1 = sg_len2(sg_sub(q, sg_at(a, ab, ac, 0.0f, t1)));
        float e2 = sg_len2(sg_sub(q, sg_at(a, ab, ac, s, t2)));
        *b1 = t0; *b2 = 0.0f;
        if (e1 < e0) { e0 = e1; *b1 = 0.0f; *b2 = t1; }
        if (e2 < e0) { *b1 = s; *b2 = t2; }
    }
}

/* step 4: the closest pair (s, u) of q0 + s * d and e0 + u * f */
static void sg_segseg(f3 q0, f3 d, f3 e0, f3 f, float *s, float *u)
{
    f3 r = sg_sub(q0, e0);
    float a = sg_dot(d, d), e = sg_dot(f, f), ff = sg_dot(f, r), b, c, den;
    if (!(a > 0.0f) && !(e > 0.0f)) { *s = 0.0f; *u = 0.0f; return; }
    if (!(a > 0.0f)) { *s = 0.0f; *u = sg_clamp01(ff / e); return; }
    c = sg_dot(d, r);
    if (!(e > 0.0f)) { *u = 0.0f; *s = sg_clamp01(-c / a); return; }
    b = sg_dot(d, f);
    den = a * e - b * b;
    *s = 0.0f;
    if (den > 0.0f) *s = sg_clamp01((b * ff - c * e) / den);
    *u = (b * *s + ff) / e;
    if (!(*u >= 0.0f)) { *u = 0.0f; *s = sg_clamp01(-c / a); }
    else if (*u > 1.0f) { *u = 1.0f; *s = sg_clamp01((b - c) / a); }
}

typedef struct { float s, b1, b2, d2; int which; } sg_cand;

/* step 3's common tail: X, c, d2 of one candidate, kept when it beats the triangle's best so far (the first of equals stays; a NaN
 * loses to anything that is not NaN) */
static void sg_try(sg_cand *best, int which, f3 q0, f3 d, f3 a, f3 ab, f3 ac, float s, float b1, float b2)
{
    f3 x = mk3(q0.x + s * d.x, q0.y + s * d.y, q0.z + s * d.z);
    float d2 = sg_len2(sg_sub(x, sg_at(a, ab, ac, b1, b2)));
    int wins = best->which < 0 || (isnan(best->d2) ? !isnan(d2) : d2 < best->d2);
    if (wins) { best->s = s; best->b1 = b1; best->b2 = b2; best->d2 = d2; best->which = which; }
}

/* steps 2-3 on one triangle in scaled mesh space */
static sg_cand sg_triangle(f3 q0, f3 q1, f3 a, f3 ab, f3 ac)
{
    sg_cand best = {0.0f, 0.0f, 0.0f, NAN, -1};
    f3 d = sg_sub(q1, q0);
    float b1, b2, s, u;
    sg_weights(q0, a, ab, ac, &b1, &b2);
    sg_try(&best, 0, q0, d, a, ab, ac, 0.0f, b1, b2);
    sg_weights(q1, a, ab, ac, &b1, &b2);
    sg_try(&best, 1, q0, d, a, ab, ac, 1.0f, b1, b2);
    if (!(sg_dot(d, d) > 0.0f)) return best;        /* a zero-length segment: the ends alone, so (a) is the point query's answer */
    sg_segseg(q0, d, a, ab, &s, &u);
    sg_try(&best, 2, q0, d, a, ab, ac, s, u, 0.0f);
    sg_segseg(q0, d, a, ac, &s, &u);
    sg_try(&best, 3, q0, d, a, ab, ac, s, 0.0f, u);
    sg_segseg(q0, d, sg_add(a, ab), sg_sub(ac, ab), &s, &u);
    sg_try(&best, 4, q0, d, a, ab, ac, s, 1.0f - u, u);
    return best;
}

/* n segments segs [n][2][3]; maxd [n] (NULL = +inf).  Outputs, each optional: dist [n] (FLT_MAX on a miss), inst / tri [n] (-1), param
 * [n], segpt / point / normal [n][3], bary / uv [n][2] (0 on a miss), crossings [n], clearance [n], within [n], which [n] (the winning
 * candidate 0..4 = a..e, -1 on a miss: the tests' coverage counts).  only_inst >= 0: that instance alone, in the distance half. */
void orcx_closest_to_segments(const OrcScene *sc, int64_t n, const float *segs, const float *maxd, int only_inst, float *dist,
                              int32_t *inst, int32_t *tri, float *param, float *segpt, float *point, float *normal, float *bary, float *uv,
                              int32_t *crossings, float *clearance, int32_t *within, int32_t *which)
{
    int64_t j;
    for (j = 0; j < n; j++) {
        f3 p0 = mk3(segs[6 * j], segs[6 * j + 1], segs[6 * j + 2]), p1 = mk3(segs[6 * j + 3], segs[6 * j + 4], segs[6 * j + 5]);
        float bound = maxd ? maxd[j] : INFINITY, d;
        sg_cand best = {0.0f, 0.0f, 0.0f, 0.0f, -1};
        int bi = -1, bt = -1, i, k, cross;
        int32_t wn;
        for (i = 0; i < sc->ninst; i++) {
            const instance_t *in = &sc->instances[i];
            const OrcMesh *m = sc->meshes[in->mesh_index];
            f3 q0 = apply_lre(in->pose, p0), q1 = apply_lre(in->pose, p1);
            if (only_inst >= 0 && i != only_inst) continue;
            for (k = 0; k < m->ntris; k++) {
                f3 a, ab, ac;
                sg_cand c;
                xo_tri(&m->tris[k], in->scale, &a, &ab, &ac);
                c = sg_triangle(q0, q1, a, ab, ac);
                if (isnan(c.d2) || !(sqrtf(c.d2) <= bound)) continue;
                if (bi < 0 || c.d2 < best.d2 || (c.d2 == best.d2 && (i < bi || (i == bi && k < bt)))) { best = c; bi = i; bt = k; }
            }
        }
        cross = xo_ray(sc, p0, mk3(p1.x - p0.x, p1.y - p0.y, p1.z - p0.z), 1.0f, &wn, NULL, 0);
        d = bi >= 0 ? sqrtf(best.d2) : FLT_MAX;
        if (dist) dist[j] = d;
        if (inst) inst[j] = bi;
        if (tri) tri[j] = bt;
        if (param) param[j] = bi >= 0 ? best.s : 0.0f;
        if (bary) { bary[2 * j] = bi >= 0 ? best.b1 : 0.0f; bary[2 * j + 1] = bi >= 0 ? best.b2 : 0.0f; }
        if (crossings) crossings[j] = cross;
        if (clearance) clearance[j] = cross > 0 ? 0.0f : d;
        if (within) within[j] = (bi >= 0 || cross > 0) ? 1 : 0;
        if (which) which[j] = bi >= 0 ? best.which : -1;
        if (bi < 0) {
            if (segpt) segpt[3 * j] = segpt[3 * j + 1] = segpt[3 * j + 2] = 0.0f;
            if (point) point[3 * j] = point[3 * j + 1] = point[3 * j + 2] = 0.0f;
            if (normal) normal[3 * j] = normal[3 * j + 1] = normal[3 * j + 2] = 0.0f;
            if (uv) uv[2 * j] = uv[2 * j + 1] = 0.0f;
            continue;
        }
        {
            const instance_t *in = &sc->instances[bi];
            const tri_t *t = &sc->meshes[in->mesh_index]->tris[bt];
            f3 q0 = apply_lre(in->pose, p0), q1 = apply_lre(in->pose, p1), dd = sg_sub(q1, q0), a, ab, ac, x, c, w, nn;
            float u0 = (1.0f - best.b2) - best.b1;
            xo_tri(t, in->scale, &a, &ab, &ac);
            x = mk3(q0.x + best.s * dd.x, q0.y + best.s * dd.y, q0.z + best.s * dd.z);
            c = sg_at(a, ab, ac, best.b1, best.b2);
            w = apply_lre(in->inv_pose, x);
            if (segpt) { segpt[3 * j] = w.x; segpt[3 * j + 1] = w.y; segpt[3 * j + 2] = w.z; }
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

/* the rule on one triangle given in scaled mesh space (host tests): q0 / q1 / a / ab / ac [3] -> out5 = s, b1, b2, d2, which */
void orcx_segment_on_triangle(const float *q0, const float *q1, const float *a, const float *ab, const float *ac, float *out5)
{
    sg_cand c = sg_triangle(mk3(q0[0], q0[1], q0[2]), mk3(q1[0], q1[1], q1[2]), mk3(a[0], a[1], a[2]), mk3(ab[0], ab[1], ab[2]),
                            mk3(ac[0], ac[1], ac[2]));
    out5[0] = c.s; out5[1] = c.b1; out5[2] = c.b2; out5[3] = c.d2; out5[4] = (float)c.which;
}

/* step 4 alone (host tests): q0 / d / e0 / f [3] -> out2 = s, u */
void orcx_segment_segment(const float *q0, const float *d, const float *e0, const float *f, float *out2)
{
    sg_segseg(mk3(q0[0], q0[1], q0[2]), mk3(d[0], d[1], d[2]), mk3(e0[0], e0[1], e0[2]), mk3(f[0], f[1], f[2]), &out2[0], &out2[1]);
}
