/* sweep_oracle.c -- TEST INFRASTRUCTURE: the brute-force first contact of a sphere that moves along a segment, the specification
 * of rt_sweep_spheres (include/rt_hip.h rule 16).  It includes tests/point_oracle.c (and through it
 * oracle/rt_oracle.c, unchanged) for its scene (OrcScene), apply_lre and pt_weights' sequence, and restates the fp32 sequence of
 * the rule on its own -- no header is shared with the kernel, so an error in either copy shows as a difference.  Every (instance,
 * triangle) is visited and every candidate in range is priced; there is no tree and no skipping.  Built by tests/sweep_oracle.py
 * with the oracle's own flags (oracle/Makefile: -ffp-contract=off). */
#include "point_oracle.c"

/* reach = (r + r * SW_KR) + M * SW_KM: rule 16 step 3's constants (the float64 study of tests/test_sweep_host.py fixes them) */
#ifndef SW_KR
#define SW_KR 0x1p-20f
#endif
#ifndef SW_KM
#define SW_KM 0x1p-20f
#endif

static f3 sw_add(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
static f3 sw_along(f3 p, float s, f3 d) { return mk3(p.x + s * d.x, p.y + s * d.y, p.z + s * d.z); }
static f3 sw_off(f3 p, float s, f3 d) { return mk3(p.x - s * d.x, p.y - s * d.y, p.z - s * d.z); }
static float sw_absmax(float m, float x)
{
    float a = fabsf(x);
    return a > m ? a : m;
}

/* step 3's bound in d2: the radius widened by a relative term and by a term in the query's largest mapped coordinate */
static float sw_reach2(float r, f3 q0, f3 q1)
{
    float m = 0.0f, rw;
    m = sw_absmax(m, q0.x); m = sw_absmax(m, q0.y); m = sw_absmax(m, q0.z);
    m = sw_absmax(m, q1.x); m = sw_absmax(m, q1.y); m = sw_absmax(m, q1.z);
    rw = (r + r * SW_KR) + m * SW_KM;
    return rw * rw;
}

typedef struct { float s, b1, b2, d2; int which; } sw_cand;

/* step 3: the candidate time s priced; it becomes the triangle's candidate when it is valid and earlier than the one so far */
static void sw_try(sw_cand *best, int which, f3 q0, f3 d, f3 a, f3 ab, f3 ac, float reach2, float s)
{
    f3 x;
    float b1, b2, d2;
    if (!(s >= 0.0f && s <= 1.0f)) return;
    if (best->which >= 0 && !(s < best->s)) return;
    x = sw_along(q0, s, d);
    pt_weights(x, a, ab, ac, &b1, &b2);
    d2 = pt_len2(pt_sub(x, pt_at(a, ab, ac, b1, b2)));
    if (!(d2 <= reach2)) return;
    best->s = s; best->b1 = b1; best->b2 = b2; best->d2 = d2; best->which = which;
}

/* the entry root of the centre's line q0 + s*d against the sphere of radius r about v, closest-approach form; aa = dot(d, d) > 0 */
static void sw_vertex(sw_cand *best, int which, f3 q0, f3 d, float aa, f3 a, f3 ab, f3 ac, float reach2, float r2, f3 v)
{
    f3 w = pt_sub(q0, v), dv;
    float smid = -pt_dot(w, d) / aa, dp2;
    dv = sw_along(w, smid, d);
    dp2 = pt_len2(dv);
    if (dp2 <= r2) sw_try(best, which, q0, d, a, ab, ac, reach2, smid - sqrtf((r2 - dp2) / aa));
}

/* the entry root against the infinite cylinder of radius r about the line e0 + u*f */
static void sw_edge(sw_cand *best, int which, f3 q0, f3 d, f3 a, f3 ab, f3 ac, float reach2, float r2, f3 e0, f3 f)
{
    float ff = pt_dot(f, f), td, tw, ap, smid, dp2;
    f3 w, dp, wp, dv;
    if (!(ff > 0.0f)) return;
    w = pt_sub(q0, e0);
    td = pt_dot(d, f) / ff; tw = pt_dot(w, f) / ff;
    dp = sw_off(d, td, f); wp = sw_off(w, tw, f);
    ap = pt_dot(dp, dp);
    if (!(ap > 0.0f)) return;
    smid = -pt_dot(wp, dp) / ap;
    dv = sw_along(wp, smid, dp);
    dp2 = pt_len2(dv);
    if (dp2 <= r2) sw_try(best, which, q0, d, a, ab, ac, reach2, smid - sqrtf((r2 - dp2) / ap));
}

/* steps 2-3 on one triangle in scaled mesh space: which = -1 when it has no valid candidate */
static sw_cand sw_triangle(f3 q0, f3 q1, float r, float reach2, f3 a, f3 ab, f3 ac)
{
    sw_cand best = {0.0f, 0.0f, 0.0f, 0.0f, -1};
    f3 d = pt_sub(q1, q0), n, u, w;
    float aa = pt_dot(d, d), r2 = r * r, m = 0.0f;
    sw_try(&best, 0, q0, d, a, ab, ac, reach2, 0.0f);
    if (!(aa > 0.0f)) return best;
    /* face: the plane offset by r on q0's side, approached */
    n = mk3(ab.y * ac.z - ab.z * ac.y, ab.z * ac.x - ab.x * ac.z, ab.x * ac.y - ab.y * ac.x);
    m = sw_absmax(m, n.x); m = sw_absmax(m, n.y); m = sw_absmax(m, n.z);
    if (m > 0.0f) {
        float lu, h0, vn, g = 0.0f, v = 0.0f;
        u = mk3(n.x / m, n.y / m, n.z / m);
        lu = sqrtf(pt_len2(u));
        w = pt_sub(q0, a);
        h0 = pt_dot(u, w); vn = pt_dot(u, d);
        if (h0 >= 0.0f) { g = h0 - r * lu; v = -vn; }
        else if (h0 < 0.0f) { g = -h0 - r * lu; v = vn; }
        if (v > 0.0f) sw_try(&best, 1, q0, d, a, ab, ac, reach2, g / v);
    }
    sw_edge(&best, 2, q0, d, a, ab, ac, reach2, r2, a, ab);
    sw_edge(&best, 3, q0, d, a, ab, ac, reach2, r2, a, ac);
    sw_edge(&best, 4, q0, d, a, ab, ac, reach2, r2, sw_add(a, ab), pt_sub(ac, ab));
    sw_vertex(&best, 5, q0, d, aa, a, ab, ac, reach2, r2, a);
    sw_vertex(&best, 6, q0, d, aa, a, ab, ac, reach2, r2, sw_add(a, ab));
    sw_vertex(&best, 7, q0, d, aa, a, ab, ac, reach2, r2, sw_add(a, ac));
    return best;
}

static void sw_put3(float *o, int64_t j, f3 v) { if (o) { o[3 * j] = v.x; o[3 * j + 1] = v.y; o[3 * j + 2] = v.z; } }

/* n sweeps segs [n][2][3], radius [n].  Outputs, each optional: time / dist [n] (FLT_MAX on a miss), inst / tri [n] (-1), centre /
 * point / normal / cnormal [n][3], bary / uv [n][2] (0 on a miss), hit [n], which [n] (the winning candidate 0..7, -1 on a miss:
 * the tests' coverage counts).  only_inst >= 0: that instance alone. */
void orcx_sweep_spheres(const OrcScene *sc, int64_t n, const float *segs, const float *radius, int only_inst, float *time, float *dist,
                        int32_t *inst, int32_t *tri, float *centre, float *point, float *normal, float *cnormal, float *bary, float *uv,
                        int32_t *hit, int32_t *which)
{
    int64_t j;
    for (j = 0; j < n; j++) {
        f3 p0 = mk3(segs[6 * j], segs[6 * j + 1], segs[6 * j + 2]), p1 = mk3(segs[6 * j + 3], segs[6 * j + 4], segs[6 * j + 5]);
        f3 zero = mk3(0.0f, 0.0f, 0.0f);
        float r = radius[j];
        sw_cand best = {0.0f, 0.0f, 0.0f, 0.0f, -1};
        int bi = -1, bt = -1, i, k;
        for (i = 0; i < sc->ninst && r >= 0.0f; i++) {
            const instance_t *in = &sc->instances[i];
            const OrcMesh *m = sc->meshes[in->mesh_index];
            f3 q0 = apply_lre(in->pose, p0), q1 = apply_lre(in->pose, p1);
            float reach2 = sw_reach2(r, q0, q1);
            if (only_inst >= 0 && i != only_inst) continue;
            for (k = 0; k < m->ntris; k++) {
                f3 a, ab, ac;
                sw_cand c;
                pt_tri(&m->tris[k], in->scale, &a, &ab, &ac);
                c = sw_triangle(q0, q1, r, reach2, a, ab, ac);
                if (c.which < 0) continue;
                if (bi < 0 || c.s < best.s ||
                    (c.s == best.s && (c.d2 < best.d2 || (c.d2 == best.d2 && (i < bi || (i == bi && k < bt)))))) { best = c; bi = i; bt = k; }
            }
        }
        if (time) time[j] = bi >= 0 ? best.s : FLT_MAX;
        if (dist) dist[j] = bi >= 0 ? sqrtf(best.d2) : FLT_MAX;
        if (inst) inst[j] = bi;
        if (tri) tri[j] = bt;
        if (bary) { bary[2 * j] = bi >= 0 ? best.b1 : 0.0f; bary[2 * j + 1] = bi >= 0 ? best.b2 : 0.0f; }
        if (hit) hit[j] = bi >= 0 ? 1 : 0;
        if (which) which[j] = bi >= 0 ? best.which : -1;
        if (bi < 0) {
            sw_put3(centre, j, zero); sw_put3(point, j, zero); sw_put3(normal, j, zero); sw_put3(cnormal, j, zero);
            if (uv) uv[2 * j] = uv[2 * j + 1] = 0.0f;
            continue;
        }
        {
            const instance_t *in = &sc->instances[bi];
            const tri_t *t = &sc->meshes[in->mesh_index]->tris[bt];
            f3 q0 = apply_lre(in->pose, p0), q1 = apply_lre(in->pose, p1), dd = pt_sub(q1, q0), a, ab, ac, x, c, nn, e;
            float u0 = (1.0f - best.b2) - best.b1;
            pt_tri(t, in->scale, &a, &ab, &ac);
            x = sw_along(q0, best.s, dd);
            c = pt_at(a, ab, ac, best.b1, best.b2);
            sw_put3(centre, j, apply_lre(in->inv_pose, x));
            sw_put3(point, j, apply_lre(in->inv_pose, c));
            nn = apply_euler(in->inv_rotation, t->normal);
            nn.x *= in->scale.x; nn.y *= in->scale.y; nn.z *= in->scale.z;
            nn = normalize3(nn);
            sw_put3(normal, j, nn);
            e = pt_sub(x, c);
            if (best.d2 > 0.0f) {
                float len = sqrtf(best.d2);
                nn = apply_euler(in->inv_rotation, mk3(e.x / len, e.y / len, e.z / len));
            }
            sw_put3(cnormal, j, nn);
            if (uv) {
                uv[2 * j] = (u0 * t->uv[0].x + best.b1 * t->uv[1].x) + best.b2 * t->uv[2].x;
                uv[2 * j + 1] = (u0 * t->uv[0].y + best.b1 * t->uv[1].y) + best.b2 * t->uv[2].y;
            }
        }
    }
}

/* the rule on one triangle given in scaled mesh space (host tests): q0 / q1 / a / ab / ac [3], r -> out5 = s, b1, b2, d2, which */
void orcx_sweep_on_triangle(const float *q0, const float *q1, float r, const float *a, const float *ab, const float *ac, float *out5)
{
    f3 Q0 = mk3(q0[0], q0[1], q0[2]), Q1 = mk3(q1[0], q1[1], q1[2]);
    sw_cand c = {0.0f, 0.0f, 0.0f, 0.0f, -1};
    if (r >= 0.0f)
        c = sw_triangle(Q0, Q1, r, sw_reach2(r, Q0, Q1), mk3(a[0], a[1], a[2]), mk3(ab[0], ab[1], ab[2]), mk3(ac[0], ac[1], ac[2]));
    out5[0] = c.s; out5[1] = c.b1; out5[2] = c.b2; out5[3] = c.d2; out5[4] = (float)c.which;
}

/* step 3's bound alone (host tests) */
float orcx_sweep_reach2(const float *q0, const float *q1, float r)
{
    return sw_reach2(r, mk3(q0[0], q0[1], q0[2]), mk3(q1[0], q1[1], q1[2]));
}
