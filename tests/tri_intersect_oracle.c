/* tri_intersect_oracle.c -- TEST INFRASTRUCTURE: brute-force triangle intersection queries over a scene, the specification of
 * rt_count_intersecting / rt_intersecting_offsets / rt_list_intersecting (include/rt_hip.h rule 10).  It
 * includes tests/crossing_oracle.c unchanged (and through it oracle/rt_oracle.c) for the scene, apply_lre / apply_euler and the
 * scene triangle's A, AB, AC; it restates rule 3's vertex form and rule 10 on its own -- no header is shared with the kernel, so an
 * error in either copy shows as a difference.  For each query every (instance, triangle) is visited in ascending order, which is
 * already the list's order.  Built by tests/tri_intersect_oracle.py with the oracle's own flags (-ffp-contract=off). */
#include "crossing_oracle.c"

/* rule 3 with tmax = 1 on the segment x -> y (o' = x, d' = y - x per component) against the triangle given by its vertices (a, b, c):
 * 1 = counted (*t = the t found), 0 = not */
static int ti_segment(f3 x, f3 y, f3 a, f3 b, f3 c, float *tout)
{
    f3 d = mk3(y.x - x.x, y.y - x.y, y.z - x.z);
    float adx = fabsf(d.x), ady = fabsf(d.y), adz = fabsf(d.z), big = adx, dz, sx, sy, sz;
    float pa[3], pb[3], pc[3], ax, ay, bx, by, cx, cy, U, V, W, det, T, t;
    int kz = 0, kx, ky, tmp;
    if (ady > big) { kz = 1; big = ady; }
    if (adz > big) kz = 2;
    kx = (kz + 1) % 3; ky = (kx + 1) % 3;
    dz = xo_c(d, kz);
    if (dz == 0.0f) return 0;                       /* a zero d' counts nothing */
    if (dz < 0.0f) { tmp = kx; kx = ky; ky = tmp; }
    sx = xo_c(d, kx) / dz; sy = xo_c(d, ky) / dz; sz = 1.0f / dz;
    pa[0] = xo_c(a, kx) - xo_c(x, kx); pa[1] = xo_c(a, ky) - xo_c(x, ky); pa[2] = xo_c(a, kz) - xo_c(x, kz);
    pb[0] = xo_c(b, kx) - xo_c(x, kx); pb[1] = xo_c(b, ky) - xo_c(x, ky); pb[2] = xo_c(b, kz) - xo_c(x, kz);
    pc[0] = xo_c(c, kx) - xo_c(x, kx); pc[1] = xo_c(c, ky) - xo_c(x, ky); pc[2] = xo_c(c, kz) - xo_c(x, kz);
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
    if (!(t > 0.0f && t <= 1.0f)) return 0;
    *tout = t;
    return 1;
}

/* step 3's box of three vertices (fminf / fmaxf, so one NaN coordinate of three is ignored, three give NaN) */
static void ti_bounds(const f3 *v, f3 *lo, f3 *hi)
{
    *lo = mk3(fminf(fminf(v[0].x, v[1].x), v[2].x), fminf(fminf(v[0].y, v[1].y), v[2].y), fminf(fminf(v[0].z, v[1].z), v[2].z));
    *hi = mk3(fmaxf(fmaxf(v[0].x, v[1].x), v[2].x), fmaxf(fmaxf(v[0].y, v[1].y), v[2].y), fmaxf(fmaxf(v[0].z, v[1].z), v[2].z));
}

/* rule 10 steps 3-5 on one pair in scaled mesh space: the query (q[0], q[1], q[2]), the scene triangle (t[0], t[1], t[2]) -> 1 = a pair,
 * with s0 / s1 the mesh-space points of the first and the last counting test (step 6); 0 = none */
static int ti_pair(const f3 *q, const f3 *t, f3 *s0, f3 *s1)
{
    f3 ql, qh, tl, th;
    int e, hit = 0;
    ti_bounds(q, &ql, &qh);
    ti_bounds(t, &tl, &th);
    if (!(tl.x <= qh.x && ql.x <= th.x && tl.y <= qh.y && ql.y <= th.y && tl.z <= qh.z && ql.z <= th.z)) return 0;
    for (e = 0; e < 6; e++) {
        const f3 *from = e < 3 ? q : t, *against = e < 3 ? t : q;
        f3 x = from[e % 3], y = from[(e + 1) % 3], p;
        float tt;
        if (!ti_segment(x, y, against[0], against[1], against[2], &tt)) continue;
        p = mk3(x.x + tt * (y.x - x.x), x.y + tt * (y.y - x.y), x.z + tt * (y.z - x.z));
        if (!hit) *s0 = p;
        *s1 = p;
        hit = 1;
    }
    return hit;
}

/* one query: the pairs with instance i and triangle k, calling back in ascending (instance, triangle) order; returns the count */
typedef void (*ti_emit)(void *ctx, int inst, int tri, f3 s0, f3 s1);
static int ti_query(const OrcScene *sc, const float *P, int32_t skip, ti_emit emit, void *ctx)
{
    int i, k, n = 0;
    for (i = 0; i < sc->ninst; i++) {
        const instance_t *in = &sc->instances[i];
        const OrcMesh *m = sc->meshes[in->mesh_index];
        f3 q[3];
        if (i == skip) continue;
        for (k = 0; k < 3; k++) q[k] = apply_lre(in->pose, mk3(P[3 * k], P[3 * k + 1], P[3 * k + 2]));
        for (k = 0; k < m->ntris; k++) {
            f3 a, ab, ac, t[3], s0, s1;
            xo_tri(&m->tris[k], in->scale, &a, &ab, &ac);
            t[0] = a;
            t[1] = mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z);
            t[2] = mk3(a.x + ac.x, a.y + ac.y, a.z + ac.z);
            if (!ti_pair(q, t, &s0, &s1)) continue;
            if (emit) emit(ctx, i, k, s0, s1);
            n++;
        }
    }
    return n;
}

/* rule 10 on one pair given in scaled mesh space (host tests): q9, t9 [3][3] -> 1 = a pair and seg6 [2][3] its segment ends */
int orct_pair(const float *q9, const float *t9, float *seg6)
{
    f3 q[3], t[3], s0 = mk3(0, 0, 0), s1 = mk3(0, 0, 0);
    int k, hit;
    for (k = 0; k < 3; k++) {
        q[k] = mk3(q9[3 * k], q9[3 * k + 1], q9[3 * k + 2]);
        t[k] = mk3(t9[3 * k], t9[3 * k + 1], t9[3 * k + 2]);
    }
    hit = ti_pair(q, t, &s0, &s1);
    seg6[0] = s0.x; seg6[1] = s0.y; seg6[2] = s0.z; seg6[3] = s1.x; seg6[4] = s1.y; seg6[5] = s1.z;
    return hit;
}

/* one segment test of step 4 (host tests): x -> y against the triangle (a, b, c), each [3] -> 1 = counted and *t */
int orct_segment(const float *x, const float *y, const float *a, const float *b, const float *c, float *t)
{
    return ti_segment(mk3(x[0], x[1], x[2]), mk3(y[0], y[1], y[2]), mk3(a[0], a[1], a[2]), mk3(b[0], b[1], b[2]), mk3(c[0], c[1], c[2]), t);
}

/* n query triangles tris [n][3][3] (world), skip [n] (NULL = none) -> count [n] */
void orct_count_intersecting(const OrcScene *sc, int64_t n, const float *tris, const int32_t *skip, int32_t *count)
{
    int64_t j;
    for (j = 0; j < n; j++) count[j] = ti_query(sc, tris + 9 * j, skip ? skip[j] : -1, NULL, NULL);
}

typedef struct {
    const OrcScene *sc;
    int64_t start, room, filled;
    int32_t *inst, *tri;
    float *normal, *segment;
} ti_room;

static void ti_put(void *ctx, int i, int k, f3 s0, f3 s1)
{
    ti_room *r = (ti_room *)ctx;
    const instance_t *in = &r->sc->instances[i];
    const tri_t *t = &r->sc->meshes[in->mesh_index]->tris[k];
    int64_t q = r->start + r->filled;
    f3 nn, w0, w1;
    if (r->filled >= r->room) return;
    nn = apply_euler(in->inv_rotation, t->normal);                              /* rt_closest_points' normal (raycast.cu:115-122) */
    nn.x *= in->scale.x; nn.y *= in->scale.y; nn.z *= in->scale.z;
    nn = normalize3(nn);
    w0 = apply_lre(in->inv_pose, s0);                                           /* closest_points' map to world */
    w1 = apply_lre(in->inv_pose, s1);
    r->inst[q] = i; r->tri[q] = k;
    r->normal[3 * q] = nn.x; r->normal[3 * q + 1] = nn.y; r->normal[3 * q + 2] = nn.z;
    r->segment[6 * q] = w0.x; r->segment[6 * q + 1] = w0.y; r->segment[6 * q + 2] = w0.z;
    r->segment[6 * q + 3] = w1.x; r->segment[6 * q + 4] = w1.y; r->segment[6 * q + 5] = w1.z;
    r->filled++;
}

/* rooms: offsets [n + 1] (CSR) or, with offsets NULL, max_hits per query.  Writes the first min(count, room) pairs of each query into
 * its room and pads the rest (instance = triangle = -1, normal and segment 0); nothing outside the rooms.  count [n] = the full count. */
void orct_list_intersecting(const OrcScene *sc, int64_t n, const float *tris, const int32_t *skip, const int64_t *offsets, int32_t max_hits,
                            int32_t *inst, int32_t *tri, float *normal, float *segment, int32_t *count)
{
    int64_t j, s;
    for (j = 0; j < n; j++) {
        ti_room r;
        r.sc = sc; r.inst = inst; r.tri = tri; r.normal = normal; r.segment = segment; r.filled = 0;
        r.start = offsets ? offsets[j] : j * (int64_t)max_hits;
        r.room = offsets ? (offsets[j + 1] > offsets[j] ? offsets[j + 1] - offsets[j] : 0) : max_hits;
        count[j] = ti_query(sc, tris + 9 * j, skip ? skip[j] : -1, ti_put, &r);
        for (s = r.filled; s < r.room; s++) {
            int64_t q = r.start + s, c;
            inst[q] = -1; tri[q] = -1;
            for (c = 0; c < 3; c++) normal[3 * q + c] = 0.0f;
            for (c = 0; c < 6; c++) segment[6 * q + c] = 0.0f;
        }
    }
}
