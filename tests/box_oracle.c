/* box_oracle.c -- TEST INFRASTRUCTURE: brute-force box queries over a scene, the specification of rt_count_in_boxes / rt_box_offsets /
 * rt_list_in_boxes / rt_occupancy_grid (include/rt_hip.h rule 11).  It includes tests/crossing_oracle.c unchanged
 * (and through it oracle/rt_oracle.c) for the scene, apply_lre and the scene triangle's A, AB, AC; it restates rule 11 on its own -- no
 * header is shared with the kernel, so an error in either copy shows as a difference.  For each box every (instance, triangle) is
 * visited in ascending order, which is already the list's order.  Built by tests/box_oracle.py with the oracle's own flags
 * (-ffp-contract=off). */
#include "crossing_oracle.c"

static float bo_dot(f3 a, f3 x) { return (a.x * x.x + a.y * x.y) + a.z * x.z; }
static f3 bo_cross(f3 u, f3 v) { return mk3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x); }
static f3 bo_sub(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }

/* step 5 on one axis: 1 = it separates the box (r[0..7], relative to C0) from the triangle (t[0..2], relative to C0) */
static int bo_separates(f3 ax, const f3 *r, const f3 *t)
{
    float minb = bo_dot(ax, r[0]), maxb = minb, d, mint, maxt;
    int k;
    for (k = 1; k < 8; k++) {
        d = bo_dot(ax, r[k]);
        minb = fminf(minb, d);
        maxb = fmaxf(maxb, d);
    }
    mint = fminf(fminf(bo_dot(ax, t[0]), bo_dot(ax, t[1])), bo_dot(ax, t[2]));
    maxt = fmaxf(fmaxf(bo_dot(ax, t[0]), bo_dot(ax, t[1])), bo_dot(ax, t[2]));
    return maxt < minb || maxb < mint;
}

/* rule 11 steps 2-5 on one pair in scaled mesh space: the mapped corners c[0..7] and the scene triangle (v[0], v[1], v[2]) -> 1 = a pair.
 * which (optional): 0 = a pair, 1 = step 4 failed, 2 + k = axis k of step 5 separated first */
static int bo_pair(const f3 *c, const f3 *v, int *which)
{
    f3 ql = c[0], qh = c[0], tl, th, r[8], t[3], f[3], ax[13];
    int k, m, n;
    for (k = 1; k < 8; k++) {
        ql = mk3(fminf(ql.x, c[k].x), fminf(ql.y, c[k].y), fminf(ql.z, c[k].z));
        qh = mk3(fmaxf(qh.x, c[k].x), fmaxf(qh.y, c[k].y), fmaxf(qh.z, c[k].z));
    }
    tl = mk3(fminf(fminf(v[0].x, v[1].x), v[2].x), fminf(fminf(v[0].y, v[1].y), v[2].y), fminf(fminf(v[0].z, v[1].z), v[2].z));
    th = mk3(fmaxf(fmaxf(v[0].x, v[1].x), v[2].x), fmaxf(fmaxf(v[0].y, v[1].y), v[2].y), fmaxf(fmaxf(v[0].z, v[1].z), v[2].z));
    if (which) *which = 1;
    if (!(tl.x <= qh.x && ql.x <= th.x && tl.y <= qh.y && ql.y <= th.y && tl.z <= qh.z && ql.z <= th.z)) return 0;
    for (k = 0; k < 8; k++) r[k] = bo_sub(c[k], c[0]);
    for (k = 0; k < 3; k++) t[k] = bo_sub(v[k], c[0]);
    f[0] = bo_sub(v[1], v[0]); f[1] = bo_sub(v[2], v[1]); f[2] = bo_sub(v[0], v[2]);
    ax[0] = r[1]; ax[1] = r[2]; ax[2] = r[4];
    ax[3] = bo_cross(f[0], f[1]);
    for (m = 0; m < 3; m++)
        for (n = 0; n < 3; n++) ax[4 + 3 * m + n] = bo_cross(r[1 << m], f[n]);
    for (k = 0; k < 13; k++) {
        if (which) *which = 2 + k;
        if (bo_separates(ax[k], r, t)) return 0;
    }
    if (which) *which = 0;
    return 1;
}

static int bo_valid(const float *B) { return B[0] <= B[3] && B[1] <= B[4] && B[2] <= B[5]; }

/* corner k of the world box B (lo then hi) under the pose */
static f3 bo_corner(const float *B, lre_t pose, int k)
{
    return apply_lre(pose, mk3(B[(k & 1) ? 3 : 0], B[(k & 2) ? 4 : 1], B[(k & 4) ? 5 : 2]));
}

/* one box: the pairs with instance i and triangle k, calling back in ascending (instance, triangle) order; returns the count */
typedef void (*bo_emit)(void *ctx, int inst, int tri);
static int bo_query(const OrcScene *sc, const float *B, bo_emit emit, void *ctx)
{
    int i, k, n = 0;
    if (!bo_valid(B)) return 0;
    for (i = 0; i < sc->ninst; i++) {
        const instance_t *in = &sc->instances[i];
        const OrcMesh *m = sc->meshes[in->mesh_index];
        f3 c[8];
        for (k = 0; k < 8; k++) c[k] = bo_corner(B, in->pose, k);
        for (k = 0; k < m->ntris; k++) {
            f3 a, ab, ac, v[3];
            xo_tri(&m->tris[k], in->scale, &a, &ab, &ac);
            v[0] = a;
            v[1] = mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z);
            v[2] = mk3(a.x + ac.x, a.y + ac.y, a.z + ac.z);
            if (!bo_pair(c, v, NULL)) continue;
            if (emit) emit(ctx, i, k);
            n++;
        }
    }
    return n;
}

/* rule 11 on one pair (host tests): box6 = world lo, hi; pose6 the instance's pose (world -> mesh, as an instance stores it); t9 the
 * triangle's vertices in scaled mesh space -> 1 = a pair; *which as bo_pair gives it, -1 = the box is not valid */
int orcb_pair(const float *box6, const float *pose6, const float *t9, int *which)
{
    f3 c[8], v[3];
    lre_t pose;
    int k;
    memcpy(&pose, pose6, sizeof pose);
    if (which) *which = -1;
    if (!bo_valid(box6)) return 0;
    for (k = 0; k < 8; k++) c[k] = bo_corner(box6, pose, k);
    for (k = 0; k < 3; k++) v[k] = mk3(t9[3 * k], t9[3 * k + 1], t9[3 * k + 2]);
    return bo_pair(c, v, which);
}

/* the eight mapped corners of step 2 (host tests): box6, pose6 -> out24 [8][3] */
void orcb_corners(const float *box6, const float *pose6, float *out24)
{
    lre_t pose;
    int k;
    memcpy(&pose, pose6, sizeof pose);
    for (k = 0; k < 8; k++) {
        f3 c = bo_corner(box6, pose, k);
        out24[3 * k] = c.x; out24[3 * k + 1] = c.y; out24[3 * k + 2] = c.z;
    }
}

/* n boxes [n][2][3] (world) -> count [n] */
void orcb_count_in_boxes(const OrcScene *sc, int64_t n, const float *boxes, int32_t *count)
{
    int64_t j;
    for (j = 0; j < n; j++) count[j] = bo_query(sc, boxes + 6 * j, NULL, NULL);
}

typedef struct {
    int64_t start, room, filled;
    int32_t *inst, *tri;
} bo_room;

static void bo_put(void *ctx, int i, int k)
{
    bo_room *r = (bo_room *)ctx;
    if (r->filled >= r->room) return;
    r->inst[r->start + r->filled] = i;
    r->tri[r->start + r->filled] = k;
    r->filled++;
}

/* rooms: offsets [n + 1] (CSR) or, with offsets NULL, max_hits per box.  Writes the first min(count, room) pairs of each box into its
 * room and pads the rest with -1; nothing outside the rooms.  count [n] = the full count. */
void orcb_list_in_boxes(const OrcScene *sc, int64_t n, const float *boxes, const int64_t *offsets, int32_t max_hits, int32_t *inst,
                        int32_t *tri, int32_t *count)
{
    int64_t j, s;
    for (j = 0; j < n; j++) {
        bo_room r;
        r.inst = inst; r.tri = tri; r.filled = 0;
        r.start = offsets ? offsets[j] : j * (int64_t)max_hits;
        r.room = offsets ? (offsets[j + 1] > offsets[j] ? offsets[j + 1] - offsets[j] : 0) : max_hits;
        count[j] = bo_query(sc, boxes + 6 * j, bo_put, &r);
        for (s = r.filled; s < r.room; s++) { inst[r.start + s] = -1; tri[r.start + s] = -1; }
    }
}
