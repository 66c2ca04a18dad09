/* section_oracle.c -- TEST INFRASTRUCTURE: brute-force plane sections over a scene, the specification of rt_count_sections /
 * rt_section_offsets / rt_list_sections (include/rt_hip.h rule 12).  It includes tests/crossing_oracle.c unchanged
 * (and through it oracle/rt_oracle.c) for the scene, apply_lre / apply_euler and the scene triangle's A, AB, AC; it restates rule 12 on
 * its own -- no header is shared with the kernel, so an error in either copy shows as a difference.  For each plane every (instance,
 * triangle) is visited in ascending order, which is already the list's order.  Built by tests/section_oracle.py with the oracle's own
 * flags (-ffp-contract=off). */
#include "crossing_oracle.c"

/* step 4: each difference rounded, each product rounded, then the two sums */
static float so_height(f3 n, f3 p, f3 x) { return (n.x * (x.x - p.x) + n.y * (x.y - p.y)) + n.z * (x.z - p.z); }

/* step 6 on one edge: the cut point from the BELOW end x (height hx < 0) towards the ABOVE end y (height hy >= 0) */
static f3 so_cut(f3 x, float hx, f3 y, float hy)
{
    float t = hx / (hx - hy);
    return mk3(x.x + t * (y.x - x.x), x.y + t * (y.y - x.y), x.z + t * (y.z - x.z));
}

/* rule 12 steps 4-6 on one pair in scaled mesh space: the plane (p, n) and the scene triangle (v[0], v[1], v[2]) -> 1 = a pair, with
 * e0 / e1 the mesh-space ends of the segment; h[0..2] (optional) the three heights */
static int so_pair(f3 p, f3 n, const f3 *v, f3 *e0, f3 *e1, float *h3)
{
    float h[3];
    int k, above = 0, below = 0;
    for (k = 0; k < 3; k++) {
        h[k] = so_height(n, p, v[k]);
        if (h3) h3[k] = h[k];
        if (h[k] >= 0.0f) above++;
        else if (h[k] < 0.0f) below++;
    }
    if (above + below != 3 || above == 0 || below == 0) return 0;
    for (k = 0; k < 3; k++) {                       /* the cycle's edge v[k] -> v[k + 1] */
        int m = (k + 1) % 3;
        if (h[k] >= 0.0f && h[m] < 0.0f) *e0 = so_cut(v[m], h[m], v[k], h[k]);         /* ABOVE -> BELOW: end 0 */
        else if (h[k] < 0.0f && h[m] >= 0.0f) *e1 = so_cut(v[k], h[k], v[m], h[m]);    /* BELOW -> ABOVE: end 1 */
    }
    return 1;
}

static int so_valid(const float *B) { return B[3] != 0.0f || B[4] != 0.0f || B[5] != 0.0f; }

/* one plane B (point then normal): the pairs with instance i and triangle k and the mesh-space ends, calling back in ascending
 * (instance, triangle) order; returns the count */
typedef void (*so_emit)(void *ctx, int inst, int tri, f3 e0, f3 e1);
static int so_query(const OrcScene *sc, const float *B, so_emit emit, void *ctx)
{
    int i, k, n = 0;
    if (!so_valid(B)) return 0;
    for (i = 0; i < sc->ninst; i++) {
        const instance_t *in = &sc->instances[i];
        const OrcMesh *m = sc->meshes[in->mesh_index];
        f3 p = apply_lre(in->pose, mk3(B[0], B[1], B[2]));
        f3 nn = apply_euler(mk3(in->pose.yaw, in->pose.pitch, in->pose.roll), mk3(B[3], B[4], B[5]));
        for (k = 0; k < m->ntris; k++) {
            f3 a, ab, ac, v[3], e0 = mk3(0, 0, 0), e1 = mk3(0, 0, 0);
            xo_tri(&m->tris[k], in->scale, &a, &ab, &ac);
            v[0] = a;
            v[1] = mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z);
            v[2] = mk3(a.x + ac.x, a.y + ac.y, a.z + ac.z);
            if (!so_pair(p, nn, v, &e0, &e1, NULL)) continue;
            if (emit) emit(ctx, i, k, e0, e1);
            n++;
        }
    }
    return n;
}

/* rule 12 on one pair (host tests): plane6 = world point, normal; pose6 the instance's pose (world -> mesh, as an instance stores it);
 * t9 the triangle's vertices in scaled mesh space -> 1 = a pair; seg6 [2][3] the MESH-space ends (0 when no pair), h3 the heights
 * (0 for an invalid plane); mapped6 (optional) p' and n' */
int orcs_pair(const float *plane6, const float *pose6, const float *t9, float *seg6, float *h3, float *mapped6)
{
    f3 v[3], p, n, e0 = mk3(0, 0, 0), e1 = mk3(0, 0, 0);
    lre_t pose;
    int k, hit = 0;
    memcpy(&pose, pose6, sizeof pose);
    p = apply_lre(pose, mk3(plane6[0], plane6[1], plane6[2]));
    n = apply_euler(mk3(pose.yaw, pose.pitch, pose.roll), mk3(plane6[3], plane6[4], plane6[5]));
    if (mapped6) { mapped6[0] = p.x; mapped6[1] = p.y; mapped6[2] = p.z; mapped6[3] = n.x; mapped6[4] = n.y; mapped6[5] = n.z; }
    for (k = 0; k < 3; k++) { v[k] = mk3(t9[3 * k], t9[3 * k + 1], t9[3 * k + 2]); h3[k] = 0.0f; }
    if (so_valid(plane6)) hit = so_pair(p, n, v, &e0, &e1, h3);
    seg6[0] = e0.x; seg6[1] = e0.y; seg6[2] = e0.z; seg6[3] = e1.x; seg6[4] = e1.y; seg6[5] = e1.z;
    return hit;
}

/* n planes [n][2][3] (world) -> count [n] */
void orcs_count_sections(const OrcScene *sc, int64_t n, const float *planes, int32_t *count)
{
    int64_t j;
    for (j = 0; j < n; j++) count[j] = so_query(sc, planes + 6 * j, NULL, NULL);
}

typedef struct {
    const OrcScene *sc;
    int64_t start, room, filled;
    int32_t *inst, *tri;
    float *segment, *normal;
} so_room;

static void so_put(void *ctx, int i, int k, f3 e0, f3 e1)
{
    so_room *r = (so_room *)ctx;
    const instance_t *in = &r->sc->instances[i];
    const tri_t *t = &r->sc->meshes[in->mesh_index]->tris[k];
    int64_t q = r->start + r->filled;
    f3 nn, w0, w1;
    if (r->filled >= r->room) return;
    nn = apply_euler(in->inv_rotation, t->normal);                              /* rt_closest_points' normal (raycast.cu:115-122) */
    nn.x *= in->scale.x; nn.y *= in->scale.y; nn.z *= in->scale.z;
    nn = normalize3(nn);
    w0 = apply_lre(in->inv_pose, e0);                                           /* closest_points' map to world */
    w1 = apply_lre(in->inv_pose, e1);
    r->inst[q] = i; r->tri[q] = k;
    r->segment[6 * q] = w0.x; r->segment[6 * q + 1] = w0.y; r->segment[6 * q + 2] = w0.z;
    r->segment[6 * q + 3] = w1.x; r->segment[6 * q + 4] = w1.y; r->segment[6 * q + 5] = w1.z;
    r->normal[3 * q] = nn.x; r->normal[3 * q + 1] = nn.y; r->normal[3 * q + 2] = nn.z;
    r->filled++;
}

/* rooms: offsets [n + 1] (CSR) or, with offsets NULL, max_hits per plane.  Writes the first min(count, room) pairs of each plane into
 * its room and pads the rest (instance = triangle = -1, segment and normal 0); nothing outside the rooms.  count [n] = the full count. */
void orcs_list_sections(const OrcScene *sc, int64_t n, const float *planes, const int64_t *offsets, int32_t max_hits, int32_t *inst,
                        int32_t *tri, float *segment, float *normal, int32_t *count)
{
    int64_t j, s;
    for (j = 0; j < n; j++) {
        so_room r;
        r.sc = sc; r.inst = inst; r.tri = tri; r.segment = segment; r.normal = normal; r.filled = 0;
        r.start = offsets ? offsets[j] : j * (int64_t)max_hits;
        r.room = offsets ? (offsets[j + 1] > offsets[j] ? offsets[j + 1] - offsets[j] : 0) : max_hits;
        count[j] = so_query(sc, planes + 6 * j, so_put, &r);
        for (s = r.filled; s < r.room; s++) {
            int64_t q = r.start + s, c;
            inst[q] = -1; tri[q] = -1;
            for (c = 0; c < 6; c++) segment[6 * q + c] = 0.0f;
            for (c = 0; c < 3; c++) normal[3 * q + c] = 0.0f;
        }
    }
}
