/* region_oracle.c -- TEST INFRASTRUCTURE: brute-force region queries over a scene, the specification of rt_count_in_regions /
 * rt_region_offsets / rt_list_in_regions (include/rt_hip.h rule 15).  It includes tests/crossing_oracle.c
 * unchanged (and through it oracle/rt_oracle.c) for the scene, apply_lre / apply_euler and the scene triangle's A, AB, AC; it restates
 * rule 15 on its own, the clip of step 5 included -- no header is shared with the kernel, so an error in either copy shows as a
 * difference.  Every plane is clipped against, also those that have every current vertex above (the kernel may skip them: the same
 * bits).  For each region every (instance, triangle) is visited in ascending order, which is already the list's order.  Built by
 * tests/region_oracle.py with the oracle's own flags (-ffp-contract=off). */
#include "crossing_oracle.c"

#define RO_MAX_PLANES 8
#define RO_MAX_VERTS 11             /* 3 + RO_MAX_PLANES */

/* rule 12 step 4: each difference rounded, each product rounded, then the two sums */
static float ro_height(f3 n, f3 p, f3 x) { return (n.x * (x.x - p.x) + n.y * (x.y - p.y)) + n.z * (x.z - p.z); }

/* rule 12 step 6's cut, from the end x that is not above towards the end y that is */
static f3 ro_cut(f3 x, float hx, f3 y, float hy)
{
    float t = hx / (hx - hy);
    return mk3(x.x + t * (y.x - x.x), x.y + t * (y.y - x.y), x.z + t * (y.z - x.z));
}

/* rule 15 steps 3-5 on one pair in scaled mesh space: K mapped planes (p[k], n[k]) and the scene triangle v[0..2] -> 0 = no pair,
 * 1 = a pair that needed the clip (inside = 0), 2 = wholly inside (inside = 1).  poly / m (optional): the clipped polygon */
static int ro_pair(int K, const f3 *p, const f3 *n, const f3 *v, f3 *poly, int *mout)
{
    f3 cur[RO_MAX_VERTS], nxt[RO_MAX_VERTS];
    float g[RO_MAX_VERTS];
    int k, i, m = 3, allin = 1;
    if (mout) *mout = 0;
    for (k = 0; k < K; k++) {                       /* step 3 */
        int above = 0, below = 0;
        for (i = 0; i < 3; i++) {
            float h = ro_height(n[k], p[k], v[i]);
            if (h >= 0.0f) above++;
            else if (h < 0.0f) below++;
        }
        if (above + below != 3 || below == 3) return 0;
        if (above != 3) allin = 0;
    }
    for (i = 0; i < 3; i++) cur[i] = v[i];
    if (!allin) {
        for (k = 0; k < K; k++) {                   /* step 5 */
            int o = 0;
            for (i = 0; i < m; i++) g[i] = ro_height(n[k], p[k], cur[i]);
            for (i = 0; i < m; i++) {
                int j = (i + 1) % m, ai = g[i] >= 0.0f, aj = g[j] >= 0.0f;
                if (ai && o < RO_MAX_VERTS) nxt[o++] = cur[i];
                if (ai != aj && o < RO_MAX_VERTS) nxt[o++] = ai ? ro_cut(cur[j], g[j], cur[i], g[i]) : ro_cut(cur[i], g[i], cur[j], g[j]);
            }
            m = o;
            for (i = 0; i < m; i++) cur[i] = nxt[i];
            if (m == 0) return 0;
        }
    }
    if (poly) for (i = 0; i < m; i++) poly[i] = cur[i];
    if (mout) *mout = m;
    return allin ? 2 : 1;
}

static int ro_valid(int K, const float *R)
{
    int k;
    if (K < 1 || K > RO_MAX_PLANES) return 0;
    for (k = 0; k < K; k++)
        if (!(R[6 * k + 3] != 0.0f || R[6 * k + 4] != 0.0f || R[6 * k + 5] != 0.0f)) return 0;
    return 1;
}

static void ro_map(int K, const float *R, lre_t pose, f3 *p, f3 *n)
{
    int k;
    for (k = 0; k < K; k++) {
        p[k] = apply_lre(pose, mk3(R[6 * k], R[6 * k + 1], R[6 * k + 2]));
        n[k] = apply_euler(mk3(pose.yaw, pose.pitch, pose.roll), mk3(R[6 * k + 3], R[6 * k + 4], R[6 * k + 5]));
    }
}

/* one region R ([K][2][3]): the pairs with instance i, triangle k and the inside flag, calling back in ascending (instance, triangle)
 * order; returns the count, *inside the number of wholly-inside pairs */
typedef void (*ro_emit)(void *ctx, int inst, int tri, int inside);
static int ro_query(const OrcScene *sc, int K, const float *R, ro_emit emit, void *ctx, int *inside)
{
    int i, k, n = 0;
    *inside = 0;
    if (!ro_valid(K, R)) return 0;
    for (i = 0; i < sc->ninst; i++) {
        const instance_t *in = &sc->instances[i];
        const OrcMesh *m = sc->meshes[in->mesh_index];
        f3 p[RO_MAX_PLANES], nn[RO_MAX_PLANES];
        ro_map(K, R, in->pose, p, nn);
        for (k = 0; k < m->ntris; k++) {
            f3 a, ab, ac, v[3];
            int r;
            xo_tri(&m->tris[k], in->scale, &a, &ab, &ac);
            v[0] = a;
            v[1] = mk3(a.x + ab.x, a.y + ab.y, a.z + ab.z);
            v[2] = mk3(a.x + ac.x, a.y + ac.y, a.z + ac.z);
            r = ro_pair(K, p, nn, v, NULL, NULL);
            if (!r) continue;
            if (emit) emit(ctx, i, k, r == 2);
            if (r == 2) (*inside)++;
            n++;
        }
    }
    return n;
}

/* rule 15 on one pair (host tests): region [K][2][3] world; pose6 the instance's pose (world -> mesh, as an instance stores it); t9 the
 * triangle's vertices in scaled mesh space -> 0 no pair, 1 a pair with inside = 0, 2 a pair with inside = 1; heights [K][3] (0 for an
 * invalid region); poly [11][3] and *m the clipped polygon in MESH space (m = 3, the triangle, when wholly inside; 0 when no pair);
 * mapped [K][2][3] (optional) p' and n' */
int orcr_pair(int K, const float *region, const float *pose6, const float *t9, float *heights, float *poly, int32_t *m, float *mapped)
{
    f3 v[3], p[RO_MAX_PLANES], n[RO_MAX_PLANES], out[RO_MAX_VERTS];
    lre_t pose;
    int k, i, r, mm = 0;
    *m = 0;
    if (K < 1 || K > RO_MAX_PLANES) return 0;
    memcpy(&pose, pose6, sizeof pose);
    ro_map(K, region, pose, p, n);
    for (i = 0; i < 3; i++) v[i] = mk3(t9[3 * i], t9[3 * i + 1], t9[3 * i + 2]);
    for (k = 0; k < K; k++) {
        if (mapped) {
            mapped[6 * k] = p[k].x; mapped[6 * k + 1] = p[k].y; mapped[6 * k + 2] = p[k].z;
            mapped[6 * k + 3] = n[k].x; mapped[6 * k + 4] = n[k].y; mapped[6 * k + 5] = n[k].z;
        }
        for (i = 0; i < 3; i++) heights[3 * k + i] = ro_valid(K, region) ? ro_height(n[k], p[k], v[i]) : 0.0f;
    }
    if (!ro_valid(K, region)) return 0;
    r = ro_pair(K, p, n, v, out, &mm);
    for (i = 0; i < mm; i++) { poly[3 * i] = out[i].x; poly[3 * i + 1] = out[i].y; poly[3 * i + 2] = out[i].z; }
    *m = mm;
    return r;
}

/* n regions [n][K][2][3] (world) -> count [n], inside [n] */
void orcr_count_in_regions(const OrcScene *sc, int64_t n, int K, const float *regions, int32_t *count, int32_t *inside)
{
    int64_t j;
    for (j = 0; j < n; j++) {
        int ins;
        count[j] = ro_query(sc, K, regions + 6 * (int64_t)K * j, NULL, NULL, &ins);
        inside[j] = ins;
    }
}

typedef struct {
    const OrcScene *sc;
    int64_t start, room, filled;
    int32_t *inst, *tri;
    uint8_t *inside;
    float *normal;
} ro_room;

static void ro_put(void *ctx, int i, int k, int inside)
{
    ro_room *r = (ro_room *)ctx;
    const instance_t *in = &r->sc->instances[i];
    const tri_t *t = &r->sc->meshes[in->mesh_index]->tris[k];
    int64_t q = r->start + r->filled;
    f3 nn;
    if (r->filled >= r->room) return;
    nn = apply_euler(in->inv_rotation, t->normal);                              /* rt_closest_points' normal */
    nn.x *= in->scale.x; nn.y *= in->scale.y; nn.z *= in->scale.z;
    nn = normalize3(nn);
    r->inst[q] = i; r->tri[q] = k; r->inside[q] = (uint8_t)inside;
    r->normal[3 * q] = nn.x; r->normal[3 * q + 1] = nn.y; r->normal[3 * q + 2] = nn.z;
    r->filled++;
}

/* rooms: offsets [n + 1] (CSR) or, with offsets NULL, max_hits per region.  Writes the first min(count, room) pairs of each region
 * into its room and pads the rest (instance = triangle = -1, inside 0, normal 0); nothing outside the rooms.  count [n] = the full
 * count. */
void orcr_list_in_regions(const OrcScene *sc, int64_t n, int K, const float *regions, const int64_t *offsets, int32_t max_hits,
                          int32_t *inst, int32_t *tri, uint8_t *inside, float *normal, int32_t *count)
{
    int64_t j, s;
    for (j = 0; j < n; j++) {
        ro_room r;
        int ins;
        r.sc = sc; r.inst = inst; r.tri = tri; r.inside = inside; r.normal = normal; r.filled = 0;
        r.start = offsets ? offsets[j] : j * (int64_t)max_hits;
        r.room = offsets ? (offsets[j + 1] > offsets[j] ? offsets[j + 1] - offsets[j] : 0) : max_hits;
        count[j] = ro_query(sc, K, regions + 6 * (int64_t)K * j, ro_put, &r, &ins);
        for (s = r.filled; s < r.room; s++) {
            int64_t q = r.start + s, c;
            inst[q] = -1; tri[q] = -1; inside[q] = 0;
            for (c = 0; c < 3; c++) normal[3 * q + c] = 0.0f;
        }
    }
}
