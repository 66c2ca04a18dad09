/* nearby_oracle.c -- TEST INFRASTRUCTURE: brute-force nearby-triangle lists over a scene, the specification of rt_nearby_offsets /
 * rt_list_nearby (include/rt_hip.h rule 9).  It includes tests/point_oracle.c unchanged (and through it
 * oracle/rt_oracle.c) for the scene, the per-instance map and the fp32 sequence of rt_closest_points' rules 1-3.  For each point every
 * (instance, triangle) is visited, the candidates under rule 4 are sorted by (d2, instance, triangle) and written into the rooms.
 * Built by tests/nearby_oracle.py with the oracle's own flags (-ffp-contract=off). */
#include "point_oracle.c"

typedef struct { float d2, b1, b2; int32_t inst, tri; } nb_pair;

static int nb_cmp(const void *pa, const void *pb)
{
    const nb_pair *a = (const nb_pair *)pa, *b = (const nb_pair *)pb;
    if (a->d2 != b->d2) return a->d2 < b->d2 ? -1 : 1;
    if (a->inst != b->inst) return a->inst < b->inst ? -1 : 1;
    return a->tri < b->tri ? -1 : (a->tri > b->tri ? 1 : 0);
}

/* every pair of one point, sorted when `sort`; returns the count (*out malloc'd, the caller frees; NULL out: count only) */
static int nb_point(const OrcScene *sc, f3 p, float bound, int sort, nb_pair **out)
{
    int i, k, n = 0, cap = 16;
    nb_pair *h = out ? (nb_pair *)malloc(sizeof(nb_pair) * cap) : NULL;
    for (i = 0; i < sc->ninst; i++) {
        const instance_t *in = &sc->instances[i];
        const OrcMesh *m = sc->meshes[in->mesh_index];
        f3 q = apply_lre(in->pose, p);
        for (k = 0; k < m->ntris; k++) {
            f3 a, ab, ac;
            float b1, b2, d2;
            pt_tri(&m->tris[k], in->scale, &a, &ab, &ac);
            pt_weights(q, a, ab, ac, &b1, &b2);
            d2 = pt_len2(pt_sub(q, pt_at(a, ab, ac, b1, b2)));
            if (isnan(d2) || !(sqrtf(d2) <= bound)) continue;
            if (h) {
                if (n == cap) { cap *= 2; h = (nb_pair *)realloc(h, sizeof(nb_pair) * cap); }
                h[n].d2 = d2; h[n].b1 = b1; h[n].b2 = b2; h[n].inst = i; h[n].tri = k;
            }
            n++;
        }
    }
    if (h && sort) qsort(h, (size_t)n, sizeof(nb_pair), nb_cmp);
    if (out) *out = h;
    return n;
}

/* n points pts [n][3], maxd [n] (NULL = +inf) -> count [n], the number of pairs of each point */
void orcn_count_nearby(const OrcScene *sc, int64_t n, const float *pts, const float *maxd, int32_t *count)
{
    int64_t j;
    for (j = 0; j < n; j++)
        count[j] = nb_point(sc, mk3(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]), maxd ? maxd[j] : INFINITY, 0, NULL);
}

/* rooms: offsets [n + 1] (CSR) or, with offsets NULL, max_hits per point.  Writes the first min(count, room) pairs of each point into
 * its room with orcx_closest_points' fields for each triangle, and pads the rest; nothing outside the rooms.  count [n] = the full
 * count. */
void orcn_list_nearby(const OrcScene *sc, int64_t n, const float *pts, const float *maxd, const int64_t *offsets, int32_t max_hits,
                      float *dist, int32_t *inst, int32_t *tri, float *point, float *normal, float *bary, float *uv, int32_t *count)
{
    int64_t j, s;
    for (j = 0; j < n; j++) {
        f3 p = mk3(pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]);
        nb_pair *h;
        int c = nb_point(sc, p, maxd ? maxd[j] : INFINITY, 1, &h);
        int64_t start = offsets ? offsets[j] : j * (int64_t)max_hits;
        int64_t room = offsets ? (offsets[j + 1] > offsets[j] ? offsets[j + 1] - offsets[j] : 0) : max_hits;
        count[j] = c;
        for (s = 0; s < room; s++) {
            int64_t q = start + s;
            if (s < c) {
                const instance_t *in = &sc->instances[h[s].inst];
                const tri_t *t = &sc->meshes[in->mesh_index]->tris[h[s].tri];
                float b1 = h[s].b1, b2 = h[s].b2, u0 = (1.0f - b2) - b1;
                f3 a, ab, ac, w, nn;
                pt_tri(t, in->scale, &a, &ab, &ac);
                w = apply_lre(in->inv_pose, pt_at(a, ab, ac, b1, b2));         /* raycast.cu:98-102's map */
                nn = apply_euler(in->inv_rotation, t->normal);                    /* raycast.cu:115-122 */
                nn.x *= in->scale.x; nn.y *= in->scale.y; nn.z *= in->scale.z;
                nn = normalize3(nn);
                dist[q] = sqrtf(h[s].d2); inst[q] = h[s].inst; tri[q] = h[s].tri;
                point[3 * q] = w.x; point[3 * q + 1] = w.y; point[3 * q + 2] = w.z;
                normal[3 * q] = nn.x; normal[3 * q + 1] = nn.y; normal[3 * q + 2] = nn.z;
                bary[2 * q] = b1; bary[2 * q + 1] = b2;
                uv[2 * q] = (u0 * t->uv[0].x + b1 * t->uv[1].x) + b2 * t->uv[2].x;
                uv[2 * q + 1] = (u0 * t->uv[0].y + b1 * t->uv[1].y) + b2 * t->uv[2].y;
            } else {
                dist[q] = FLT_MAX; inst[q] = -1; tri[q] = -1;
                point[3 * q] = point[3 * q + 1] = point[3 * q + 2] = 0.0f;
                normal[3 * q] = normal[3 * q + 1] = normal[3 * q + 2] = 0.0f;
                bary[2 * q] = bary[2 * q + 1] = 0.0f; uv[2 * q] = uv[2 * q + 1] = 0.0f;
            }
        }
        free(h);
    }
}
