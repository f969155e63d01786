// cd_points.h -- closest-point queries against the mesh: nearest triangle and within-radius.  Not reference behaviour.
//   k_closest_points<ANY> : one lane per query point, in the order given (neighbouring points share a wave: coherent points should be
//       neighbours).  A point with no radius meets every box, so a pre-order walk alone would test everything before the first near
//       leaf in Morton order; the lane therefore works in two phases, both in the one loop below (ONE inline site of pt_tri):
//       SEED   from the root, a greedy descent: a cursor at each child of the node (both halves of its record), on to the child
//              whose box is nearer to the point, ties to the left, down to a leaf, whose triangle gives the first candidate and the
//              first bound  best = min(rmax, dist).
//       WALK   the queries' stackless pre-order walk from the ROOT (RecCursor, cd_bvh.h: the walk, its step bound and its guards are
//              described there): a subtree is entered when its box's lower-bound distance does not exceed `best`, CLOSED, so that a
//              triangle at the same distance with a smaller ID is still seen; `best` shrinks with every better candidate.  The seed
//              leaf may be tested a second time: no bookkeeping avoids it.
//       At a leaf the exact FP64 predicate pt_tri (cd_math.h) runs INLINE, for the reason k_cast_rays gives: the bound shrinks with
//       every candidate, so a queue would carry boxes the next candidate makes pointless.  Of the triangles with dist <= rmax the
//       smallest (dist, triangle ID, face index) wins.  ANY: the lane stops at the first triangle within rmax, often the seed.
//       n == 1 has no records: the lane tests leaf 0 and is done.
//   The filter only filters.  The box distance is FP64 on the stored fp32 bounds read as [lo, prox_hi(hi)] (converted exactly), per
//       axis the gap  g_a = max((lo_a - pad) - p_a, (p_a - hi_a) - pad, 0)  with pad = 2^-20 max(M, |p|_inf), M the largest
//       |coordinate| of the root box; a subtree is skipped only when  (g_x^2 + g_y^2) + g_z^2 > best^2.  The padded gap vector is no
//       longer than the true distance to the box minus pad (each positive component shrinks by pad), pt_tri's dist is below the true
//       distance to the triangle by at most a few 2^-52 (M + |p|_inf) = 2^-30 pad, and the roundings of the gaps and squares are
//       relative 2^-52: the pad covers all of it with a margin of about 2^30 (the proof: DESIGN.md section 14).  The comparison is
//       written so that a NaN enters, never culls; an overflowing best^2 (a huge finite rmax) is +inf and culls nothing.
//   k_pt_tri_points : pt_tri on explicit operands, the pin of the device function (cd_pt_tri_points).
#pragma once
#include "cd_rays.h"

namespace cd {

constexpr int POINT_THREADS = 64;
constexpr uint32_t POINT_NONE = 0xffffffffu;
struct alignas(64) PointState { unsigned long long n_found, node_visits, tri_tests, pad[5]; };

// the squared lower-bound distance from p to the padded box  (h0, h1: a record half, lo = h0.xyz, hi = (h0.w, h1.x, h1.y))
__device__ __forceinline__ double pt_box2(const float4 h0, const float4 h1, const d3 p, const double pad)
{
#define CD_PT_AXIS(LO, HI, P) fmax2(fmax2(((double)(LO) - pad) - (P), ((P) - (double)prox_hi(HI)) - pad), 0.0)
    const double gx = CD_PT_AXIS(h0.x, h0.w, p.x), gy = CD_PT_AXIS(h0.y, h1.x, p.y), gz = CD_PT_AXIS(h0.z, h1.y, p.z);
#undef CD_PT_AXIS
    return (gx * gx + gy * gy) + gz * gz;
}

template <bool ANY>
__global__ __launch_bounds__(POINT_THREADS) void k_closest_points(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, const LeafTri *__restrict__ leaf,
                                                                  const uint32_t *__restrict__ perm, const double *__restrict__ verts, const double *__restrict__ root_box, int n,
                                                                  const double *__restrict__ points, unsigned long long np, PointState *__restrict__ st,
                                                                  uint32_t *__restrict__ face, uint32_t *__restrict__ ids, double *__restrict__ dist,
                                                                  double *__restrict__ closest, double *__restrict__ uv, uint8_t *__restrict__ feature, uint8_t *__restrict__ side)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * POINT_THREADS + threadIdx.x;
    bool active = i < np;
    d3 p{0.0, 0.0, 0.0};
    double rmax = 0.0, pad = 0.0;
    if (active) {
        const double *r = points + 4 * i;
        p = d3{r[0], r[1], r[2]}; rmax = r[3];
        pad = dmax_abs3(root_max_abs(root_box), p) * PROX_SLACK;
    }
    double best = rmax, best2 = rmax * rmax;                             // the bound: min(rmax, the best candidate's dist), and its square
    uint32_t bface = POINT_NONE, bid = 0u, bfeat = 0u, bside = 0u;
    double bu = 0.0, bv = 0.0;
    d3 bq{0.0, 0.0, 0.0};
    uint32_t visits = 0, tests = 0;
    RecCursor w{}, seed{};                                               // the WALK's cursor; of `seed` only the step count is used (SEED's moves)
    uint32_t root = 0, cur = 0;
    bool seeding = true;
    const bool leaf_only = n == 1;                                       // no records: leaf 0 is the whole tree
    if (active && !leaf_only) {
        root = (uint32_t)*root_name;
        cur = root;
        active = rec_internal((int32_t)root, n);                         // (no tree: nothing is read; nothing is found)
    }
    while (active) {
        bool test = leaf_only;
        uint32_t k = 0;
        if (!leaf_only) {
            if (seeding) {                                               // the nearer child of `cur`, ties to the left
                RecCursor l, r;
                l.at_left(recs, n, cur); r.at_right(recs, n, cur);
                visits += 2;
                if (pt_box2(r.h0, r.h1, p, pad) < pt_box2(l.h0, l.h1, p, pad)) l = r;
                if (l.internal(n)) {
                    cur = (uint32_t)l.link();
                    if (!seed.count(n)) break;                           // (the descent's own moves, up to n - 1, under the walk's rule)
                    continue;
                }
                if (l.leaf(n)) { test = true; k = l.leaf_index(); }
            } else {
                ++visits;
                const bool enter = !(pt_box2(w.h0, w.h1, p, pad) > best2);   // CLOSED; a NaN enters
                if (enter && w.internal(n)) {
                    if (!w.descend(recs, n)) break;
                    continue;
                }
                if (enter && w.leaf(n)) { test = true; k = w.leaf_index(); }
            }
        }
        if (test) {
            ++tests;
            const LeafTri lt = leaf[k];
            const PtTri r = pt_tri(p, load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            if (r.dist <= rmax) {
                const uint32_t f = perm[k];
                if (ANY) { bface = f; break; }
                // the smallest (dist, ID, face index)
                if (bface == POINT_NONE || r.dist < best || (r.dist == best && (lt.id < bid || (lt.id == bid && f < bface)))) {
                    bface = f; bid = lt.id; best = r.dist; best2 = r.dist * r.dist;
                    bu = r.u; bv = r.v; bq = r.q; bfeat = r.feature; bside = r.side;
                }
            }
        }
        if (leaf_only) break;
        if (seeding) {                                                   // the walk starts at the root, with 2 n moves of its own
            seeding = false;
            w.start_root(recs, n, root);                                 // (true: the root was checked before the loop)
            continue;
        }
        if (!w.next(recs, n)) break;
    }
    if (i < np) {
        const bool found = bface != POINT_NONE;
        face[i] = bface;
        if (!ANY) {
            if (ids) ids[i] = found ? bid : 0u;
            if (dist) dist[i] = found ? best : __builtin_inf();
            if (closest) { closest[3 * i] = found ? bq.x : 0.0; closest[3 * i + 1] = found ? bq.y : 0.0; closest[3 * i + 2] = found ? bq.z : 0.0; }
            if (uv) { uv[2 * i] = found ? bu : 0.0; uv[2 * i + 1] = found ? bv : 0.0; }
            if (feature) feature[i] = (uint8_t)(found ? bfeat : 0u);
            if (side) side[i] = (uint8_t)(found ? bside : 0u);
        }
    }
    item_counters_add(i < np && bface != POINT_NONE, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);
}

// cd_pt_tri_points: pt_tri on explicit operands, n x 3 doubles (p) and n x 9 (p0, p1, p2)
__global__ __launch_bounds__(256) void k_pt_tri_points(const double *__restrict__ pts, const double *__restrict__ tri, unsigned long long n, double *__restrict__ dist,
                                                       double *__restrict__ closest, double *__restrict__ uv, uint8_t *__restrict__ feature, uint8_t *__restrict__ side)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double *q = pts + 3 * i, *p = tri + 9 * i;
        const PtTri r = pt_tri(d3{q[0], q[1], q[2]}, d3{p[0], p[1], p[2]}, d3{p[3], p[4], p[5]}, d3{p[6], p[7], p[8]});
        dist[i] = r.dist;
        if (closest) { closest[3 * i] = r.q.x; closest[3 * i + 1] = r.q.y; closest[3 * i + 2] = r.q.z; }
        if (uv) { uv[2 * i] = r.u; uv[2 * i + 1] = r.v; }
        if (feature) feature[i] = (uint8_t)r.feature;
        if (side) side[i] = (uint8_t)r.side;
    }
}

}  // namespace cd
