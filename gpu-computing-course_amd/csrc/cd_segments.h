// cd_segments.h -- segment queries against the mesh: every triangle within a radius of a segment (a capsule), and the nearest.  Not
// reference behaviour.
//   An item is (a, b, r): the segment a + s (b - a), s in [0, 1], and a radius; a == b is a point.  The per-pair predicate is seg_tri
//   (cd_math.h): a row / an answer is a triangle with seg_tri's dist <= r, CLOSED.
//   k_segments_descend / k_segments_exact : the all-results pattern of cd_within.h as it stands -- within_walk with SegFilter at the
//       item's own bound r, leaf hits through prox_walk's queue to the workgroup's shard, then seg_tri at full lanes over the shards
//       (ShardSlice), rows appended with one atomic per workgroup and round (pair_append); nothing is written at or past cap rows.
//       n == 1 has no records: every item is a candidate against leaf 0.
//   k_segments_closest<ANY> : k_closest_points' lane.  SEED: from the root the greedy descent on pt_box2 of the segment's MIDPOINT, ties
//       to the left, down to a leaf, whose triangle gives the first bound best = min(r, dist) -- any leaf is a correct seed, the
//       midpoint's is a near one.  WALK: the stackless pre-order walk from the root, a box entered when it meets the segment at
//       bound = best, CLOSED, so that a triangle at the same distance with a smaller ID is still seen; seg_tri runs INLINE and best
//       shrinks with every better candidate.  Of the triangles with dist <= r the smallest (dist, ID, face index) wins.  ANY: the lane
//       stops at the first triangle within r.  n == 1: the lane tests leaf 0 and is done.
//   The filter only filters.  SegFilter::meets is ray_box(h0, h1, a, d, pad + bound, 1.0): the slab test over s in [0, 1] against the
//       stored fp32 box read as [lo, prox_hi(hi)] and inflated by pad + bound on every axis, pad = 2^-20 max(M, |a|_inf, |b|_inf), M the
//       largest |coordinate| of the root box.  The proof:
//       (i)   dist > 0 rows.  Let x on the segment and y on the triangle be the true closest pair, |x - y| = D.  y lies in the leaf's
//             box and in every box on its root path; |x_a - y_a| <= D on every axis, so x lies in the box inflated by D on every axis,
//             and x = a + s d for an s in [0, 1]: the exact slab test at inflation D passes.  seg_tri's dist is below D by at most a
//             few 2^-52 M' (M' = max(M, |a|_inf, |b|_inf)) = 2^-30 pad, and a row has dist <= bound, so D <= bound + 2^-30 pad.
//       (ii)  cross = 1 rows (dist = 0).  ray_tri's gate: the computed P = a + t d lies within G <= 2^-10 pad of the triangle's box on
//             every axis, t in [0, 1] (cd_rays.h's case with tfar = 1).
//       (iii) rounding.  The quotients (bound - a_k) / d_k are IEEE divisions of one rounded difference, off by a relative 2^-52 of
//             values no larger than M' + pad + bound; where bound is finite and far above M' the box is inflated far beyond the mesh
//             and the slab interval contains [0, 1] with room.  The pad covers (i)'s 2^-30, (ii)'s 2^-10 and this with cd_points.h's
//             margin.
//       bound = +inf: every slab is [-inf, +inf], the quotients are -inf / +inf (never inf - inf: the coordinates are finite), tn stays
//       0 and tf stays 1: nothing is culled.  A zero d component tests a_k against the inflated interval and divides nothing; an
//       all-zero d is the padded containment test of the point a, the closed ball's box test.  No NaN arises for finite input, and
//       ray_box's comparisons are written so that a NaN would widen, never cull.
//   k_seg_tri_points : seg_tri on explicit operands, the pin of the device function (cd_seg_tri_points).
#pragma once
#include "cd_within.h"

namespace cd {

constexpr int SEGMENT_THREADS = 64;
constexpr uint32_t SEGMENT_NONE = 0xffffffffu;

struct SegFilter {
    d3 a, d; double pad, bound;
    __device__ __forceinline__ bool meets(const RecCursor &w) const { return ray_box(w.h0, w.h1, a, d, pad + bound, 1.0); }
};
// an item's filter at its own radius
__device__ __forceinline__ SegFilter seg_filter(const double *__restrict__ r, const double *__restrict__ root_box)
{
    SegFilter q;
    const d3 b = d3{r[3], r[4], r[5]};
    q.a = d3{r[0], r[1], r[2]}; q.d = sub(b, q.a); q.bound = r[6];
    q.pad = dmax_abs3(dmax_abs3(root_max_abs(root_box), q.a), b) * PROX_SLACK;
    return q;
}

__global__ __launch_bounds__(PROX_DESC_THREADS) void k_segments_descend(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name,
                                                                        const double *__restrict__ root_box, int n, const uint32_t *__restrict__ sort_flags /* 9 words */,
                                                                        const double *__restrict__ segs, unsigned long long ns, ProxState *__restrict__ st,
                                                                        uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * PROX_DESC_THREADS + threadIdx.x;
    const bool active = i < ns;
    SegFilter q{};
    if (active) q = seg_filter(segs + 7 * i, root_box);
    within_walk(recs, root_name, n, (uint32_t)i, active, q, st, cand, shard_cap);
}

// the values of one seg_tri evaluation into row / item `at` of the arrays (each may be NULL)
struct SegOut {
    uint32_t *ids; double *dist, *s, *on_seg, *on_tri, *uv; uint8_t *feature, *end, *cross, *side;
    __device__ __forceinline__ void put(unsigned long long at, uint32_t id, const SegTri &r) const
    {
        if (ids) ids[at] = id;
        if (dist) dist[at] = r.dist;
        if (s) s[at] = r.s;
        if (on_seg) { on_seg[3 * at] = r.qs.x; on_seg[3 * at + 1] = r.qs.y; on_seg[3 * at + 2] = r.qs.z; }
        if (on_tri) { on_tri[3 * at] = r.qt.x; on_tri[3 * at + 1] = r.qt.y; on_tri[3 * at + 2] = r.qt.z; }
        if (uv) { uv[2 * at] = r.u; uv[2 * at + 1] = r.v; }
        if (feature) feature[at] = (uint8_t)r.feature;
        if (end) end[at] = (uint8_t)r.end;
        if (cross) cross[at] = (uint8_t)r.cross;
        if (side) side[at] = (uint8_t)r.side;
    }
};

// rows[2 at] = the item, rows[2 at + 1] = the face index; o: the triangle's ID and seg_tri's values
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_segments_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                      const uint32_t *__restrict__ perm, const double *__restrict__ verts, const double *__restrict__ segs,
                                                                      ProxState *__restrict__ st, unsigned long long cap, uint32_t *__restrict__ rows, const SegOut o)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long tested = 0;
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        bool hit = false;
        uint2 c = make_uint2(0u, 0u);
        uint32_t id = 0;
        SegTri r{};
        if (i < sl.total) {
            c = sl.list[i];
            const LeafTri lt = leaf[c.y];
            const double *p = segs + 7 * (size_t)c.x;
            ++tested;
            r = seg_tri(d3{p[0], p[1], p[2]}, d3{p[3], p[4], p[5]}, load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            hit = r.dist <= p[6];
            id = lt.id;
        }
        pair_append(hit, &st->n_pairs, cap, [&](unsigned long long at) {
            rows[2 * at] = c.x; rows[2 * at + 1] = perm[c.y];
            o.put(at, id, r);
        });
    }
    group_counters_add<1>(&tested, &st->n_tested);
}

template <bool ANY>
__global__ __launch_bounds__(SEGMENT_THREADS) void k_segments_closest(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, const LeafTri *__restrict__ leaf,
                                                                      const uint32_t *__restrict__ perm, const double *__restrict__ verts, const double *__restrict__ root_box, int n,
                                                                      const double *__restrict__ segs, unsigned long long ns, PointState *__restrict__ st,
                                                                      uint32_t *__restrict__ face, const SegOut o)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * SEGMENT_THREADS + threadIdx.x;
    bool active = i < ns;
    SegFilter q{};
    d3 b{0.0, 0.0, 0.0}, mid{0.0, 0.0, 0.0};
    double rmax = 0.0;
    if (active) {
        const double *r = segs + 7 * i;
        q = seg_filter(r, root_box);
        b = d3{r[3], r[4], r[5]}; rmax = r[6];
        mid = d3{q.a.x + 0.5 * q.d.x, q.a.y + 0.5 * q.d.y, q.a.z + 0.5 * q.d.z};
    }
    uint32_t bface = SEGMENT_NONE, bid = 0u;                             // q.bound: min(r, the best candidate's dist)
    SegTri best{};
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
            if (seeding) {                                               // the child of `cur` nearer to the midpoint, ties to the left
                RecCursor l, r;
                l.at_left(recs, n, cur); r.at_right(recs, n, cur);
                visits += 2;
                if (pt_box2(r.h0, r.h1, mid, q.pad) < pt_box2(l.h0, l.h1, mid, q.pad)) l = r;
                if (l.internal(n)) {
                    cur = (uint32_t)l.link();
                    if (!seed.count(n)) break;                           // (the descent's own moves, up to n - 1, under the walk's rule)
                    continue;
                }
                if (l.leaf(n)) { test = true; k = l.leaf_index(); }
            } else {
                ++visits;
                const bool enter = q.meets(w);                           // CLOSED
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
            const SegTri r = seg_tri(q.a, b, load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            if (r.dist <= rmax) {
                const uint32_t f = perm[k];
                if (ANY) { bface = f; break; }
                // the smallest (dist, ID, face index)
                if (bface == SEGMENT_NONE || r.dist < best.dist || (r.dist == best.dist && (lt.id < bid || (lt.id == bid && f < bface)))) {
                    bface = f; bid = lt.id; best = r; q.bound = r.dist;
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
    if (i < ns) {
        const bool found = bface != SEGMENT_NONE;
        face[i] = bface;
        if (!ANY) {
            if (!found) { best = SegTri{}; best.dist = __builtin_inf(); }
            o.put(i, found ? bid : 0u, best);
        }
    }
    item_counters_add(i < ns && bface != SEGMENT_NONE, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);
}

// cd_seg_tri_points: seg_tri on explicit operands, n x 6 doubles (a, b) and n x 9 (p0, p1, p2)
__global__ __launch_bounds__(256) void k_seg_tri_points(const double *__restrict__ segs, const double *__restrict__ tri, unsigned long long n, const SegOut o)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double *q = segs + 6 * i, *p = tri + 9 * i;
        o.put(i, 0u, seg_tri(d3{q[0], q[1], q[2]}, d3{q[3], q[4], q[5]}, d3{p[0], p[1], p[2]}, d3{p[3], p[4], p[5]}, d3{p[6], p[7], p[8]}));
    }
}

}  // namespace cd
