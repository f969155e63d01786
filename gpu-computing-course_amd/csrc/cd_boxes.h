// cd_boxes.h -- box queries: every triangle that meets an axis-aligned box, as rows and as counts.  Not reference behaviour
// (DESIGN.md section 23).
//   A box is six doubles {x1, x2, y1, y2, z1, z2}, CLOSED; the per-pair predicate is box_tri (cd_math.h).
//   k_boxes_descend / k_boxes_exact : cd_boxes_overlap_all, built as cd_within.h builds its calls.  The bound is the item's own box and
//       never shrinks, so the descent is within_walk with RegionFilter (one lane per box, in the order given, one wave per workgroup;
//       n == 1: every box is a candidate against leaf 0) and the exact stage is the ShardSlice / pair_append scaffold with box_tri:
//       a row for every hit, nothing written at or past cap rows, every candidate one evaluation (n_tested).
//   k_boxes_count<ANY> : cd_boxes_count, the inline walk of cd_inside.h: one lane per box walks the records from the ROOT in pre-order
//       and runs box_tri INLINE at a leaf, adding to two registers (count, n_inside).  Integer sums: the result does not depend on the
//       order of the walk.  No candidate buffer, no atomics on results, nothing that can overflow.  ANY: the lane stops at its first
//       hit.  n == 1 has no records: the lane tests leaf 0 and is done.
//   The filter only filters (cd_inside.h's argument).  A node box is the stored fp32 bounds read as [lo, prox_hi(hi)], converted
//       exactly to double; the query box is taken as given, with no pad.  A subtree is skipped only when  node_lo_a > hi_a  or
//       node_hi_a < lo_a  on some axis (CLOSED; written so that a NaN enters).  box_tri's gate is exact comparisons of the inputs, so a
//       face that hits has, on every axis, a vertex >= lo_a and a vertex <= hi_a: its FP64 box meets the query box.  Every stored box
//       of an ancestor contains that FP64 box (lo rounded down, prox_hi(hi) an upper bound), so neither comparison above holds there:
//       every face that hits is reached, and box_tri alone decides.  Which other faces are tested changes the counters only.
//   CONTAINED SUBTREES ARE NOT WALKED (k_boxes_count).  The records are walked in pre-order over contiguous leaf ranges: the lane keeps
//       `pos`, the first leaf position it has not yet passed (0 at the start, end + 1 after every subtree it finishes or skips,
//       unchanged by a descent), so the subtree at the cursor covers the leaves [pos, end].  When the node's box [lo, prox_hi(hi)]
//       lies inside the query box on all three axes (exact comparisons; a NaN means not contained), every vertex of every triangle of
//       the subtree lies in the node's box, so in the closed query box: box_tri takes rule 2 for each of them -- hit, inside = 1 --
//       and that is decided by comparisons alone, which is why rule 2 comes before any arithmetic.  The lane adds end - pos + 1 to
//       both sums and moves on with next(); with ANY it stops there.
//       The root has no record of its own (the walk starts at its children); its box is the tree's FP64 root box (boxes[0 .. 5],
//       cd_root_box).  The lane tests it first, by the same argument with the exact box: a query box that contains the whole mesh
//       counts n leaves with one box tested and no box_tri at all.
//   k_box_tri_points : box_tri on explicit operands, the pin of the device function (cd_box_tri_points).
#pragma once
#include "cd_within.h"

namespace cd {

constexpr int BOXES_THREADS = 64;

// prox_walk's filter and the count walk's two tests: the query box as given against a record half (lo = h0.xyz, hi = (h0.w, h1.x, h1.y))
struct RegionFilter {
    Box b;
    __device__ __forceinline__ bool meets(const RecCursor &w) const
    {
        return !((double)w.h0.x > b.x2 || (double)prox_hi(w.h0.w) < b.x1 || (double)w.h0.y > b.y2 || (double)prox_hi(w.h1.x) < b.y1 ||
                 (double)w.h0.z > b.z2 || (double)prox_hi(w.h1.y) < b.z1);       // CLOSED; a NaN enters
    }
    __device__ __forceinline__ bool contains(const RecCursor &w) const
    {
        return (double)w.h0.x >= b.x1 && (double)prox_hi(w.h0.w) <= b.x2 && (double)w.h0.y >= b.y1 && (double)prox_hi(w.h1.x) <= b.y2 &&
               (double)w.h0.z >= b.z1 && (double)prox_hi(w.h1.y) <= b.z2;        // a NaN: not contained
    }
    __device__ __forceinline__ bool contains(const double *__restrict__ r /* an FP64 box */) const
    {
        return r[0] >= b.x1 && r[1] <= b.x2 && r[2] >= b.y1 && r[3] <= b.y2 && r[4] >= b.z1 && r[5] <= b.z2;
    }
};
__device__ __forceinline__ Box load_query_box(const double *__restrict__ boxes, unsigned long long i)
{
    const double *r = boxes + 6 * (size_t)i;
    return Box{r[0], r[1], r[2], r[3], r[4], r[5]};
}

__global__ __launch_bounds__(PROX_DESC_THREADS) void k_boxes_descend(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, int n,
                                                                     const uint32_t *__restrict__ sort_flags /* 9 words */, const double *__restrict__ boxes,
                                                                     unsigned long long nb, ProxState *__restrict__ st, uint2 *__restrict__ cand,
                                                                     unsigned long long shard_cap)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * PROX_DESC_THREADS + threadIdx.x;
    const bool active = i < nb;
    RegionFilter q{};
    if (active) q.b = load_query_box(boxes, i);
    within_walk(recs, root_name, n, (uint32_t)i, active, q, st, cand, shard_cap);
}

// rows[2 at] = the item, rows[2 at + 1] = the face index; the other arrays (each may be NULL): the triangle's ID and box_tri's inside
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_boxes_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                   const uint32_t *__restrict__ perm, const double *__restrict__ verts, const double *__restrict__ boxes,
                                                                   ProxState *__restrict__ st, unsigned long long cap, uint32_t *__restrict__ rows,
                                                                   uint32_t *__restrict__ ids, uint8_t *__restrict__ inside)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long tested = 0;
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        uint2 c = make_uint2(0u, 0u);
        uint32_t id = 0;
        BoxTri r{false, false, 0u};
        if (i < sl.total) {
            c = sl.list[i];
            const LeafTri lt = leaf[c.y];
            ++tested;
            r = box_tri(load_query_box(boxes, c.x), load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            id = lt.id;
        }
        pair_append(r.hit, &st->n_pairs, cap, [&](unsigned long long at) {
            rows[2 * at] = c.x; rows[2 * at + 1] = perm[c.y];
            if (ids) ids[at] = id;
            if (inside) inside[at] = r.inside ? 1 : 0;
        });
    }
    group_counters_add<1>(&tested, &st->n_tested);
}

// count[i] / n_inside[i] (may be NULL): the rows item i has in cd_boxes_overlap_all, and those with inside = 1; ANY: count is 0 or 1
template <bool ANY>
__global__ __launch_bounds__(BOXES_THREADS) void k_boxes_count(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, const LeafTri *__restrict__ leaf,
                                                               const double *__restrict__ verts, const double *__restrict__ root_box, int n,
                                                               const uint32_t *__restrict__ sort_flags /* 9 words */, const double *__restrict__ boxes,
                                                               unsigned long long nb, PointState *__restrict__ st, uint32_t *__restrict__ count,
                                                               uint32_t *__restrict__ n_inside)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * BOXES_THREADS + threadIdx.x;
    bool active = i < nb;
    RegionFilter q{};
    if (active) q.b = load_query_box(boxes, i);
    uint32_t cnt = 0, nin = 0, visits = 0, tests = 0, pos = 0;
    RecCursor w{};
    const bool leaf_only = n == 1;                                       // no records: leaf 0 is the whole tree
    if (active && !leaf_only) {
        ++visits;                                                        // the root: its FP64 box, which no record holds
        if (q.contains(root_box)) { cnt = nin = (uint32_t)n; active = false; }
        else active = w.start_root(recs, n, (uint32_t)*root_name);       // (no tree: nothing is read; nothing is counted)
    }
    while (active) {
        bool test = leaf_only;
        uint32_t k = 0;
        if (!leaf_only) {
            ++visits;
            const bool node = w.internal(n) || w.leaf(n);                // (a link that is neither is not entered, not tested and not counted)
            if (node && w.end >= pos && q.contains(w)) {                 // the leaves [pos, end]: all hit, all inside
                const uint32_t m = w.end - pos + 1u;
                cnt += m; nin += m;
                if (ANY) break;
            } else {
                const bool enter = q.meets(w);
                if (enter && w.internal(n)) {
                    if (!w.descend(recs, n)) break;
                    continue;
                }
                if (enter && w.leaf(n)) { test = true; k = w.leaf_index(); }
            }
            pos = w.end + 1u;
        }
        if (test) {
            ++tests;
            const LeafTri lt = leaf[k];
            const BoxTri r = box_tri(q.b, load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            if (r.hit) {
                ++cnt;
                if (r.inside) ++nin;
                if (ANY) break;
            }
        }
        if (leaf_only || !w.next(recs, n)) break;
    }
    if (ANY && cnt) cnt = 1u;
    if (i < nb) {
        count[i] = cnt;
        if (n_inside) n_inside[i] = nin;
    }
    item_counters_add(i < nb && cnt != 0u, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);
}

// cd_box_tri_points: box_tri on explicit operands, n x 6 doubles (the boxes) and n x 9 (p0, p1, p2)
__global__ __launch_bounds__(256) void k_box_tri_points(const double *__restrict__ boxes, const double *__restrict__ tri, unsigned long long n, uint8_t *__restrict__ hit,
                                                        uint8_t *__restrict__ inside, uint8_t *__restrict__ code)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double *p = tri + 9 * i;
        const BoxTri r = box_tri(load_query_box(boxes, i), d3{p[0], p[1], p[2]}, d3{p[3], p[4], p[5]}, d3{p[6], p[7], p[8]});
        hit[i] = r.hit ? 1 : 0;
        if (inside) inside[i] = r.inside ? 1 : 0;
        if (code) code[i] = (uint8_t)r.code;
    }
}

}  // namespace cd
