// cd_planes.h -- plane queries: the faces a plane cuts, with the segment of each, and how many faces lie on each side.  Not reference
// behaviour.
//   A plane is four doubles {nx, ny, nz, d}: the points with n . x = d; the per-pair predicate is plane_tri (cd_math.h).
//   ONE ITEM, MANY LANES.  A plane meets much of the mesh by its nature, and the typical call has few planes: the one-lane-an-item
//       walks of cd_within.h and cd_boxes.h would leave the device idle.  A work item here is (plane k, slab j); slab j is the leaf
//       positions [j L, min((j + 1) L, n) - 1], L = CD_PLANE_SLAB, S = ceil(n / L) slabs a plane.  Work item k S + j is lane k S + j:
//       a wave holds neighbouring slabs of one plane (neighbouring parts of the tree, walks of similar length), or several planes of
//       a small mesh.  One wave per workgroup, as in the other descents.
//   A SLAB NEEDS NO NEW TREE DATA.  The records are walked in pre-order over contiguous leaf ranges (cd_bvh.h), and
//       RecCursor::start_behind(a - 1) starts a walk at exactly the leaves (a - 1, n - 1].  The lane of slab [a, b] starts at the
//       root for a = 0 and behind a - 1 otherwise, keeps `pos`, the first leaf position it has not yet passed (a at the start,
//       end + 1 after every subtree it finishes or skips, unchanged by a descent: k_boxes_count's), and stops once pos > b -- or by
//       the cursor's step rule.  The subtree at the cursor covers the leaves [pos, end]; it may reach past b, and then only its
//       leaves up to b are this lane's: a leaf is tested, queued or counted by the one lane whose slab holds its position, so the
//       slabs' results are disjoint and their union is the plane's.  n == 1 has no records: the lane takes leaf 0.
//   THE FILTER IS EXACT AND NEEDS NO PAD (PlaneFilter).  For a node box [lo, prox_hi(hi)], widened exactly to double, plane_side is
//       evaluated at two corners: per axis the bound that minimises n_a x_a (lo_a for n_a >= 0, else hi_a), and the one that maximises
//       it.  A rounded product with a constant of fixed sign, a rounded sum and the rounded subtraction of d are all monotone, and
//       every vertex of the subtree lies in the box (cd_boxes.h's argument), so s_min <= s_i <= s_max as computed, for every vertex.
//       s_min >= 0: no vertex is below, every face is ABOVE.  s_max < 0: every face is BELOW.  Both are written so that a NaN
//       decides nothing and the subtree is entered.  Only otherwise is the subtree entered: the filter of the rows call and the
//       counted-without-walking shortcut of the count call are the same test.  The root has no record; its box is the tree's FP64
//       root box, and every lane tests it first: a plane that misses the mesh costs one test a lane.
//   k_planes_count   : cd_planes_count.  The walk above with plane_tri's class INLINE at a leaf.  A subtree on one side adds
//       min(end, b) - pos + 1 to that side's sum.  Three integer sums in registers, added to the plane's three counts with one
//       integer atomic each at the end (the counts are zeroed on the stream first): the order cannot matter.  A wave whose lanes all
//       work on one plane sums first and adds once.  No candidate buffer, nothing that can overflow.
//   k_planes_descend : cd_planes_cut_all's filter walk.  (k, leaf position) of every leaf whose box the plane may cut goes through a
//       wave-shared LDS queue to the workgroup's shard, 64 at a time -- prox_walk's queue and flush (cd_proximity.h), restated in
//       plane_walk because prox_walk's loop has no bound to stop at and is not to be instantiated differently.
//   k_planes_exact   : the ShardSlice / pair_append scaffold with plane_tri, as k_boxes_exact: a row for every CUT face.
//   k_plane_tri_points : plane_tri on explicit operands, the pin of the device function (cd_plane_tri_points).
#pragma once
#include "cd_boxes.h"

namespace cd {

constexpr int PLANES_THREADS = 64;
constexpr uint32_t PLANE_SLAB = CD_PLANE_SLAB;
static_assert(PLANE_SLAB >= 1u && (PLANE_SLAB & (PLANE_SLAB - 1u)) == 0u, "CD_PLANE_SLAB is a power of two");

// on which side of the plane does a box lie: PLANE_ABOVE (no point of it below), PLANE_BELOW (every point below), else PLANE_CUT
struct PlaneFilter {
    Plane p;
    __device__ __forceinline__ uint32_t side(double x1, double x2, double y1, double y2, double z1, double z2) const
    {
        const bool px = p.nx >= 0.0, py = p.ny >= 0.0, pz = p.nz >= 0.0;
        const double s_min = plane_side(p, px ? x1 : x2, py ? y1 : y2, pz ? z1 : z2);
        const double s_max = plane_side(p, px ? x2 : x1, py ? y2 : y1, pz ? z2 : z1);
        return s_min >= 0.0 ? PLANE_ABOVE : (s_max < 0.0 ? PLANE_BELOW : PLANE_CUT);     // a NaN: PLANE_CUT, the subtree is entered
    }
    __device__ __forceinline__ uint32_t side(const RecCursor &w) const
    {
        return side((double)w.h0.x, (double)prox_hi(w.h0.w), (double)w.h0.y, (double)prox_hi(w.h1.x), (double)w.h0.z, (double)prox_hi(w.h1.y));
    }
    __device__ __forceinline__ uint32_t side(const double *__restrict__ r /* an FP64 box */) const { return side(r[0], r[1], r[2], r[3], r[4], r[5]); }
};
__device__ __forceinline__ Plane load_plane(const double *__restrict__ planes, unsigned long long k)
{
    const double *r = planes + 4 * (size_t)k;
    return Plane{r[0], r[1], r[2], r[3]};
}

// The work item of a lane: plane k and the leaf positions [lo, hi] of its slab (active: the lane has one)
struct PlaneSlab {
    uint32_t k, lo, hi; bool active;
    __device__ __forceinline__ PlaneSlab(unsigned long long np, int n)
    {
        const unsigned long long slabs = ((unsigned long long)n + PLANE_SLAB - 1u) / PLANE_SLAB;
        const unsigned long long i = (unsigned long long)blockIdx.x * PLANES_THREADS + threadIdx.x;
        active = i < np * slabs;
        k = (uint32_t)(i / slabs);
        lo = (uint32_t)(i % slabs) * PLANE_SLAB;
        const unsigned long long e = (unsigned long long)lo + PLANE_SLAB;
        hi = (uint32_t)(e < (unsigned long long)n ? e : (unsigned long long)n) - 1u;
    }
    // the cursor at the slab's first subtree (false: there is no tree, nothing is read)
    __device__ __forceinline__ bool start(RecCursor &w, const NodeRec32 *__restrict__ recs, int n, uint32_t root) const
    {
        if (lo == 0u) return w.start_root(recs, n, root);
        w.start_behind(recs, n, lo - 1u);                                // (lo <= n - 1: lo - 1 is a split)
        return true;
    }
};

__device__ __forceinline__ void plane_counts_add(uint32_t *__restrict__ c, uint32_t v) { if (c && v) atomicAdd(c, v); }

// n_cut[k], n_below[k], n_above[k] (the last two may be NULL), zeroed before the launch: the rows plane k has in cd_planes_cut_all,
// the faces wholly below it, the faces with no vertex below it
__global__ __launch_bounds__(PLANES_THREADS) void k_planes_count(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, const LeafTri *__restrict__ leaf,
                                                                 const double *__restrict__ verts, const double *__restrict__ root_box, int n,
                                                                 const uint32_t *__restrict__ sort_flags /* 9 words */, const double *__restrict__ planes,
                                                                 unsigned long long np, PointState *__restrict__ st, uint32_t *__restrict__ n_cut,
                                                                 uint32_t *__restrict__ n_below, uint32_t *__restrict__ n_above)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const PlaneSlab sl(np, n);
    bool active = sl.active;
    PlaneFilter q{};
    if (active) q.p = load_plane(planes, sl.k);
    uint32_t above = 0, below = 0, cut = 0, visits = 0, tests = 0, pos = sl.lo;
    auto add = [&](uint32_t cls, uint32_t m) { above += cls == PLANE_ABOVE ? m : 0u; below += cls == PLANE_BELOW ? m : 0u; cut += cls == PLANE_CUT ? m : 0u; };
    RecCursor w{};
    const bool leaf_only = n == 1;                                       // no records: leaf 0 is the whole tree
    if (active && !leaf_only) {
        ++visits;                                                        // the root: its FP64 box, which no record holds
        const uint32_t side = q.side(root_box);
        if (side != PLANE_CUT) { add(side, sl.hi - sl.lo + 1u); active = false; }   // (the slab's own length: every slab sees the root)
        else active = sl.start(w, recs, n, (uint32_t)*root_name);        // (no tree: nothing is read; nothing is counted)
    }
    while (active) {
        bool test = leaf_only;
        uint32_t k = 0;
        if (!leaf_only) {
            ++visits;
            const bool node = (w.internal(n) || w.leaf(n)) && w.end >= pos;   // (a link that is neither is not entered, not tested and not counted)
            if (node) {
                const uint32_t side = q.side(w);
                if (side != PLANE_CUT) add(side, (w.end < sl.hi ? w.end : sl.hi) - pos + 1u);     // the leaves [pos, min(end, hi)]: all on one side
                else if (w.internal(n)) {
                    if (!w.descend(recs, n)) break;
                    continue;
                } else { test = true; k = w.leaf_index(); }
            }
            pos = w.end + 1u;
        }
        if (test) {
            ++tests;
            const LeafTri lt = leaf[k];
            add(plane_tri(q.p, load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2)).cls, 1u);
        }
        if (leaf_only || pos > sl.hi || !w.next(recs, n)) break;
    }
    // A wave's lanes are neighbouring slabs, on a mesh of more than 64 L faces mostly of ONE plane: then the wave adds its sums,
    // one atomic a count and wave instead of one a lane (DESIGN.md section 24 has what the lanes' own atomics cost).  Lane 0 has
    // a work item whenever any lane has one.
    const uint32_t k0 = __shfl(sl.k, 0);
    if (__all(!sl.active || sl.k == k0)) {
        const uint32_t c = (uint32_t)wave_sum_u64(sl.active ? cut : 0u), b = (uint32_t)wave_sum_u64(sl.active ? below : 0u), a = (uint32_t)wave_sum_u64(sl.active ? above : 0u);
        if (threadIdx.x == 0 && sl.active) {
            plane_counts_add(n_cut + k0, c);
            plane_counts_add(n_below ? n_below + k0 : nullptr, b);
            plane_counts_add(n_above ? n_above + k0 : nullptr, a);
        }
    } else if (sl.active) {
        plane_counts_add(n_cut + sl.k, cut);
        plane_counts_add(n_below ? n_below + sl.k : nullptr, below);
        plane_counts_add(n_above ? n_above + sl.k : nullptr, above);
    }
    item_counters_add(false, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);     // (planes with a row: the host counts them)
}

// The bounded, queued descent of one wave of work items: the walk of the slab [sl.lo, sl.hi] entering every subtree the plane may
// cut, and prox_walk's candidate queue (cd_proximity.h): leaf hits (plane, leaf position) go through a wave-shared LDS queue to the
// workgroup's shard of `cand`, 64 at a time (nothing is written past shard_cap; the shard's counter counts all).  One wave per
// workgroup; every lane of it calls this (a lane with no work item: sl.active = false).
__device__ __forceinline__ void plane_walk(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, const double *__restrict__ root_box, int n,
                                           const PlaneSlab sl, const PlaneFilter q, unsigned long long *__restrict__ shard_ctr, uint2 *__restrict__ cand,
                                           unsigned long long shard_cap)
{
    __shared__ uint2 queue[PROX_QCAP];
    unsigned long long *ctr = &shard_ctr[(blockIdx.x & (NSHARD - 1)) * PROX_SHARD_STRIDE];
    uint2 *shard = cand + (size_t)(blockIdx.x & (NSHARD - 1)) * shard_cap;
    const uint32_t lane = threadIdx.x;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    const bool leaf_only = n == 1;                                       // no records: every plane is a candidate against leaf 0
    bool active = sl.active;
    uint32_t pos = sl.lo;
    RecCursor w{};
    if (active && !leaf_only) active = q.side(root_box) == PLANE_CUT && sl.start(w, recs, n, (uint32_t)*root_name);
    uint32_t qn = 0;                                                     // (wave-uniform)
    while (__ballot(active) != 0ull) {
        bool hit = false; uint32_t k = 0;
        if (active && leaf_only) { hit = true; active = false; }
        else if (active) {
            const bool enter = (w.internal(n) || w.leaf(n)) && w.end >= pos && q.side(w) == PLANE_CUT;
            if (enter && w.internal(n)) active = w.descend(recs, n);
            else {
                if (enter) { hit = true; k = w.leaf_index(); }
                pos = w.end + 1u;
                active = pos <= sl.hi && w.next(recs, n);
            }
        }
        const unsigned long long bal = __ballot(hit);
        if (hit) queue[qn + __popcll(bal & lt_mask)] = make_uint2(sl.k, k);
        qn += (uint32_t)__popcll(bal);
        __syncthreads();
        const bool last = __ballot(active) == 0ull;
        while (qn >= 64u || (qn > 0u && last)) {                         // full batches, and at the end whatever is left
            const uint32_t m = qn < 64u ? qn : 64u;
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(ctr, (unsigned long long)m);
            base = __shfl(base, 0);
            if (lane < m && base + lane < shard_cap) shard[base + lane] = queue[lane];
            uint2 rest = make_uint2(0u, 0u);
            const bool moved = lane + 64u < qn;
            if (moved) rest = queue[lane + 64u];
            __syncthreads();
            if (moved) queue[lane] = rest;
            __syncthreads();
            qn -= m;
        }
    }
}

__global__ __launch_bounds__(PLANES_THREADS) void k_planes_descend(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name,
                                                                   const double *__restrict__ root_box, int n, const uint32_t *__restrict__ sort_flags /* 9 words */,
                                                                   const double *__restrict__ planes, unsigned long long np, ProxState *__restrict__ st,
                                                                   uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const PlaneSlab sl(np, n);
    PlaneFilter q{};
    if (sl.active) q.p = load_plane(planes, sl.k);
    plane_walk(recs, root_name, root_box, n, sl, q, st->shard, cand, shard_cap);
}

// rows[2 at] = the plane, rows[2 at + 1] = the face index; the other arrays (each may be NULL): the triangle's ID and plane_tri's values
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_planes_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                    const uint32_t *__restrict__ perm, const double *__restrict__ verts, const double *__restrict__ planes,
                                                                    ProxState *__restrict__ st, unsigned long long cap, uint32_t *__restrict__ rows,
                                                                    uint32_t *__restrict__ ids, double *__restrict__ seg, uint8_t *__restrict__ edge,
                                                                    double *__restrict__ t, uint8_t *__restrict__ on)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long tested = 0;
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        uint2 c = make_uint2(0u, 0u);
        uint32_t id = 0;
        PlaneTri r{};
        if (i < sl.total) {
            c = sl.list[i];
            const LeafTri lt = leaf[c.y];
            ++tested;
            r = plane_tri(load_plane(planes, c.x), load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            id = lt.id;
        }
        pair_append(i < sl.total && r.cls == PLANE_CUT, &st->n_pairs, cap, [&](unsigned long long at) {
            rows[2 * at] = c.x; rows[2 * at + 1] = perm[c.y];
            if (ids) ids[at] = id;
            if (seg) { double *s = seg + 6 * at; s[0] = r.a.x; s[1] = r.a.y; s[2] = r.a.z; s[3] = r.b.x; s[4] = r.b.y; s[5] = r.b.z; }
            if (edge) { edge[2 * at] = (uint8_t)r.edge_a; edge[2 * at + 1] = (uint8_t)r.edge_b; }
            if (t) { t[2 * at] = r.ta; t[2 * at + 1] = r.tb; }
            if (on) on[at] = (uint8_t)r.on;
        });
    }
    group_counters_add<1>(&tested, &st->n_tested);
}

// cd_plane_tri_points: plane_tri on explicit operands, n x 4 doubles (the planes) and n x 9 (p0, p1, p2)
__global__ __launch_bounds__(256) void k_plane_tri_points(const double *__restrict__ planes, const double *__restrict__ tri, unsigned long long n, uint8_t *__restrict__ cls,
                                                          double *__restrict__ seg, uint8_t *__restrict__ edge, double *__restrict__ t, uint8_t *__restrict__ on)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double *p = tri + 9 * i;
        const PlaneTri r = plane_tri(load_plane(planes, i), d3{p[0], p[1], p[2]}, d3{p[3], p[4], p[5]}, d3{p[6], p[7], p[8]});
        cls[i] = (uint8_t)r.cls;
        if (seg) { double *s = seg + 6 * i; s[0] = r.a.x; s[1] = r.a.y; s[2] = r.a.z; s[3] = r.b.x; s[4] = r.b.y; s[5] = r.b.z; }
        if (edge) { edge[2 * i] = (uint8_t)r.edge_a; edge[2 * i + 1] = (uint8_t)r.edge_b; }
        if (t) { t[2 * i] = r.ta; t[2 * i + 1] = r.tb; }
        if (on) on[i] = (uint8_t)r.on;
    }
}

}  // namespace cd
