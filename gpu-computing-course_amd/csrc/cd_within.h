// cd_within.h -- all-results point and ray queries: every triangle within a point's radius, every triangle a ray hits.  Not reference
// behaviour.
//   The single-answer queries (cd_points.h, cd_rays.h) run their exact test inline because their bound shrinks with every candidate.
//   Here the bound is the item's own rmax / tmax and never shrinks, so these queries take the pair queries' pattern (cd_proximity.h): a
//   filter walk that queues candidates, then the exact predicate at full lanes.
//   k_within_descend / k_rays_all_descend : one lane per item, in the order given (neighbouring items share a wave: coherent items
//       should be neighbours), one wave per workgroup.  The lane walks the records from the ROOT (prox_walk over RecCursor, cd_bvh.h:
//       the walk, its step bound and its guards are described there) and enters a subtree when the single-answer query's box filter
//       passes with the item's own bound: !(pt_box2 > rmax^2) for a point, ray_box over [0, tmax] for a ray.  Leaf hits (item, leaf
//       position) go through prox_walk's wave-shared LDS queue to the workgroup's shard, 64 at a time.  n == 1 has no records: every
//       item is a candidate against leaf 0.
//   k_within_exact / k_rays_all_exact     : FP64, one candidate per thread and round (ShardSlice): pt_tri / ray_tri on the item and the
//       leaf's vertices, a row for dist <= rmax / ray_tri's hit, appended with one atomic per workgroup and round (pair_append); nothing
//       is written at or past cap rows.  Every candidate is one exact evaluation (n_tested).
//   The filters only filter.  The pads are those of cd_points.h and cd_rays.h, and a subtree is skipped here exactly when those kernels
//       skip it before their first candidate (best = rmax, tbest = tmax): the proofs in those headers cover this case as it stands, so
//       every (item, triangle) the predicate accepts is a candidate and the predicate alone decides.  The rows and every value in them
//       therefore depend on the mesh and the items only.
//   A shard that overflows is detected from its counter (nothing is written past its capacity); the host grows the buffer and redoes the
//       pass.  The first allocation is WITHIN_SHARD_FIRST candidates a shard.
//   Known limit: an item whose bound meets every box (rmax = +inf) walks the whole tree in ONE lane -- correct and bounded by the walk's
//       step rule, but slow: 2 n moves while the other lanes of its wave wait.
#pragma once
#include "cd_points.h"

namespace cd {

constexpr unsigned long long WITHIN_SHARD_FIRST = 1ull << 14;            // candidates a shard in the first allocation (NSHARD shards)

// prox_walk's filters: the single-answer queries' box tests with the item's own bound
struct PointFilter {
    d3 p; double pad, r2;
    __device__ __forceinline__ bool meets(const RecCursor &w) const { return !(pt_box2(w.h0, w.h1, p, pad) > r2); }   // CLOSED; a NaN enters
};
struct RayFilter {
    d3 o, d; double pad, tmax;
    __device__ __forceinline__ bool meets(const RecCursor &w) const { return ray_box(w.h0, w.h1, o, d, pad, tmax); }
};

// The descent of one wave of items.  One wave per workgroup; every lane of it calls this (a lane with no item: active = false).
template <class Filter>
__device__ __forceinline__ void within_walk(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, int n, uint32_t item, bool active,
                                            const Filter q, ProxState *__restrict__ st, uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (n == 1) {                                                        // no records: leaf 0 is the whole tree
        const uint32_t sh = blockIdx.x & (NSHARD - 1);                   // (the workgroup's shard, as prox_walk takes it)
        const unsigned long long bal = __ballot(active);
        unsigned long long base = 0;
        if (threadIdx.x == 0 && bal) base = atomicAdd(&st->shard[sh * PROX_SHARD_STRIDE], (unsigned long long)__popcll(bal));
        base = __shfl(base, 0);
        const unsigned long long at = base + (unsigned long long)__popcll(bal & ((1ull << threadIdx.x) - 1ull));
        if (active && at < shard_cap) cand[(size_t)sh * shard_cap + at] = make_uint2(item, 0u);
        return;
    }
    RecCursor w{};
    if (active) active = w.start_root(recs, n, (uint32_t)*root_name);    // (no tree: nothing is read; no candidates)
    prox_walk(recs, n, item, active, w, q, st->shard, cand, shard_cap);
}

__global__ __launch_bounds__(PROX_DESC_THREADS) void k_within_descend(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name,
                                                                      const double *__restrict__ root_box, int n, const uint32_t *__restrict__ sort_flags /* 9 words */,
                                                                      const double *__restrict__ points, unsigned long long np, ProxState *__restrict__ st,
                                                                      uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * PROX_DESC_THREADS + threadIdx.x;
    const bool active = i < np;
    PointFilter q{};
    if (active) {
        const double *r = points + 4 * i;
        q.p = d3{r[0], r[1], r[2]};
        q.r2 = r[3] * r[3];                                              // (a huge finite rmax: +inf, which culls nothing)
        q.pad = dmax_abs3(root_max_abs(root_box), q.p) * PROX_SLACK;
    }
    within_walk(recs, root_name, n, (uint32_t)i, active, q, st, cand, shard_cap);
}

__global__ __launch_bounds__(PROX_DESC_THREADS) void k_rays_all_descend(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name,
                                                                        const double *__restrict__ root_box, int n, const uint32_t *__restrict__ sort_flags /* 9 words */,
                                                                        const double *__restrict__ rays, unsigned long long nr, ProxState *__restrict__ st,
                                                                        uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * PROX_DESC_THREADS + threadIdx.x;
    const bool active = i < nr;
    RayFilter q{};
    if (active) {
        const double *r = rays + 7 * i;
        q.o = d3{r[0], r[1], r[2]}; q.d = d3{r[3], r[4], r[5]}; q.tmax = r[6];
        q.pad = dmax_abs3(root_max_abs(root_box), q.o) * PROX_SLACK;
    }
    within_walk(recs, root_name, n, (uint32_t)i, active, q, st, cand, shard_cap);
}

// rows[2 at] = the item, rows[2 at + 1] = the face index; the other arrays (each may be NULL): the triangle's ID and pt_tri's values
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_within_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                    const uint32_t *__restrict__ perm, const double *__restrict__ verts, const double *__restrict__ points,
                                                                    ProxState *__restrict__ st, unsigned long long cap, uint32_t *__restrict__ rows,
                                                                    uint32_t *__restrict__ ids, double *__restrict__ dist, double *__restrict__ closest,
                                                                    double *__restrict__ uv, uint8_t *__restrict__ feature, uint8_t *__restrict__ side)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long tested = 0;
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        bool hit = false;
        uint2 c = make_uint2(0u, 0u);
        uint32_t id = 0;
        PtTri r{};
        if (i < sl.total) {
            c = sl.list[i];
            const LeafTri lt = leaf[c.y];
            const double *p = points + 4 * (size_t)c.x;
            ++tested;
            r = pt_tri(d3{p[0], p[1], p[2]}, load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            hit = r.dist <= p[3];
            id = lt.id;
        }
        pair_append(hit, &st->n_pairs, cap, [&](unsigned long long at) {
            rows[2 * at] = c.x; rows[2 * at + 1] = perm[c.y];
            if (ids) ids[at] = id;
            if (dist) dist[at] = r.dist;
            if (closest) { closest[3 * at] = r.q.x; closest[3 * at + 1] = r.q.y; closest[3 * at + 2] = r.q.z; }
            if (uv) { uv[2 * at] = r.u; uv[2 * at + 1] = r.v; }
            if (feature) feature[at] = (uint8_t)r.feature;
            if (side) side[at] = (uint8_t)r.side;
        });
    }
    group_counters_add<1>(&tested, &st->n_tested);
}

// rows as k_within_exact's; the other arrays (each may be NULL): the triangle's ID and ray_tri's values
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_rays_all_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                      const uint32_t *__restrict__ perm, const double *__restrict__ verts, const double *__restrict__ rays,
                                                                      ProxState *__restrict__ st, unsigned long long cap, uint32_t *__restrict__ rows,
                                                                      uint32_t *__restrict__ ids, double *__restrict__ t_out, double *__restrict__ uv,
                                                                      uint8_t *__restrict__ side)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long tested = 0;
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        uint2 c = make_uint2(0u, 0u);
        uint32_t id = 0;
        RayHit h{false, 0.0, 0.0, 0.0, 0u};
        if (i < sl.total) {
            c = sl.list[i];
            const LeafTri lt = leaf[c.y];
            const double *r = rays + 7 * (size_t)c.x;
            ++tested;
            h = ray_tri(d3{r[0], r[1], r[2]}, d3{r[3], r[4], r[5]}, r[6], load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            id = lt.id;
        }
        pair_append(h.hit, &st->n_pairs, cap, [&](unsigned long long at) {
            rows[2 * at] = c.x; rows[2 * at + 1] = perm[c.y];
            if (ids) ids[at] = id;
            if (t_out) t_out[at] = h.t;
            if (uv) { uv[2 * at] = h.u; uv[2 * at + 1] = h.v; }
            if (side) side[at] = (uint8_t)h.side;
        });
    }
    group_counters_add<1>(&tested, &st->n_tested);
}

}  // namespace cd
