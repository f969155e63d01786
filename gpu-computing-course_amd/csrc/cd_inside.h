// cd_inside.h -- inside / outside of a closed mesh for points: crossings of an axis-parallel line counted with one owner each.  Not
// reference behaviour.
//   k_points_inside<C> : one lane per query point, in the order given (neighbouring points share a wave: coherent points should be
//       neighbours), one wave per workgroup.  The lane walks the records from the ROOT in the queries' stackless pre-order (RecCursor,
//       cd_bvh.h: the walk, its step bound and its guards are described there) along the whole COLUMN of its point, the line through p
//       parallel to axis C: with a = (C + 1) % 3 and b = (C + 2) % 3 a subtree is entered when p_a and p_b lie in its box on the axes a
//       and b; axis C is not tested.  No bound shrinks, so there is no seed phase.
//       At a leaf the exact FP64 predicate column_tri (cd_math.h) runs INLINE and the lane adds to four registers: the faces that cover
//       p above it and below it (n_above, n_below) and the sums of their orientations (w_above, w_below).  Integer sums: the result
//       does not depend on the order of the walk.  No candidate buffer, no atomics on results, nothing that can overflow.
//       inside = w_above != 0, or with `parity` n_above odd.  n == 1 has no records: the lane tests leaf 0 and is done.
//   The filter only filters.  A box is the stored fp32 bounds read as [lo, prox_hi(hi)] (converted exactly) and padded as pt_box2 pads
//       them: per axis the subtree is skipped only when  (lo - pad) - p > 0  or  (p - hi) - pad > 0,  pad = 2^-20 max(M, |p|_inf).
//       column_tri's gate lets a face cover only when p_a and p_b lie in the CLOSED ranges of its own three vertices, compared exactly:
//       p is then inside the face's FP64 (a, b) box, every stored box of an ancestor contains that box (lo rounded down, prox_hi(hi)
//       an upper bound), so lo <= p <= hi holds there before any pad and neither difference above is positive.  Every face that can
//       count is reached; which other faces are tested changes the counters only.  The comparisons are written so that a NaN enters.
//   k_column_tri_points : column_tri on explicit operands, the pin of the device function (cd_column_tri_points).
#pragma once
#include "cd_points.h"

namespace cd {

constexpr int INSIDE_THREADS = 64;

// does the column of p meet the padded box on the axes A and B?  (h0, h1: a record half, lo = h0.xyz, hi = (h0.w, h1.x, h1.y))
template <int A, int B>
__device__ __forceinline__ bool column_box_meets(const float4 h0, const float4 h1, const double pa, const double pb, const double pad)
{
    const float lo_a = A == 0 ? h0.x : (A == 1 ? h0.y : h0.z), hi_a = A == 0 ? h0.w : (A == 1 ? h1.x : h1.y);
    const float lo_b = B == 0 ? h0.x : (B == 1 ? h0.y : h0.z), hi_b = B == 0 ? h0.w : (B == 1 ? h1.x : h1.y);
    return !(((double)lo_a - pad) - pa > 0.0 || (pa - (double)prox_hi(hi_a)) - pad > 0.0 ||
             ((double)lo_b - pad) - pb > 0.0 || (pb - (double)prox_hi(hi_b)) - pad > 0.0);       // CLOSED; a NaN enters
}

// points: np rows of `stride` doubles, the first three the point (3: cd_points_inside; 4: cd_closest_points' rows, of cd_signed_distance)
template <int C>
__global__ __launch_bounds__(INSIDE_THREADS) void k_points_inside(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, const LeafTri *__restrict__ leaf,
                                                                  const double *__restrict__ verts, const double *__restrict__ root_box, int n,
                                                                  const uint32_t *__restrict__ sort_flags /* 9 words */, const double *__restrict__ points, int stride,
                                                                  unsigned long long np, int parity, PointState *__restrict__ st, uint8_t *__restrict__ inside,
                                                                  uint32_t *__restrict__ n_above, uint32_t *__restrict__ n_below, int32_t *__restrict__ w_above,
                                                                  int32_t *__restrict__ w_below)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    constexpr int A = (C + 1) % 3, B = (C + 2) % 3;
    const unsigned long long i = (unsigned long long)blockIdx.x * INSIDE_THREADS + threadIdx.x;
    bool active = i < np;
    d3 p{0.0, 0.0, 0.0};
    double pad = 0.0;
    if (active) {
        const double *r = points + (size_t)stride * i;
        p = d3{r[0], r[1], r[2]};
        pad = dmax_abs3(root_max_abs(root_box), p) * PROX_SLACK;
    }
    const double pa = axis3(p, A), pb = axis3(p, B);
    uint32_t na = 0, nb = 0, visits = 0, tests = 0;
    int32_t wa = 0, wb = 0;
    RecCursor w{};
    const bool leaf_only = n == 1;                                       // no records: leaf 0 is the whole tree
    if (active && !leaf_only) active = w.start_root(recs, n, (uint32_t)*root_name);   // (no tree: nothing is read; nothing is counted)
    while (active) {
        bool test = leaf_only;
        uint32_t k = 0;
        if (!leaf_only) {
            ++visits;
            const bool enter = column_box_meets<A, B>(w.h0, w.h1, pa, pb, pad);
            if (enter && w.internal(n)) {
                if (!w.descend(recs, n)) break;
                continue;
            }
            if (enter && w.leaf(n)) { test = true; k = w.leaf_index(); }
        }
        if (test) {
            ++tests;
            const LeafTri lt = leaf[k];
            const ColumnTri r = column_tri(p, C, load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            if (r.counted) {
                if (r.above) { ++na; wa += r.o; }
                else { ++nb; wb += r.o; }
            }
        }
        if (leaf_only || !w.next(recs, n)) break;
    }
    const bool in = parity ? (na & 1u) != 0u : wa != 0;
    if (i < np) {
        inside[i] = in ? 1 : 0;
        if (n_above) n_above[i] = na;
        if (n_below) n_below[i] = nb;
        if (w_above) w_above[i] = wa;
        if (w_below) w_below[i] = wb;
    }
    item_counters_add(i < np && in, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);
}

// cd_column_tri_points: column_tri on explicit operands, n x 3 doubles (p) and n x 9 (v0, v1, v2); cover = o, the gate included
__global__ __launch_bounds__(256) void k_column_tri_points(const double *__restrict__ pts, const double *__restrict__ tri, unsigned long long n, int axis,
                                                           int8_t *__restrict__ cover, uint8_t *__restrict__ above, double *__restrict__ E, double *__restrict__ zc,
                                                           double *__restrict__ S)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double *q = pts + 3 * i, *p = tri + 9 * i;
        const ColumnTri r = column_tri(d3{q[0], q[1], q[2]}, axis, d3{p[0], p[1], p[2]}, d3{p[3], p[4], p[5]}, d3{p[6], p[7], p[8]});
        cover[i] = (int8_t)r.o;
        if (above) above[i] = r.above ? 1 : 0;
        if (E) { E[3 * i] = r.e0; E[3 * i + 1] = r.e1; E[3 * i + 2] = r.e2; }
        if (zc) zc[i] = r.zc;
        if (S) S[i] = r.s;
    }
}

}  // namespace cd
