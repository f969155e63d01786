// cd_sweep.h -- swept-point queries: points that move linearly from p0 to p1 against the mesh whose vertices move linearly from x0 (the
// context's vertices, the tree's) to x1, each point with a threshold `dist` of its own: which triangles the point comes within dist of
// during the step, when first, and where on the triangle.  Not reference behaviour.  Per (point, triangle):
// conservative advancement with report threshold dist and target h = dist / 2 (pt_advance below, restated in tests/sweep_ref.py bit for
// bit): ccd_advance (cd_ccd.h) with pt_tri (cd_math.h) in place of tri_distance and a rate bound of the point's own.
//   The swept tree is cd_ccd.h's (k_ccd_links, k_ccd_refit), launched on this query's own swept records and counters.
//   k_sweep_descend : the all-rows query's filter, in cd_within.h's pattern: one lane per item, in the order given, one wave per
//       workgroup; within_walk over the SWEPT records from the root with BoxFilter<HiTrue>; the query box is the FP64 box of {p0, p1}
//       widened with directed rounding by the item's own ccd_pad, 2 dist + 2 dist 2^-20 + M 2^-20, M the larger of the refit's M and the
//       item's largest |coordinate|.  n == 1 has no records: every item is a candidate against leaf 0.
//   k_sweep_exact   : FP64, one candidate per thread and round (ShardSlice): the skip_vertex filter, the gate, pt_advance; a row for a
//       reported pair, appended with one atomic per workgroup and round (pair_append); nothing is written at or past cap rows.
//   k_sweep_first   : the first contact of every item, in cd_points.h's pattern: one lane per item walks the swept records from the root
//       with the same box filter and runs the filter, the gate and pt_advance INLINE at a leaf, because the lane's best toi so far cuts
//       later advancements short (pt_advance's `cut`).  Of the reported triangles the smallest (toi, ID, face index) wins.
//   k_pt_advance_points : pt_advance on explicit positions (cd_pt_advance_points): the pin of the device code.
//   The filter only filters: the gate (below) passes only when the FP64 boxes lie within 2 dist of each other up to the rounding of four
//       additions, the swept records' boxes are true bounds of the triangles' swept boxes (fp32 rounded outward), and the pad's 2^-20
//       terms exceed those roundings by 2^30: every pair through the gate is a candidate, and the gate and pt_advance alone decide.
#pragma once
#include "cd_within.h"
#include "cd_ccd.h"

namespace cd {

constexpr uint32_t SWEEP_NONE = 0xffffffffu;          // no face (cd_sweep_points), no vertex to skip (skip_vertex)
constexpr int SWEEP_THREADS = 64;                     // k_sweep_first

// ---------------------------------------------------------------- the per-pair function
// The triangle's vertex k (0..2) at x0 and x1 (p0 / p1: what swept_box reads) and the point at the two ends (q0 / q1).
struct SweepMeshSrc {
    const double *__restrict__ x0; const double *__restrict__ x1; const double *__restrict__ item /* 7 doubles */; uint32_t v0, v1, v2;
    __device__ __forceinline__ uint32_t vid(int k) const { return k == 0 ? v0 : (k == 1 ? v1 : v2); }
    __device__ __forceinline__ d3 p0(int k) const { return load_vertex(x0, vid(k)); }
    __device__ __forceinline__ d3 p1(int k) const { return load_vertex(x1, vid(k)); }
    __device__ __forceinline__ d3 q0() const { return d3{item[0], item[1], item[2]}; }
    __device__ __forceinline__ d3 q1() const { return d3{item[3], item[4], item[5]}; }
    __device__ __forceinline__ void launder() { asm volatile("" : "+v"(x0), "+v"(x1), "+v"(item)); }
};
struct SweepPointSrc {                                // item: 7 doubles (p0, p1, dist); tri: 18 doubles, a0 a1 a2 then b0 b1 b2
    const double *__restrict__ item; const double *__restrict__ tri;
    __device__ __forceinline__ d3 p0(int k) const { return d3{tri[3 * k], tri[3 * k + 1], tri[3 * k + 2]}; }
    __device__ __forceinline__ d3 p1(int k) const { return d3{tri[9 + 3 * k], tri[9 + 3 * k + 1], tri[9 + 3 * k + 2]}; }
    __device__ __forceinline__ d3 q0() const { return d3{item[0], item[1], item[2]}; }
    __device__ __forceinline__ d3 q1() const { return d3{item[3], item[4], item[5]}; }
    __device__ __forceinline__ void launder() { asm volatile("" : "+v"(item), "+v"(tri)); }
};

// L = max_i |(b_i - a_i) - (p1 - p0)| (1 + 2^-20), |v| = sqrt((x x + y y) + z z): no point of the triangle moves faster, relative to the
// point, than its fastest vertex does (a point of the triangle moves by a convex combination of the three differences).
template <class S> __device__ __forceinline__ double pt_rate(const S &s)
{
    const d3 dp = sub(s.q1(), s.q0());
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const d3 v = sub(sub(s.p1(k), s.p0(k)), dp);
        const double l = __builtin_sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
        m = l > m ? l : m;
    }
    return m * CCD_L_SLACK;
}

// where the advancement evaluates a position that moves from a to b: a itself (stage 0), a + t (b - a) (stage 1), b itself (stage 2)
__device__ __forceinline__ d3 sweep_at(const d3 a, const d3 b, int stage, double t)
{
    if (stage == 0) return a;
    if (stage == 2) return b;
    return d3{a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z)};
}

// Conservative advancement.  Reported: toi finite; r.dist <= dist, or r.dist > dist for a pair left unresolved
// after CCD_MAX_EVALS evaluations (toi = the t of the last one).  Not reported: toi = +inf.  r: pt_tri of the last evaluation, q on the
// triangle as it stands there.  CUT (k_sweep_first): the advancement stops, not reported, as soon as the t of its next evaluation
// exceeds `cut` (strictly: a pair that would report AT cut is still evaluated).  t only grows and an unresolved pair's toi is its last
// t, so a pair stopped this way would have reported, if at all, with toi > cut.
template <bool CUT, class S> __device__ inline void pt_advance(const S &src, double dist, double cut, double &toi, PtTri &rout, uint32_t &evals)
{
    S s = src;
    const double h = dist * 0.5, L = pt_rate(s);
    double t = 0.0, res = __builtin_inf();
    PtTri r{};
    int stage = 0;
    uint32_t n = 0;
    for (;;) {                                        // one pt_tri call site (inlined once)
        s.launder();                                  // (the positions are loaded again each round)
        r = pt_tri(sweep_at(s.q0(), s.q1(), stage, t), sweep_at(s.p0(0), s.p1(0), stage, t), sweep_at(s.p0(1), s.p1(1), stage, t),
                   sweep_at(s.p0(2), s.p1(2), stage, t));
        ++n;
        if (r.dist <= dist) { res = stage == 2 ? 1.0 : t; break; }
        if (stage == 2 || L == 0.0) break;            // apart at the end, or a common translation apart at the start: not reported
        if (n >= (uint32_t)CCD_MAX_EVALS) { res = t; break; }   // unresolved (r.dist > dist)
        const double tn = t + (r.dist - h) / L;
        if (tn >= 1.0) stage = 2; else { t = tn; stage = 1; }
        if (CUT && (stage == 2 ? 1.0 : t) > cut) break;
    }
    toi = res; rout = r; evals = n;
}

// The FP64 gate: the box of {p0, p1} and the triangle's swept box, each widened by dist (lo - dist, hi + dist), overlap (closed).
template <class S> __device__ __forceinline__ bool pt_gate(const S &s, double dist)
{
    const d3 a = s.q0(), b = s.q1();
    const Box p{fmin2(a.x, b.x), fmax2(a.x, b.x), fmin2(a.y, b.y), fmax2(a.y, b.y), fmin2(a.z, b.z), fmax2(a.z, b.z)};
    const Box q = swept_box(s, 0);
    return (p.x1 - dist) <= (q.x2 + dist) && (q.x1 - dist) <= (p.x2 + dist) && (p.y1 - dist) <= (q.y2 + dist) &&
           (q.y1 - dist) <= (p.y2 + dist) && (p.z1 - dist) <= (q.z2 + dist) && (q.z1 - dist) <= (p.z2 + dist);
}

// ---------------------------------------------------------------- the walk's filter
// The item's fp32 query box: the box of {p0, p1} widened by ccd_pad's formula with the item's own dist and M = max(the refit's, the
// item's largest |coordinate|).  n == 1: no refit has run (and no box is compared).
__device__ __forceinline__ BoxFilter<HiTrue> sweep_filter(const double *__restrict__ r, const CcdState *__restrict__ cst)
{
    const d3 a = d3{r[0], r[1], r[2]}, b = d3{r[3], r[4], r[5]};
    const double dist = r[6];
    const double m = dmax_abs3(dmax_abs3((double)__uint_as_float(cst->m_bits), a), b);
    const float pad = __double2float_ru(2.0 * dist + 2.0 * dist * PROX_SLACK + m * PROX_SLACK);
    const Box p{fmin2(a.x, b.x), fmax2(a.x, b.x), fmin2(a.y, b.y), fmax2(a.y, b.y), fmin2(a.z, b.z), fmax2(a.z, b.z)};
    return BoxFilter<HiTrue>{query_box32(p, pad)};
}

// ---------------------------------------------------------------- all rows
__global__ __launch_bounds__(PROX_DESC_THREADS) void k_sweep_descend(const NodeRec32 *__restrict__ swept, const int32_t *__restrict__ root_name, int n,
                                                                     const uint32_t *__restrict__ sort_flags /* 9 words */, const double *__restrict__ items,
                                                                     unsigned long long np, const CcdState *__restrict__ cst, ProxState *__restrict__ st,
                                                                     uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * PROX_DESC_THREADS + threadIdx.x;
    const bool active = i < np;
    BoxFilter<HiTrue> q{};
    if (active) q = sweep_filter(items + 7 * i, cst);
    within_walk(swept, root_name, n, (uint32_t)i, active, q, st, cand, shard_cap);
}

// rows[2 at] = the item, rows[2 at + 1] = the face index; the other arrays (each may be NULL): the triangle's ID, toi and pt_tri's
// values of the reporting evaluation.  Counters: pairs through the gate (st->n_tested), pt_tri evaluations and unresolved rows (cst).
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_sweep_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                   const uint32_t *__restrict__ perm, const double *__restrict__ x0, const double *__restrict__ x1,
                                                                   const double *__restrict__ items, const uint32_t *__restrict__ skip, ProxState *__restrict__ st,
                                                                   CcdState *__restrict__ cst, unsigned long long cap, uint32_t *__restrict__ rows,
                                                                   uint32_t *__restrict__ ids, double *__restrict__ toi_out, double *__restrict__ dist_out,
                                                                   double *__restrict__ closest, double *__restrict__ uv, uint8_t *__restrict__ feature,
                                                                   uint8_t *__restrict__ side)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long sums[3] = {0, 0, 0};                              // through the gate, evaluations, unresolved
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        bool hit = false;
        uint2 c = make_uint2(0u, 0u);
        uint32_t id = 0;
        double toi = 0.0;
        PtTri r{};
        if (i < sl.total) {
            c = sl.list[i];
            const LeafTri lt = leaf[c.y];
            const uint32_t sv = skip ? skip[c.x] : SWEEP_NONE;
            if (sv == SWEEP_NONE || (lt.v0 != sv && lt.v1 != sv && lt.v2 != sv)) {
                const double *it = items + 7 * (size_t)c.x;
                const double dist = it[6];
                const SweepMeshSrc src{x0, x1, it, lt.v0, lt.v1, lt.v2};
                if (pt_gate(src, dist)) {
                    ++sums[0];
                    uint32_t ne = 0;
                    pt_advance<false>(src, dist, 0.0, toi, r, ne);
                    sums[1] += ne;
                    hit = toi <= 1.0;
                    sums[2] += (hit && !(r.dist <= dist)) ? 1u : 0u;
                    id = lt.id;
                }
            }
        }
        pair_append(hit, &st->n_pairs, cap, [&](unsigned long long at) {
            rows[2 * at] = c.x; rows[2 * at + 1] = perm[c.y];
            if (ids) ids[at] = id;
            if (toi_out) toi_out[at] = toi;
            if (dist_out) dist_out[at] = r.dist;
            if (closest) { closest[3 * at] = r.q.x; closest[3 * at + 1] = r.q.y; closest[3 * at + 2] = r.q.z; }
            if (uv) { uv[2 * at] = r.u; uv[2 * at + 1] = r.v; }
            if (feature) feature[at] = (uint8_t)r.feature;
            if (side) side[at] = (uint8_t)r.side;
        });
    }
    group_counters_add<3>(sums, &st->n_tested, &cst->n_evals, &cst->n_unresolved);
}

// ---------------------------------------------------------------- first contact
// face[i] = SWEEP_NONE, toi[i] = +inf and zeros elsewhere for an item no triangle is reported for.  Counters: items with a row, records
// visited, pt_tri evaluations (which the cut-off lowers; the answer it leaves alone).
__global__ __launch_bounds__(SWEEP_THREADS) void k_sweep_first(const NodeRec32 *__restrict__ swept, const int32_t *__restrict__ root_name, const LeafTri *__restrict__ leaf,
                                                               const uint32_t *__restrict__ perm, const double *__restrict__ x0, const double *__restrict__ x1, int n,
                                                               const uint32_t *__restrict__ sort_flags /* 9 words */, const double *__restrict__ items,
                                                               const uint32_t *__restrict__ skip, unsigned long long np, const CcdState *__restrict__ cst,
                                                               PointState *__restrict__ st, uint32_t *__restrict__ face, uint32_t *__restrict__ ids,
                                                               double *__restrict__ toi_out, double *__restrict__ dist_out, double *__restrict__ closest,
                                                               double *__restrict__ uv, uint8_t *__restrict__ feature, uint8_t *__restrict__ side)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * SWEEP_THREADS + threadIdx.x;
    bool active = i < np;
    const double *it = items + 7 * (active ? i : 0ull);
    BoxFilter<HiTrue> q{};
    double dist = 0.0;
    uint32_t sv = SWEEP_NONE;
    const bool leaf_only = n == 1;                                       // no records: leaf 0 is the whole tree
    if (active) {
        dist = it[6];
        if (skip) sv = skip[i];
        if (!leaf_only) q = sweep_filter(it, cst);
    }
    double btoi = __builtin_inf();                                       // the best row so far: the smallest (toi, ID, face index)
    uint32_t bface = SWEEP_NONE, bid = 0u;
    PtTri br{};
    uint32_t visits = 0, tests = 0;
    RecCursor w{};
    if (active && !leaf_only) active = w.start_root(swept, n, (uint32_t)*root_name);   // (no tree: nothing is read; nothing is found)
    while (active) {
        bool test = leaf_only;
        uint32_t k = 0;
        if (!leaf_only) {
            ++visits;
            const bool enter = q.meets(w);
            if (enter && w.internal(n)) {
                if (!w.descend(swept, n)) break;
                continue;
            }
            if (enter && w.leaf(n)) { test = true; k = w.leaf_index(); }
        }
        if (test) {
            const LeafTri lt = leaf[k];
            if (sv == SWEEP_NONE || (lt.v0 != sv && lt.v1 != sv && lt.v2 != sv)) {
                const SweepMeshSrc src{x0, x1, it, lt.v0, lt.v1, lt.v2};
                if (pt_gate(src, dist)) {
                    double toi; PtTri r; uint32_t ne;
                    pt_advance<true>(src, dist, btoi, toi, r, ne);
                    tests += ne;
                    if (toi <= 1.0) {
                        const uint32_t f = perm[k];
                        if (bface == SWEEP_NONE || toi < btoi || (toi == btoi && (lt.id < bid || (lt.id == bid && f < bface)))) {
                            bface = f; bid = lt.id; btoi = toi; br = r;
                        }
                    }
                }
            }
        }
        if (leaf_only || !w.next(swept, n)) break;
    }
    if (i < np) {
        const bool found = bface != SWEEP_NONE;
        face[i] = bface;
        if (ids) ids[i] = found ? bid : 0u;
        if (toi_out) toi_out[i] = btoi;
        if (dist_out) dist_out[i] = found ? br.dist : 0.0;
        if (closest) { closest[3 * i] = found ? br.q.x : 0.0; closest[3 * i + 1] = found ? br.q.y : 0.0; closest[3 * i + 2] = found ? br.q.z : 0.0; }
        if (uv) { uv[2 * i] = found ? br.u : 0.0; uv[2 * i + 1] = found ? br.v : 0.0; }
        if (feature) feature[i] = (uint8_t)(found ? br.feature : 0u);
        if (side) side[i] = (uint8_t)(found ? br.side : 0u);
    }
    item_counters_add(i < np && bface != SWEEP_NONE, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);
}

// cd_pt_advance_points: pt_advance on explicit positions, n x 7 doubles (p0, p1, dist) and n x 18 (a0 a1 a2, b0 b1 b2)
__global__ __launch_bounds__(CCD_THREADS) void k_pt_advance_points(const double *__restrict__ items, const double *__restrict__ tri, unsigned long long n,
                                                                   double *__restrict__ toi, double *__restrict__ dist, double *__restrict__ closest,
                                                                   double *__restrict__ uv, uint8_t *__restrict__ feature, uint8_t *__restrict__ side,
                                                                   uint32_t *__restrict__ evals)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * CCD_THREADS + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * CCD_THREADS) {
        double t; PtTri r; uint32_t e;
        pt_advance<false>(SweepPointSrc{items + 7 * i, tri + 18 * i}, items[7 * i + 6], 0.0, t, r, e);
        toi[i] = t;
        if (dist) dist[i] = r.dist;
        if (closest) { closest[3 * i] = r.q.x; closest[3 * i + 1] = r.q.y; closest[3 * i + 2] = r.q.z; }
        if (uv) { uv[2 * i] = r.u; uv[2 * i + 1] = r.v; }
        if (feature) feature[i] = (uint8_t)r.feature;
        if (side) side[i] = (uint8_t)r.side;
        if (evals) evals[i] = e;
    }
}

}  // namespace cd
