// cd_sweep_segments.h -- swept-segment queries: segments whose ends move linearly, a from a0 to a1 and b from b0 to b1, against the mesh
// whose vertices move linearly from x0 (the context's vertices, the tree's) to x1, each segment with a threshold `dist` of its own: which
// triangles the segment comes within dist of during the step, when first, and where on the segment and on the triangle.  The edge-edge
// half of a CCD pass, the moving capsule, the strand element.  Not reference behaviour.
//   An item is 13 doubles (a0, b0, a1, b1, dist); a0 == b0 and a1 == b1 is a moving point.  Per (segment, triangle): conservative
//   advancement with report threshold dist and target h = dist / 2 (seg_advance below, restated in tests/swept_segment_ref.py bit for
//   bit): cd_sweep.h's pt_advance with seg_tri (cd_math.h) in place of pt_tri and a rate bound over the six (end, vertex) differences.
//   The swept tree is cd_ccd.h's (k_ccd_links, k_ccd_refit), launched on the swept-point queries' own records and counters.
//   k_sweep_segments_descend : k_sweep_descend with the query box of the four points {a0, b0, a1, b1}, widened with directed rounding by
//       ccd_pad's formula, 2 dist + 2 dist 2^-20 + M 2^-20, M the larger of the refit's M and the item's largest |coordinate| (twelve).
//       n == 1 has no records: every item is a candidate against leaf 0.
//   k_sweep_segments_exact   : k_sweep_exact's body: the two-index skip filter, the gate, seg_advance; a row for a reported pair,
//       appended with one atomic per workgroup and round (pair_append); nothing is written at or past cap rows.
//   k_sweep_segments_first   : k_sweep_first's lane: the filter, the gate and seg_advance INLINE at a leaf, the lane's best toi so far
//       cutting later advancements short.  Of the reported triangles the smallest (toi, ID, face index) wins.  The lane carries only
//       the winner's (toi, stage, leaf, ID, face) and evaluates seg_tri once more at sweep_at(stage, toi) behind the walk: the same
//       operands and the same operations, so the same bits as the row's (section 25's trade: SegTri's twelve values stay out of the walk).
//   k_seg_advance_points : seg_advance on explicit positions (cd_seg_advance_points): the pin of the device code.
//   The filter only filters, by section 20's argument with four points in place of two: the gate passes only when the FP64 box of the
//       four points and the triangle's swept box lie within 2 dist of each other up to the rounding of four additions, the swept
//       records' boxes are true bounds of the triangles' swept boxes (fp32 rounded outward), the query box is the four points' box
//       rounded outward, and the pad's 2^-20 terms exceed those roundings by 2^30: every pair through the gate is a candidate, and
//       the gate and seg_advance alone decide.
#pragma once
#include "cd_sweep.h"
#include "cd_segments.h"

namespace cd {

constexpr int SWEEP_SEGMENT_THREADS = 64;             // k_sweep_segments_first

// ---------------------------------------------------------------- the per-pair function
// The triangle's vertex k (0..2) at x0 and x1 (p0 / p1: what swept_box reads) and the segment's ends at the two ends of the step.
struct SweepSegMeshSrc {
    const double *__restrict__ x0; const double *__restrict__ x1; const double *__restrict__ item /* 13 doubles */; uint32_t v0, v1, v2;
    __device__ __forceinline__ uint32_t vid(int k) const { return k == 0 ? v0 : (k == 1 ? v1 : v2); }
    __device__ __forceinline__ d3 p0(int k) const { return load_vertex(x0, vid(k)); }
    __device__ __forceinline__ d3 p1(int k) const { return load_vertex(x1, vid(k)); }
    __device__ __forceinline__ d3 a0() const { return d3{item[0], item[1], item[2]}; }
    __device__ __forceinline__ d3 b0() const { return d3{item[3], item[4], item[5]}; }
    __device__ __forceinline__ d3 a1() const { return d3{item[6], item[7], item[8]}; }
    __device__ __forceinline__ d3 b1() const { return d3{item[9], item[10], item[11]}; }
    __device__ __forceinline__ void launder() { asm volatile("" : "+v"(x0), "+v"(x1), "+v"(item)); }
};
struct SweepSegPointSrc {                             // item: 13 doubles; tri: 18 doubles, the vertices at x0 then at x1
    const double *__restrict__ item; const double *__restrict__ tri;
    __device__ __forceinline__ d3 p0(int k) const { return d3{tri[3 * k], tri[3 * k + 1], tri[3 * k + 2]}; }
    __device__ __forceinline__ d3 p1(int k) const { return d3{tri[9 + 3 * k], tri[9 + 3 * k + 1], tri[9 + 3 * k + 2]}; }
    __device__ __forceinline__ d3 a0() const { return d3{item[0], item[1], item[2]}; }
    __device__ __forceinline__ d3 b0() const { return d3{item[3], item[4], item[5]}; }
    __device__ __forceinline__ d3 a1() const { return d3{item[6], item[7], item[8]}; }
    __device__ __forceinline__ d3 b1() const { return d3{item[9], item[10], item[11]}; }
    __device__ __forceinline__ void launder() { asm volatile("" : "+v"(item), "+v"(tri)); }
};

// L = max over the ends j in {a, b} and the vertices i of |(x1_i - x0_i) - (j1 - j0)| (1 + 2^-20), |v| = sqrt((x x + y y) + z z): a point
// of the segment moves by a convex combination of its two ends' displacements and a point of the triangle by one of its three vertices',
// so the relative displacement of any two such points is a convex combination of the six differences.  With a == b at both ends the six
// norms are pt_rate's three, each twice.
template <class S> __device__ __forceinline__ double seg_rate(const S &s)
{
    const d3 da = sub(s.a1(), s.a0()), db = sub(s.b1(), s.b0());
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const d3 dv = sub(s.p1(k), s.p0(k));
        const d3 v = sub(dv, da), w = sub(dv, db);
        const double l = __builtin_sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
        m = l > m ? l : m;
        const double g = __builtin_sqrt((w.x * w.x + w.y * w.y) + w.z * w.z);
        m = g > m ? g : m;
    }
    return m * CCD_L_SLACK;
}

// seg_tri of the pair as it stands at (stage, t): every one of the five positions through sweep_at
template <class S> __device__ __forceinline__ SegTri seg_tri_at(const S &s, int stage, double t)
{
    return seg_tri(sweep_at(s.a0(), s.a1(), stage, t), sweep_at(s.b0(), s.b1(), stage, t), sweep_at(s.p0(0), s.p1(0), stage, t),
                   sweep_at(s.p0(1), s.p1(1), stage, t), sweep_at(s.p0(2), s.p1(2), stage, t));
}

// Conservative advancement: pt_advance's loop, word for word, with seg_tri.  Reported: toi finite; r.dist <= dist
// (a crossing evaluation has dist 0 and reports like any other), or r.dist > dist for a pair left unresolved after CCD_MAX_EVALS
// evaluations (toi = the t of the last one).  Not reported: toi = +inf.  r: seg_tri of the last evaluation, qs and qt on the segment and
// the triangle as they stand there; stage_out: where that evaluation was made (sweep_at's stage; with toi it names the operands again).
// CUT (k_sweep_segments_first): pt_advance's rule -- the advancement stops, not reported, as soon as the t of its next evaluation exceeds
// `cut`, strictly.
template <bool CUT, class S> __device__ inline void seg_advance(const S &src, double dist, double cut, double &toi, SegTri &rout, uint32_t &evals, int &stage_out)
{
    S s = src;
    const double h = dist * 0.5, L = seg_rate(s);
    double t = 0.0, res = __builtin_inf();
    SegTri r{};
    int stage = 0;
    uint32_t n = 0;
    for (;;) {                                        // one seg_tri call site (inlined once)
        s.launder();                                  // (the positions are loaded again each round)
        r = seg_tri_at(s, stage, t);
        ++n;
        if (r.dist <= dist) { res = stage == 2 ? 1.0 : t; break; }
        if (stage == 2 || L == 0.0) break;            // apart at the end, or a common translation apart at the start: not reported
        if (n >= (uint32_t)CCD_MAX_EVALS) { res = t; break; }   // unresolved (r.dist > dist)
        const double tn = t + (r.dist - h) / L;
        if (tn >= 1.0) stage = 2; else { t = tn; stage = 1; }
        if (CUT && (stage == 2 ? 1.0 : t) > cut) break;
    }
    toi = res; rout = r; evals = n; stage_out = stage;
}

// the FP64 box of the four points
template <class S> __device__ __forceinline__ Box seg_sweep_box(const S &s)
{
    const d3 a = s.a0(), b = s.b0(), c = s.a1(), d = s.b1();
    return Box{fmin2(fmin2(a.x, b.x), fmin2(c.x, d.x)), fmax2(fmax2(a.x, b.x), fmax2(c.x, d.x)), fmin2(fmin2(a.y, b.y), fmin2(c.y, d.y)),
               fmax2(fmax2(a.y, b.y), fmax2(c.y, d.y)), fmin2(fmin2(a.z, b.z), fmin2(c.z, d.z)), fmax2(fmax2(a.z, b.z), fmax2(c.z, d.z))};
}
// The FP64 gate, pt_gate's shape: the box of {a0, b0, a1, b1} and the triangle's swept box, each widened by dist, overlap (closed).
template <class S> __device__ __forceinline__ bool seg_gate(const S &s, double dist)
{
    const Box p = seg_sweep_box(s);
    const Box q = swept_box(s, 0);
    return (p.x1 - dist) <= (q.x2 + dist) && (q.x1 - dist) <= (p.x2 + dist) && (p.y1 - dist) <= (q.y2 + dist) &&
           (q.y1 - dist) <= (p.y2 + dist) && (p.z1 - dist) <= (q.z2 + dist) && (q.z1 - dist) <= (p.z2 + dist);
}
// item k's two skip indices against a triangle: true when the triangle holds neither (SWEEP_NONE: no index)
__device__ __forceinline__ bool seg_skip_passes(uint32_t s0, uint32_t s1, const LeafTri &lt)
{
    return (s0 == SWEEP_NONE || (lt.v0 != s0 && lt.v1 != s0 && lt.v2 != s0)) && (s1 == SWEEP_NONE || (lt.v0 != s1 && lt.v1 != s1 && lt.v2 != s1));
}

// ---------------------------------------------------------------- the walk's filter
// sweep_filter's sibling: the box of the four points widened by ccd_pad's formula with the item's own dist and M = max(the refit's, the
// item's largest |coordinate|).  n == 1: no refit has run (and no box is compared).
__device__ __forceinline__ BoxFilter<HiTrue> sweep_segment_filter(const double *__restrict__ r, const CcdState *__restrict__ cst)
{
    const SweepSegPointSrc s{r, nullptr};
    const double dist = r[12];
    const double m = dmax_abs3(dmax_abs3(dmax_abs3(dmax_abs3((double)__uint_as_float(cst->m_bits), s.a0()), s.b0()), s.a1()), s.b1());
    const float pad = __double2float_ru(2.0 * dist + 2.0 * dist * PROX_SLACK + m * PROX_SLACK);
    return BoxFilter<HiTrue>{query_box32(seg_sweep_box(s), pad)};
}

// ---------------------------------------------------------------- all rows
__global__ __launch_bounds__(PROX_DESC_THREADS) void k_sweep_segments_descend(const NodeRec32 *__restrict__ swept, const int32_t *__restrict__ root_name, int n,
                                                                              const uint32_t *__restrict__ sort_flags /* 9 words */, const double *__restrict__ items,
                                                                              unsigned long long np, const CcdState *__restrict__ cst, ProxState *__restrict__ st,
                                                                              uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * PROX_DESC_THREADS + threadIdx.x;
    const bool active = i < np;
    BoxFilter<HiTrue> q{};
    if (active) q = sweep_segment_filter(items + 13 * i, cst);
    within_walk(swept, root_name, n, (uint32_t)i, active, q, st, cand, shard_cap);
}

// the values of one reported pair into row / item `at` of the arrays (each may be NULL): SegOut with toi
struct SweepSegOut {
    SegOut o; double *toi;
    __device__ __forceinline__ void put(unsigned long long at, uint32_t id, double t, const SegTri &r) const
    {
        o.put(at, id, r);
        if (toi) toi[at] = t;
    }
};

// rows[2 at] = the item, rows[2 at + 1] = the face index; o: the triangle's ID, toi and seg_tri's values of the reporting evaluation.
// Counters: pairs through the gate (st->n_tested), seg_tri evaluations and unresolved rows (cst).
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_sweep_segments_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                            const uint32_t *__restrict__ perm, const double *__restrict__ x0, const double *__restrict__ x1,
                                                                            const double *__restrict__ items, const uint32_t *__restrict__ skip /* 2 an item */,
                                                                            ProxState *__restrict__ st, CcdState *__restrict__ cst, unsigned long long cap,
                                                                            uint32_t *__restrict__ rows, const SweepSegOut o)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long sums[3] = {0, 0, 0};                              // through the gate, evaluations, unresolved
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        bool hit = false;
        uint2 c = make_uint2(0u, 0u);
        uint32_t id = 0;
        double toi = 0.0;
        SegTri r{};
        if (i < sl.total) {
            c = sl.list[i];
            const LeafTri lt = leaf[c.y];
            const uint32_t s0 = skip ? skip[2 * (size_t)c.x] : SWEEP_NONE, s1 = skip ? skip[2 * (size_t)c.x + 1] : SWEEP_NONE;
            if (seg_skip_passes(s0, s1, lt)) {
                const double *it = items + 13 * (size_t)c.x;
                const double dist = it[12];
                const SweepSegMeshSrc src{x0, x1, it, lt.v0, lt.v1, lt.v2};
                if (seg_gate(src, dist)) {
                    ++sums[0];
                    uint32_t ne = 0;
                    int stage;
                    seg_advance<false>(src, dist, 0.0, toi, r, ne, stage);
                    sums[1] += ne;
                    hit = toi <= 1.0;
                    sums[2] += (hit && !(r.dist <= dist)) ? 1u : 0u;
                    id = lt.id;
                }
            }
        }
        pair_append(hit, &st->n_pairs, cap, [&](unsigned long long at) {
            rows[2 * at] = c.x; rows[2 * at + 1] = perm[c.y];
            o.put(at, id, toi, r);
        });
    }
    group_counters_add<3>(sums, &st->n_tested, &cst->n_evals, &cst->n_unresolved);
}

// ---------------------------------------------------------------- first contact
// face[i] = SWEEP_NONE, toi[i] = +inf and zeros elsewhere for an item no triangle is reported for.  Counters: items with a row, records
// visited, seg_tri evaluations of the walk (which the cut-off lowers; the answer it leaves alone).
__global__ __launch_bounds__(SWEEP_SEGMENT_THREADS) void k_sweep_segments_first(const NodeRec32 *__restrict__ swept, const int32_t *__restrict__ root_name,
                                                                               const LeafTri *__restrict__ leaf, const uint32_t *__restrict__ perm,
                                                                               const double *__restrict__ x0, const double *__restrict__ x1, int n,
                                                                               const uint32_t *__restrict__ sort_flags /* 9 words */, const double *__restrict__ items,
                                                                               const uint32_t *__restrict__ skip /* 2 an item */, unsigned long long np,
                                                                               const CcdState *__restrict__ cst, PointState *__restrict__ st,
                                                                               uint32_t *__restrict__ face, const SweepSegOut o)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const unsigned long long i = (unsigned long long)blockIdx.x * SWEEP_SEGMENT_THREADS + threadIdx.x;
    bool active = i < np;
    const double *it = items + 13 * (active ? i : 0ull);
    BoxFilter<HiTrue> q{};
    double dist = 0.0;
    uint32_t s0 = SWEEP_NONE, s1 = SWEEP_NONE;
    const bool leaf_only = n == 1;                                       // no records: leaf 0 is the whole tree
    if (active) {
        dist = it[12];
        if (skip) { s0 = skip[2 * i]; s1 = skip[2 * i + 1]; }
        if (!leaf_only) q = sweep_segment_filter(it, cst);
    }
    double btoi = __builtin_inf();                                       // the best row so far: the smallest (toi, ID, face index)
    uint32_t bface = SWEEP_NONE, bid = 0u, bleaf = 0u;
    int bstage = 0;
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
            if (seg_skip_passes(s0, s1, lt)) {
                const SweepSegMeshSrc src{x0, x1, it, lt.v0, lt.v1, lt.v2};
                if (seg_gate(src, dist)) {
                    double toi; SegTri r; uint32_t ne; int stage;
                    seg_advance<true>(src, dist, btoi, toi, r, ne, stage);
                    tests += ne;
                    if (toi <= 1.0) {
                        const uint32_t f = perm[k];
                        if (bface == SWEEP_NONE || toi < btoi || (toi == btoi && (lt.id < bid || (lt.id == bid && f < bface)))) {
                            bface = f; bid = lt.id; btoi = toi; bleaf = k; bstage = stage;
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
        SegTri r{};                                                      // (all zero: nothing is reported for this item)
        if (found) {                                                     // the winner's reporting evaluation once more: the same operands, the same bits
            const LeafTri lt = leaf[bleaf];
            SweepSegMeshSrc src{x0, x1, it, lt.v0, lt.v1, lt.v2};
            src.launder();
            r = seg_tri_at(src, bstage, btoi);
        }
        o.put(i, found ? bid : 0u, btoi, r);
    }
    item_counters_add(i < np && bface != SWEEP_NONE, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);
}

// cd_seg_advance_points: seg_advance on explicit positions, n x 13 doubles and n x 18 (the vertices at x0, then at x1)
__global__ __launch_bounds__(CCD_THREADS) void k_seg_advance_points(const double *__restrict__ items, const double *__restrict__ tri, unsigned long long n,
                                                                    const SweepSegOut o, uint32_t *__restrict__ evals)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * CCD_THREADS + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * CCD_THREADS) {
        double t; SegTri r; uint32_t e; int stage;
        seg_advance<false>(SweepSegPointSrc{items + 13 * i, tri + 18 * i}, items[13 * i + 12], 0.0, t, r, e, stage);
        o.put(i, 0u, t, r);
        if (evals) evals[i] = e;
    }
}

}  // namespace cd
