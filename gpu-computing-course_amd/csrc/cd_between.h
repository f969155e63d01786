// cd_between.h -- queries between two meshes: contact, proximity and continuous collision of the triangles of context a against
// those of context b.  Not reference behaviour.  A pair is (a's triangle, b's triangle); every per-pair
// predicate takes a's triangle first; the two vertex arrays are unrelated, so there is no neighbour filter.
//   k_between_mbits   : CCD only.  The largest |coordinate| of a's swept leaf boxes (x0 and x1) into CcdState::m_bits, beside what
//       k_ccd_refit leaves there for b's: M of the CCD pad covers both meshes.
//   k_between_descend : fp32 filter.  One lane per leaf of a (sorted order) walks b's records from b's ROOT (prox_walk,
//       cd_proximity.h, with the cursor of cd_bvh.h started at the root).  Static: b's records read as
//       [lo, prox_hi(hi)], the query box a's FP64 leaf box widened by prox_pad over both root boxes.  Swept: b's swept records (true
//       bounds, k_ccd_links + k_ccd_refit over b), the query box a's swept box widened by ccd_pad.  nb == 1: no records; every leaf of
//       a is a candidate against b's leaf 0 and the exact stage decides.
//   k_between_exact   : FP64, one instance per query kind.  Contact: the strict box test (box.cuh:40-43, counted), then tri_contact.
//       Proximity: tri_distance.  CCD: the swept-box gate, then ccd_advance on a two-mesh source.  Append with one atomic per workgroup
//       and round, as k_prox_exact (the exact stage's scaffold, cd_proximity.h).
// The pads are section 10's and 11's with M over both meshes, so every pair the FP64 definition accepts is a candidate and the FP64
// stage alone decides: the result does not depend on either tree.
#pragma once
#include "cd_ccd.h"

namespace cd {

enum BetweenKind { BW_CONTACT = 0, BW_PROXIMITY = 1, BW_CCD = 2 };

// vertex k of the pair: 0..2 a's triangle (a's x0 / x1), 3..5 b's (b's x0 / x1).  (k is a constant after unrolling.)
struct CcdTwoMeshSrc {
    const double *__restrict__ ax0; const double *__restrict__ ax1; const double *__restrict__ bx0; const double *__restrict__ bx1;
    uint32_t a0, a1, a2, b0, b1, b2;
    __device__ __forceinline__ uint32_t vid(int k) const { return k == 0 ? a0 : (k == 1 ? a1 : (k == 2 ? a2 : (k == 3 ? b0 : (k == 4 ? b1 : b2)))); }
    __device__ __forceinline__ d3 p0(int k) const { return load_vertex(k < 3 ? ax0 : bx0, vid(k)); }
    __device__ __forceinline__ d3 p1(int k) const { return load_vertex(k < 3 ? ax1 : bx1, vid(k)); }
    __device__ __forceinline__ void launder() { asm volatile("" : "+v"(ax0), "+v"(ax1), "+v"(bx0), "+v"(bx1)); }
};

__global__ __launch_bounds__(CCD_THREADS) void k_between_mbits(const LeafTri *__restrict__ leaf, const double *__restrict__ x0, const double *__restrict__ x1,
                                                               int n, CcdState *__restrict__ st)
{
    const uint32_t j = blockIdx.x * CCD_THREADS + threadIdx.x;
    uint32_t mbits = 0u;
    if ((int)j < n) {
        const LeafTri lt = leaf[j];
        const Box b = swept_box(CcdMeshSrc{x0, x1, lt.v0, lt.v1, lt.v2, 0u, 0u, 0u}, 0);
        const double m = fmax2(fmax2(dabs(b.x1), dabs(b.x2)), fmax2(fmax2(dabs(b.y1), dabs(b.y2)), fmax2(dabs(b.z1), dabs(b.z2))));
        mbits = __float_as_uint(__double2float_ru(m)) & 0x7fffffffu;         // (as k_ccd_refit: a leaf of -0.0 coordinates has m = -0.0)
    }
    for (int o = 32; o; o >>= 1) { const uint32_t v = __shfl_xor(mbits, o); mbits = v > mbits ? v : mbits; }   // (non-negative floats: bits order as values)
    if ((threadIdx.x & 63) == 0 && mbits) atomicMax(&st->m_bits, mbits);
}

// SWEPT = false: contact and proximity over b's static records; true: CCD over b's swept records.  root_a / root_b: the FP64 root boxes
// (static pad); ax1: a's x1 (swept).  The sort flags of both contexts are checked as k_prox_descend checks its own.
template <bool SWEPT>
__global__ __launch_bounds__(PROX_DESC_THREADS) void k_between_descend(const NodeRec32 *__restrict__ recs_b, const int32_t *__restrict__ root_name_b, int nb,
                                                                       const LeafTri *__restrict__ leaf_a, const double *__restrict__ ax0,
                                                                       const double *__restrict__ ax1, int na, const double *__restrict__ root_a,
                                                                       const double *__restrict__ root_b, double dist, const uint32_t *__restrict__ flags_a,
                                                                       const uint32_t *__restrict__ flags_b, CcdState *__restrict__ st,
                                                                       uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (sort_failed(flags_a) || sort_failed(flags_b)) return;           // the records are not a tree (the host redoes the build)
    const uint32_t j = blockIdx.x * PROX_DESC_THREADS + threadIdx.x;
    if (nb == 1) {                                                       // no records: leaf 0 is the whole tree
        if ((int)j < na) {
            const uint32_t sh = blockIdx.x & (NSHARD - 1);               // (the workgroup's shard, as prox_walk takes it)
            const unsigned long long at = atomicAdd(&st->shard[sh * PROX_SHARD_STRIDE], 1ull);
            if (at < shard_cap) cand[(size_t)sh * shard_cap + at] = make_uint2(j, 0u);
        }
        return;
    }
    float pad;
    if (SWEPT) pad = ccd_pad(st, dist);
    else {
        const float pa = prox_pad(root_a, dist), pb = prox_pad(root_b, dist);
        pad = pa > pb ? pa : pb;                                         // (prox_pad is monotonic in M: the pad of the larger M)
    }
    bool active = (int)j < na;
    QueryBox32 q{};
    RecCursor w{};
    if (active) {
        const LeafTri lt = leaf_a[j];
        q = query_box32(SWEPT ? swept_box(CcdMeshSrc{ax0, ax1, lt.v0, lt.v1, lt.v2, 0u, 0u, 0u}, 0)
                              : box_set(load_vertex(ax0, lt.v0), load_vertex(ax0, lt.v1), load_vertex(ax0, lt.v2)), pad);
        active = w.start_root(recs_b, nb, (uint32_t)*root_name_b);
    }
    if (SWEPT) prox_walk(recs_b, nb, j, active, w, BoxFilter<HiTrue>{q}, st->shard, cand, shard_cap);
    else prox_walk(recs_b, nb, j, active, w, BoxFilter<HiNextUp>{q}, st->shard, cand, shard_cap);
}

template <int KIND, bool WIT>                          // (WIT, the witness calls: wleaf[at] = (leaf of a, leaf of b) of the hit, as k_prox_exact)
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_between_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap,
                                                                     const LeafTri *__restrict__ leaf_a, const double *__restrict__ ax0, const double *__restrict__ ax1,
                                                                     const LeafTri *__restrict__ leaf_b, const double *__restrict__ bx0, const double *__restrict__ bx1,
                                                                     double dist, CcdState *__restrict__ st, uint32_t *__restrict__ pairs,
                                                                     double *__restrict__ toi_out, double *__restrict__ dists, unsigned long long cap,
                                                                     uint2 *__restrict__ wleaf)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long sums[3] = {0, 0, 0};                              // tested, evals, unresolved: CcdState's order
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        bool hit = false;
        uint32_t ida = 0, idb = 0; double toi = 0.0, d = 0.0;
        uint2 lv = make_uint2(0u, 0u);
        if (i < sl.total) {
            const uint2 c = sl.list[i];
            const LeafTri A = leaf_a[c.x], B = leaf_b[c.y];
            lv = c;
            ida = A.id; idb = B.id;
            if (KIND == BW_CONTACT) {
                const d3 P1 = load_vertex(ax0, A.v0), P2 = load_vertex(ax0, A.v1), P3 = load_vertex(ax0, A.v2);
                const d3 Q1 = load_vertex(bx0, B.v0), Q2 = load_vertex(bx0, B.v1), Q3 = load_vertex(bx0, B.v2);
                if (box_overlap(box_set(P1, P2, P3), box_set(Q1, Q2, Q3))) {                  // box.cuh:40-43
                    ++sums[0];
                    hit = tri_contact_fast(P1, P2, P3, Q1, Q2, Q3);                           // tri_contact.cuh:19-78, a's triangle as P
                }
            } else if (KIND == BW_PROXIMITY) {
                ++sums[0];
                d = tri_distance(load_vertex(ax0, A.v0), load_vertex(ax0, A.v1), load_vertex(ax0, A.v2),
                                 load_vertex(bx0, B.v0), load_vertex(bx0, B.v1), load_vertex(bx0, B.v2));
                hit = d <= dist;
            } else {
                const CcdTwoMeshSrc src{ax0, ax1, bx0, bx1, A.v0, A.v1, A.v2, B.v0, B.v1, B.v2};
                if (ccd_gate(src, dist)) {
                    ++sums[0];
                    uint32_t ne = 0;
                    ccd_advance(src, dist, toi, d, ne);
                    sums[1] += ne;
                    hit = toi <= 1.0;
                    sums[2] += (hit && !(d <= dist)) ? 1u : 0u;
                }
            }
        }
        pair_append(hit, &st->n_pairs, cap, [&](unsigned long long at) {
            pairs[2 * at] = ida; pairs[2 * at + 1] = idb;
            if (KIND == BW_PROXIMITY) dists[at] = d;
            if (KIND == BW_CCD) { toi_out[at] = toi; dists[at] = d; }
            if (WIT) wleaf[at] = lv;
        });
    }
    group_counters_add<KIND == BW_CCD ? 3 : 1>(sums, &st->n_tested, &st->n_evals, &st->n_unresolved);     // (only CCD counts evaluations and unresolved pairs)
}

}  // namespace cd
