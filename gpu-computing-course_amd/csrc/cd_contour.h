// cd_contour.h -- where the pairs in contact cut each other: the intersection segment of every pair cd_find_collisions_contour and
// cd_find_collisions_between_contour report.  Not reference behaviour.  The per-pair function is tri_isect
// (cd_math.h).  The collision path's own kernels (k_descend_half, k_exact) are not involved: the self call is a pass of its own behind
// the tree, shaped like the proximity pass.
//   Self call: k_prox_descend (cd_proximity.h) with dist = 0 -- the fp32 boxes are outer bounds, widened by M 2^-20, and boxes that touch
//       count, so every pair of leaves whose FP64 boxes overlap strictly is a candidate -- then
//   k_contour_exact : FP64, on the exact stage's scaffold (ShardSlice, pair_append, group_counters_add).  The contact definition of the
//       collision path by leaf pair: neighbour filter (collision.cuh:38), different IDs (tri_contact.cuh:81 lets no equal-ID pair through
//       in either direction), strict box overlap (box.cuh:40-43), then -- counted as tested -- tri_contact with the smaller ID's triangle
//       as P (the order k_exact swaps to).  Appends (smaller ID, larger ID) and, when wleaf is not NULL, the two leaf positions, A's first.
//   Between call: k_between_exact<BW_CONTACT, true> (cd_between.h), which notes (leaf of a, leaf of b).
//   k_pair_contour : one lane per REPORTED pair, for both calls, as k_pair_witness: faces from perm[], the rest tri_isect(A, B).  Every
//       output may be NULL.
//   k_tri_isect_points : tri_isect on explicit positions (cd_tri_isect_points): the pin of the device code.
#pragma once
#include "cd_between.h"

namespace cd {

constexpr int CONTOUR_THREADS = 256;

// code: 3 bytes a row (endpoint 0 and 1 as term | side << 3, 7 = missing; the mask); param: t u v of endpoint 0, then of 1; points: x of
// endpoint 0, then of 1.  Every output may be NULL.
__device__ __forceinline__ void contour_store(const TriIsect &w, unsigned long long k, uint8_t *__restrict__ code, double *__restrict__ param,
                                              double *__restrict__ points)
{
    if (code) {
        code[3 * k] = (uint8_t)(w.e[0].term | w.e[0].side << 3); code[3 * k + 1] = (uint8_t)(w.e[1].term | w.e[1].side << 3);
        code[3 * k + 2] = (uint8_t)w.mask;
    }
    if (param) { double *p = param + 6 * k; p[0] = w.e[0].t; p[1] = w.e[0].u; p[2] = w.e[0].v; p[3] = w.e[1].t; p[4] = w.e[1].u; p[5] = w.e[1].v; }
    if (points) {
        double *p = points + 6 * k;
        p[0] = w.e[0].x.x; p[1] = w.e[0].x.y; p[2] = w.e[0].x.z; p[3] = w.e[1].x.x; p[4] = w.e[1].x.y; p[5] = w.e[1].x.z;
    }
}

__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_contour_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                     const double *__restrict__ verts, ProxState *__restrict__ st, uint32_t *__restrict__ pairs,
                                                                     unsigned long long cap, uint2 *__restrict__ wleaf /* NULL: the pairs only */)
{
    const ShardSlice sl(st->shard, cand, shard_cap);
    unsigned long long tested = 0;
    for (unsigned long long b0 = sl.first(); b0 < sl.total; b0 += sl.stride()) {
        const unsigned long long i = b0 + threadIdx.x;
        bool hit = false;
        uint32_t ida = 0, idb = 0;
        uint2 lv = make_uint2(0u, 0u);
        if (i < sl.total) {
            const uint2 c = sl.list[i];
            LeafTri A = leaf[c.x], B = leaf[c.y];
            lv = c;
            if (neighbor_count(A.v0, A.v1, A.v2, B.v0, B.v1, B.v2) < 1 && A.id != B.id) {    // collision.cuh:38, tri_contact.cuh:81
                if (B.id < A.id) { const LeafTri t = A; A = B; B = t; lv = make_uint2(c.y, c.x); }   // A: the smaller ID, in front as k_exact puts it
                const d3 P1 = load_vertex(verts, A.v0), P2 = load_vertex(verts, A.v1), P3 = load_vertex(verts, A.v2);
                const d3 Q1 = load_vertex(verts, B.v0), Q2 = load_vertex(verts, B.v1), Q3 = load_vertex(verts, B.v2);
                if (box_overlap(box_set(P1, P2, P3), box_set(Q1, Q2, Q3))) {                 // box.cuh:40-43
                    ++tested;
                    hit = tri_contact_fast(P1, P2, P3, Q1, Q2, Q3);                          // tri_contact.cuh:19-78
                }
                ida = A.id; idb = B.id;
            }
        }
        pair_append(hit, &st->n_pairs, cap, [&](unsigned long long at) { pairs[2 * at] = ida; pairs[2 * at + 1] = idb; if (wleaf) wleaf[at] = lv; });
    }
    group_counters_add<1>(&tested, &st->n_tested);
}

__global__ __launch_bounds__(CONTOUR_THREADS) void k_pair_contour(const uint2 *__restrict__ wleaf, unsigned long long n,
                                                                 const LeafTri *__restrict__ leaf_a, const uint32_t *__restrict__ perm_a, const double *__restrict__ ax0,
                                                                 const LeafTri *__restrict__ leaf_b, const uint32_t *__restrict__ perm_b, const double *__restrict__ bx0,
                                                                 uint32_t *__restrict__ faces, uint8_t *__restrict__ code, double *__restrict__ param,
                                                                 double *__restrict__ points)
{
    const unsigned long long k = (unsigned long long)blockIdx.x * CONTOUR_THREADS + threadIdx.x;
    if (k >= n) return;
    const uint2 l = wleaf[k];
    if (faces) { faces[2 * k] = perm_a[l.x]; faces[2 * k + 1] = perm_b[l.y]; }
    if (!code && !param && !points) return;
    const LeafTri A = leaf_a[l.x], B = leaf_b[l.y];
    const TriIsect w = tri_isect(load_vertex(ax0, A.v0), load_vertex(ax0, A.v1), load_vertex(ax0, A.v2),
                                 load_vertex(bx0, B.v0), load_vertex(bx0, B.v1), load_vertex(bx0, B.v2));
    contour_store(w, k, code, param, points);
}

// cd_tri_isect_points: tri_isect on explicit positions, n x 18 doubles (A's three vertices, then B's)
__global__ __launch_bounds__(CONTOUR_THREADS) void k_tri_isect_points(const double *__restrict__ tri, unsigned long long n, uint8_t *__restrict__ code,
                                                                     double *__restrict__ param, double *__restrict__ points)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * CONTOUR_THREADS + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * CONTOUR_THREADS) {
        const double *t = tri + 18 * i;
        const TriIsect w = tri_isect(d3{t[0], t[1], t[2]}, d3{t[3], t[4], t[5]}, d3{t[6], t[7], t[8]},
                                     d3{t[9], t[10], t[11]}, d3{t[12], t[13], t[14]}, d3{t[15], t[16], t[17]});
        contour_store(w, i, code, param, points);
    }
}

}  // namespace cd
