// cd_witness.h -- where the pair queries' distance is attained: the closest points of the pairs cd_find_proximity, cd_find_ccd and
// their between-mesh forms report (cd_find_*_witness).  Not reference behaviour.  The per-pair function is
// tri_witness (cd_math.h).
//   The exact stages (k_prox_exact, k_ccd_exact, k_between_exact) have a WIT instance that notes the two leaf positions of every hit, A's
//       first, beside the pair it appends (wleaf[at]): tri_distance's loop in the candidate pass stays as it is (188 VGPRs already).
//   k_pair_witness : one lane per REPORTED pair (a small fraction of the candidates), for all four calls.  A's triangle from
//       (leaf_a, ax0 / ax1), B's from (leaf_b, bx0 / bx1) -- the self calls pass their own mesh twice.  toi == NULL: the positions are
//       x0 (proximity).  Else row k is evaluated where the advancement reported it: x1 itself when toi[k] == 1, otherwise
//       a + toi (b - a) per coordinate as ccd_at writes it (x0's values at toi == 0).  faces: perm[] of the two leaves, the indices in
//       cd_create's face list.  Every output may be NULL.  A row whose leaf of A is WITNESS_NO_PAIR gets zeros.
//   k_tri_witness_points : tri_witness on explicit positions (cd_tri_witness_points): the pin of the device code.
#pragma once
#include "cd_between.h"

namespace cd {

constexpr int WITNESS_THREADS = 256;
constexpr uint32_t WITNESS_NO_PAIR = 0xffffffffu;     // in wleaf[k].x: row k has no pair (only the nearest queries leave such rows)

// every output may be NULL
__device__ __forceinline__ void witness_store(const TriWitness &w, unsigned long long k, double *__restrict__ points, double *__restrict__ bary,
                                              uint8_t *__restrict__ feature)
{
    if (points) {
        double *p = points + 6 * k;
        p[0] = w.qa.x; p[1] = w.qa.y; p[2] = w.qa.z; p[3] = w.qb.x; p[4] = w.qb.y; p[5] = w.qb.z;
    }
    if (bary) { double *b = bary + 4 * k; b[0] = w.ua; b[1] = w.va; b[2] = w.ub; b[3] = w.vb; }
    if (feature) { feature[2 * k] = (uint8_t)w.fa; feature[2 * k + 1] = (uint8_t)w.fb; }
}

// vertex v where row k is evaluated (MOVING: t is the row's toi)
template <bool MOVING>
__device__ __forceinline__ d3 witness_vertex(const double *__restrict__ x0, const double *__restrict__ x1, uint32_t v, double t)
{
    const d3 a = load_vertex(x0, v);
    if (!MOVING) return a;
    const d3 b = load_vertex(x1, v);
    if (t == 1.0) return b;
    return d3{a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z)};
}

template <bool MOVING>
__global__ __launch_bounds__(WITNESS_THREADS) void k_pair_witness(const uint2 *__restrict__ wleaf, unsigned long long n,
                                                                 const LeafTri *__restrict__ leaf_a, const uint32_t *__restrict__ perm_a,
                                                                 const double *__restrict__ ax0, const double *__restrict__ ax1,
                                                                 const LeafTri *__restrict__ leaf_b, const uint32_t *__restrict__ perm_b,
                                                                 const double *__restrict__ bx0, const double *__restrict__ bx1,
                                                                 const double *__restrict__ toi, uint32_t *__restrict__ faces,
                                                                 double *__restrict__ points, double *__restrict__ bary, uint8_t *__restrict__ feature)
{
    const unsigned long long k = (unsigned long long)blockIdx.x * WITNESS_THREADS + threadIdx.x;
    if (k >= n) return;
    const uint2 l = wleaf[k];
    if (l.x == WITNESS_NO_PAIR) {                                        // cd_nearest_between's "nothing" row: no leaves, feature 0 / 0 and zeros
        if (faces) { faces[2 * k] = WITNESS_NO_PAIR; faces[2 * k + 1] = WITNESS_NO_PAIR; }
        witness_store(TriWitness{}, k, points, bary, feature);
        return;
    }
    if (faces) { faces[2 * k] = perm_a[l.x]; faces[2 * k + 1] = perm_b[l.y]; }
    if (!points && !bary && !feature) return;
    const LeafTri A = leaf_a[l.x], B = leaf_b[l.y];
    const double t = MOVING ? toi[k] : 0.0;
    const TriWitness w = tri_witness(witness_vertex<MOVING>(ax0, ax1, A.v0, t), witness_vertex<MOVING>(ax0, ax1, A.v1, t), witness_vertex<MOVING>(ax0, ax1, A.v2, t),
                                     witness_vertex<MOVING>(bx0, bx1, B.v0, t), witness_vertex<MOVING>(bx0, bx1, B.v1, t), witness_vertex<MOVING>(bx0, bx1, B.v2, t));
    witness_store(w, k, points, bary, feature);
}

// cd_tri_witness_points: tri_witness on explicit positions, n x 18 doubles (A's three vertices, then B's)
__global__ __launch_bounds__(WITNESS_THREADS) void k_tri_witness_points(const double *__restrict__ tri, unsigned long long n, double *__restrict__ dist,
                                                                       double *__restrict__ points, double *__restrict__ bary, uint8_t *__restrict__ feature)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * WITNESS_THREADS + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * WITNESS_THREADS) {
        const double *t = tri + 18 * i;
        const TriWitness w = tri_witness(d3{t[0], t[1], t[2]}, d3{t[3], t[4], t[5]}, d3{t[6], t[7], t[8]},
                                         d3{t[9], t[10], t[11]}, d3{t[12], t[13], t[14]}, d3{t[15], t[16], t[17]});
        dist[i] = w.dist;
        witness_store(w, i, points, bary, feature);
    }
}

}  // namespace cd
