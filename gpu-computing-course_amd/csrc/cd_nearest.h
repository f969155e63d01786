// cd_nearest.h -- nearest-triangle and separation-distance queries between two meshes: for every triangle of context a the nearest
// triangle of context b, and the nearest pair of all.  Not reference behaviour.  The self form -- one mesh against
// itself, k_nearest_self -- is below, before k_nearest_min.  The per-pair predicate is
// tri_distance (cd_math.h), a's triangle first; the witness is k_pair_witness's (cd_witness.h) over the leaf pairs left here.
//   k_nearest_between<MIN> : one lane per leaf of a in a's SORTED order (neighbours in a wave are neighbours in space); the row is
//       written at perm_a[j], the triangle's index in cd_create's face list.  The lane walks b's records as k_closest_points walks
//       them for a point (cd_points.h), with A's FP64 box in the point's place:
//       SEED   a greedy descent from b's root to the child whose box is nearer to A's box, ties to the left, down to a leaf, whose
//              triangle gives the first candidate and the first bound  best = min(rmax, dist);
//       WALK   RecCursor's stackless pre-order walk from the ROOT (cd_bvh.h: its guards and its 2 n step rule): a subtree is entered
//              when its box's lower-bound distance to A's box does not exceed the bound, CLOSED, so that a triangle at the same
//              distance with a smaller ID is still seen.
//       tri_distance is the rolled 33-term loop and costs ~190 VGPRs: inside a walking lane it would run with one lane of the wave
//       at a time.  The loop therefore has two halves: every lane walks until it HOLDS A PENDING LEAF or is done, then the wave
//       evaluates all pending leaves in one pass of the ONE inline site of tri_distance.  A lane that holds a leaf has already moved
//       its cursor on (the next subtree in pre-order does not depend on the bound); the bound shrinks before the next box is tested.
//       Of the triangles with dist <= rmax (tested on dist itself, never on the squares) the smallest (dist, ID of B, face of B) wins.
//       nb == 1 has no records: the lane tests leaf 0 and is done.
//       MIN (the separation distance): the lanes of the whole grid share one 64-bit word, the bits of the smallest distance any lane
//       has evaluated (non-negative doubles order as unsigned integers; the host starts it at rmax; atomicMin).  A lane prunes
//       against  min(own best, word), CLOSED: the word never drops below the final minimum, so every pair AT the final minimum is
//       still entered and evaluated by its lane, and that lane's lexicographic best among the pairs it saw is its true row.  Rows
//       of lanes whose nearest triangle is farther than the final minimum may be anything not below it (or nothing): k_nearest_min
//       takes the minimum, which they cannot win.  The word is read once before the seed and once after every evaluation pass; how
//       often is a tuning choice -- a stale (larger) value only prunes less.
//   k_nearest_min : one workgroup; the na rows reduced to the one row with the smallest (dist, ID a, face a, ID b, face b).  The face
//       of a is unique per row, so the order is total and the result does not depend on how the rows are dealt to the threads.
//       When the walks are done the shared word IS the smallest distance of any row, so a row is a candidate only at that distance.
//   The filter only filters.  The query is A's FP64 box [loA, hiA] (box_set of its three vertices); a stored box is read as
//       [lo, prox_hi(hi)] (converted exactly); per axis the gap  g = max((lo - pad) - hiA, (loA - hi) - pad, 0)  with
//       pad = 2^-20 max(M_a, M_b), M the largest |coordinate| of a root box; a subtree is skipped only when
//       (g_x^2 + g_y^2) + g_z^2 > bound^2.  The padded gap vector is no longer than the true distance between the boxes minus pad, the
//       true distance between A and any triangle of the subtree is no shorter than that between their boxes, tri_distance is below the
//       true distance by at most a few 2^-52 M = 2^-30 pad, and the roundings of the gaps and squares are relative 2^-52: the pad
//       covers all of it (the proof: DESIGN.md section 18).  A pair in contact (dist = 0) has strictly overlapping FP64 boxes, hence
//       gap 0 on every axis, and 0 > bound^2 never holds.  The comparison is written so that a NaN enters, never culls; an overflowing
//       bound^2 is +inf and culls nothing.
#pragma once
#include "cd_points.h"
#include "cd_witness.h"

namespace cd {

constexpr int NEAREST_THREADS = 64;
constexpr int NEAREST_MIN_THREADS = 256;
constexpr uint32_t NEAREST_NONE = 0xffffffffu;
// min_bits: the MIN instance's shared bound (the bits of a non-negative double)
struct alignas(64) NearestState { unsigned long long n_found, node_visits, tri_tests, min_bits, pad[4]; };
static_assert(sizeof(NearestState) == 64, "one 64-byte counter record");

// the squared lower-bound distance from A's box to the padded box  (h0, h1: a record half, lo = h0.xyz, hi = (h0.w, h1.x, h1.y))
__device__ __forceinline__ double box_box2(const float4 h0, const float4 h1, const Box &a, const double pad)
{
#define CD_NB_AXIS(LO, HI, ALO, AHI) fmax2(fmax2(((double)(LO) - pad) - (AHI), ((ALO) - (double)prox_hi(HI)) - pad), 0.0)
    const double gx = CD_NB_AXIS(h0.x, h0.w, a.x1, a.x2), gy = CD_NB_AXIS(h0.y, h1.x, a.y1, a.y2), gz = CD_NB_AXIS(h0.z, h1.y, a.z1, a.z2);
#undef CD_NB_AXIS
    return (gx * gx + gy * gy) + gz * gz;
}

template <bool MIN>
__global__ __launch_bounds__(NEAREST_THREADS) void k_nearest_between(const NodeRec32 *__restrict__ recs_b, const int32_t *__restrict__ root_name_b,
                                                                     const LeafTri *__restrict__ leaf_b, const uint32_t *__restrict__ perm_b,
                                                                     const double *__restrict__ bverts, const double *__restrict__ root_b, int nb,
                                                                     const LeafTri *__restrict__ leaf_a, const uint32_t *__restrict__ perm_a,
                                                                     const double *__restrict__ averts, const double *__restrict__ root_a, int na,
                                                                     double rmax, NearestState *__restrict__ st, uint32_t *__restrict__ faces,
                                                                     uint32_t *__restrict__ ids, double *__restrict__ dist, uint2 *__restrict__ wleaf)
{
    enum { SEED = 0, WALK = 1, DONE = 2 };
    const uint32_t j = blockIdx.x * NEAREST_THREADS + threadIdx.x;
    const bool mine = (int)j < na;
    LeafTri A{};
    Box abox{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (mine) {
        A = leaf_a[j];
        abox = box_set(load_vertex(averts, A.v0), load_vertex(averts, A.v1), load_vertex(averts, A.v2));
    }
    const double pad = fmax2(root_max_abs(root_a), root_max_abs(root_b)) * PROX_SLACK;
    double best = rmax;                                                  // own bound: min(rmax, the best candidate's dist)
    double bound = best;                                                 // MIN: min(best, the shared word); else best
    if (MIN) bound = fmin2(bound, __longlong_as_double((long long)st->min_bits));
    double bound2 = bound * bound;
    uint32_t bleaf = NEAREST_NONE, bface = NEAREST_NONE, bid = 0u;
    uint32_t visits = 0, tests = 0;
    RecCursor w{}, seed{};                                               // the WALK's cursor; of `seed` only the step count is used (SEED's moves)
    uint32_t root = 0, cur = 0;
    const bool leaf_only = nb == 1;                                      // no records: leaf 0 is the whole tree
    int mode = mine ? SEED : DONE;
    if (mine && !leaf_only) {
        root = (uint32_t)*root_name_b;
        cur = root;
        if (!rec_internal((int32_t)root, nb)) mode = DONE;               // (no tree: nothing is read; nothing is found)
    }
    bool pending = false;
    uint32_t k = 0;
    if (mine && leaf_only) { pending = true; mode = DONE; }              // (k = 0)
    while (mode != DONE || pending) {
        // every lane walks until it holds a pending leaf or is done
        while (mode != DONE && !pending) {
            if (mode == SEED) {                                          // the nearer child of `cur`, ties to the left
                RecCursor l, r;
                l.at_left(recs_b, nb, cur); r.at_right(recs_b, nb, cur);
                visits += 2;
                if (box_box2(r.h0, r.h1, abox, pad) < box_box2(l.h0, l.h1, abox, pad)) l = r;
                if (l.internal(nb)) {
                    cur = (uint32_t)l.link();
                    if (!seed.count(nb)) mode = DONE;                    // (the descent's own moves, up to n - 1, under the walk's rule)
                    continue;
                }
                if (l.leaf(nb)) { pending = true; k = l.leaf_index(); }
                mode = WALK;                                             // the walk starts at the root, with 2 n moves of its own
                w.start_root(recs_b, nb, root);                          // (true: the root was checked before the loop)
            } else {
                ++visits;
                const bool enter = !(box_box2(w.h0, w.h1, abox, pad) > bound2);   // CLOSED; a NaN enters
                if (enter && w.internal(nb)) {
                    if (!w.descend(recs_b, nb)) mode = DONE;
                    continue;
                }
                if (enter && w.leaf(nb)) { pending = true; k = w.leaf_index(); }
                if (!w.next(recs_b, nb)) mode = DONE;                    // (the cursor moves on before the leaf is evaluated: its path does not depend on the bound)
            }
        }
        // the wave evaluates all pending leaves in one pass
        if (pending) {
            pending = false;
            ++tests;
            const LeafTri B = leaf_b[k];
            const double d = tri_distance(load_vertex(averts, A.v0), load_vertex(averts, A.v1), load_vertex(averts, A.v2),
                                          load_vertex(bverts, B.v0), load_vertex(bverts, B.v1), load_vertex(bverts, B.v2));
            if (d <= rmax) {
                const uint32_t f = perm_b[k];
                // the smallest (dist, ID, face index)
                if (bface == NEAREST_NONE || d < best || (d == best && (B.id < bid || (B.id == bid && f < bface)))) {
                    bleaf = k; bface = f; bid = B.id; best = d;
                    if (MIN) atomicMin(&st->min_bits, (unsigned long long)__double_as_longlong(d));
                }
            }
            bound = best;
            if (MIN) bound = fmin2(bound, __longlong_as_double((long long)__hip_atomic_load(&st->min_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
            bound2 = bound * bound;
        }
    }
    const bool found = bface != NEAREST_NONE;
    if (mine) {
        const uint32_t i = perm_a[j];
        faces[2 * (size_t)i] = found ? i : NEAREST_NONE; faces[2 * (size_t)i + 1] = bface;
        ids[2 * (size_t)i] = found ? A.id : 0u; ids[2 * (size_t)i + 1] = found ? bid : 0u;
        dist[i] = found ? best : __builtin_inf();
        wleaf[i] = make_uint2(found ? j : NEAREST_NONE, bleaf);
    }
    item_counters_add(mine && found, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);
}

// ---- the self form: the nearest non-neighbouring triangle of the SAME mesh (cd_nearest_self) ----------------------
//   k_nearest_self<MIN> : k_nearest_between with one tree on both sides -- the same box_box2 and pad (both roots are the one root), the
//       same two-halved loop around the ONE inline site of tri_distance, the same acceptance on d <= rmax, the same shared word.  What
//       differs:
//       EXCLUSION  a leaf the walk enters is tested BEFORE it becomes pending: leaf j itself and every leaf that shares a vertex index
//              with j (neighbor_count >= 1, cd_find_proximity's rule) are passed over.  That costs one LeafTri load in the walk and
//              saves the wave-wide evaluation pass; an excluded leaf is not an evaluation.
//       ORDER  tri_distance(A, B) and tri_distance(B, A) differ in their last bits, so the two triangles are swapped into
//              k_prox_exact's order before the call: A is the one with the smaller (ID, face index).  Both rows that hold a pair hold
//              the same bits, cd_find_proximity's.  wleaf keeps the PLAYED order, so that k_pair_witness evaluates the same call.
//       SEED   a greedy descent of the own tree ends at leaf j.  The first bound comes from an ADMISSIBLE leaf near j in Morton order
//              instead: of j + 1, j - 1, j + 2, ... up to NEAREST_SELF_SEED steps each side, the admissible leaf whose FP64 box is
//              nearest to A's (the first of equals; the first admissible leaf alone is a poor seed where the Morton curve jumps:
//              DESIGN.md section 21 has the counts); none found: no seed, the bound stays rmax.  The seed only tightens the bound (it
//              is a candidate like any other; the walk passes over it when it meets it again), so the rows do not depend on it.
//       n == 1 has no partner and no records: nothing is read.  n == 2 is one record, two leaf children.
#ifndef CD_NEAREST_SELF_SEED
#define CD_NEAREST_SELF_SEED 16                       // (0: the no-seed build of the seed decision)
#endif
constexpr uint32_t NEAREST_SELF_SEED = CD_NEAREST_SELF_SEED;

// the squared distance between two FP64 boxes (0 when they meet): the seed's choice only, never a filter
__device__ __forceinline__ double box_gap2(const Box &a, const Box &b)
{
    const double gx = fmax2(fmax2(b.x1 - a.x2, a.x1 - b.x2), 0.0), gy = fmax2(fmax2(b.y1 - a.y2, a.y1 - b.y2), 0.0), gz = fmax2(fmax2(b.z1 - a.z2, a.z1 - b.z2), 0.0);
    return (gx * gx + gy * gy) + gz * gz;
}

template <bool MIN>
__global__ __launch_bounds__(NEAREST_THREADS) void k_nearest_self(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name,
                                                                  const LeafTri *__restrict__ leaf, const uint32_t *__restrict__ perm,
                                                                  const double *__restrict__ verts, const double *__restrict__ root_box, int n,
                                                                  double rmax, NearestState *__restrict__ st, uint32_t *__restrict__ faces,
                                                                  uint32_t *__restrict__ ids, double *__restrict__ dist, uint2 *__restrict__ wleaf)
{
    const uint32_t j = blockIdx.x * NEAREST_THREADS + threadIdx.x;
    const bool mine = (int)j < n;
    LeafTri A{};
    Box abox{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t own = 0;                                                    // the row: leaf j's index in cd_create's face list
    if (mine) {
        A = leaf[j];
        own = perm[j];
        abox = box_set(load_vertex(verts, A.v0), load_vertex(verts, A.v1), load_vertex(verts, A.v2));
    }
    const double pad = root_max_abs(root_box) * PROX_SLACK;
    double best = rmax;                                                  // own bound: min(rmax, the best candidate's dist)
    double bound = best;                                                 // MIN: min(best, the shared word); else best
    if (MIN) bound = fmin2(bound, __longlong_as_double((long long)st->min_bits));
    double bound2 = bound * bound;
    uint32_t bleaf = NEAREST_NONE, bface = NEAREST_NONE, bid = 0u;
    uint32_t visits = 0, tests = 0;
    RecCursor w{};
    bool walking = mine && n > 1;                                        // (n == 1: no partner, no records)
    if (walking) walking = w.start_root(recs, n, (uint32_t)*root_name);  // (no tree: nothing is read; nothing is found)
    // SEED: of the admissible leaves j + 1, j - 1, j + 2, ... the one whose box is nearest to A's (the first of equals)
    uint32_t seeded = NEAREST_NONE;                                      // the seed's leaf, not evaluated a second time
    if (walking) {
        double near2 = 0.0;
        for (uint32_t step = 0; step < 2u * NEAREST_SELF_SEED; ++step) {
            const uint32_t off = (step >> 1) + 1u;
            const bool up = !(step & 1u);
            if (up ? off >= (uint32_t)n - j : off > j) continue;
            const uint32_t c = up ? j + off : j - off;
            const LeafTri S = leaf[c];
            if (neighbor_count(A.v0, A.v1, A.v2, S.v0, S.v1, S.v2) >= 1) continue;
            const double g2 = box_gap2(abox, box_set(load_vertex(verts, S.v0), load_vertex(verts, S.v1), load_vertex(verts, S.v2)));
            if (seeded == NEAREST_NONE || g2 < near2) { seeded = c; near2 = g2; }
        }
    }
    bool pending = seeded != NEAREST_NONE;
    uint32_t k = seeded;
    while (walking || pending) {
        // every lane walks until it holds a pending leaf or is done
        while (walking && !pending) {
            ++visits;
            const bool enter = !(box_box2(w.h0, w.h1, abox, pad) > bound2);   // CLOSED; a NaN enters
            if (enter && w.internal(n)) {
                walking = w.descend(recs, n);
                continue;
            }
            if (enter && w.leaf(n)) {
                k = w.leaf_index();
                if (k != j && k != seeded) {                             // the exclusions, before the leaf becomes pending
                    const LeafTri B = leaf[k];
                    pending = neighbor_count(A.v0, A.v1, A.v2, B.v0, B.v1, B.v2) < 1;   // collision.cuh:38
                }
            }
            walking = w.next(recs, n);                                   // (the cursor moves on before the leaf is evaluated: its path does not depend on the bound)
        }
        // the wave evaluates all pending leaves in one pass
        if (pending) {
            pending = false;
            ++tests;
            const LeafTri B = leaf[k];
            const uint32_t f = perm[k];
            const bool swap = B.id < A.id || (B.id == A.id && f < own);  // A: the smaller ID (then face index), as k_prox_exact
            const LeafTri P = swap ? B : A, Q = swap ? A : B;
            const double d = tri_distance(load_vertex(verts, P.v0), load_vertex(verts, P.v1), load_vertex(verts, P.v2),
                                          load_vertex(verts, Q.v0), load_vertex(verts, Q.v1), load_vertex(verts, Q.v2));
            if (d <= rmax) {
                // the smallest (dist, ID, face index)
                if (bface == NEAREST_NONE || d < best || (d == best && (B.id < bid || (B.id == bid && f < bface)))) {
                    bleaf = k; bface = f; bid = B.id; best = d;
                    if (MIN) atomicMin(&st->min_bits, (unsigned long long)__double_as_longlong(d));
                }
            }
            bound = best;
            if (MIN) bound = fmin2(bound, __longlong_as_double((long long)__hip_atomic_load(&st->min_bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
            bound2 = bound * bound;
        }
    }
    const bool found = bface != NEAREST_NONE;
    if (mine) {
        const bool swap = found && (bid < A.id || (bid == A.id && bface < own));
        faces[2 * (size_t)own] = found ? own : NEAREST_NONE; faces[2 * (size_t)own + 1] = bface;
        ids[2 * (size_t)own] = found ? A.id : 0u; ids[2 * (size_t)own + 1] = found ? bid : 0u;
        dist[own] = found ? best : __builtin_inf();
        wleaf[own] = found ? (swap ? make_uint2(bleaf, j) : make_uint2(j, bleaf)) : make_uint2(NEAREST_NONE, NEAREST_NONE);   // the played order
    }
    item_counters_add(mine && found, visits, tests, &st->n_found, &st->node_visits, &st->tri_tests);
}

// a row's five keys: (dist, ID a, face a, ID b, face b); a "nothing" row (dist = +inf, faces 0xFFFFFFFF) loses against every found row
struct NearestKey { double d; uint32_t ida, fa, idb, fb; uint2 leaf; };
__device__ __forceinline__ bool nearest_less(const NearestKey &x, const NearestKey &y)
{
    if (x.fa == NEAREST_NONE || y.fa == NEAREST_NONE) return x.fa != NEAREST_NONE;
    if (x.d != y.d) return x.d < y.d;
    if (x.ida != y.ida) return x.ida < y.ida;
    if (x.fa != y.fa) return x.fa < y.fa;
    if (x.idb != y.idb) return x.idb < y.idb;
    return x.fb < y.fb;
}

// the na rows -> row `out` (one workgroup)
__global__ __launch_bounds__(NEAREST_MIN_THREADS) void k_nearest_min(unsigned long long na, unsigned long long out, NearestState *__restrict__ st,
                                                                      uint32_t *__restrict__ faces, uint32_t *__restrict__ ids,
                                                                      double *__restrict__ dist, uint2 *__restrict__ wleaf)
{
    __shared__ NearestKey sh[NEAREST_MIN_THREADS];
    NearestKey m{__builtin_inf(), 0u, NEAREST_NONE, 0u, NEAREST_NONE, make_uint2(NEAREST_NONE, NEAREST_NONE)};
    // the shared word is final here: the smallest distance any row holds (rmax when no row holds one).  Only rows AT it can win, so
    // the other four keys are read for those alone.
    const double dmin = __longlong_as_double((long long)st->min_bits);
    for (unsigned long long i = threadIdx.x; i < na; i += NEAREST_MIN_THREADS) {
        if (!(dist[i] <= dmin)) continue;
        const NearestKey r{dist[i], ids[2 * i], faces[2 * i], ids[2 * i + 1], faces[2 * i + 1], wleaf[i]};
        if (nearest_less(r, m)) m = r;
    }
    sh[threadIdx.x] = m;
    __syncthreads();
    for (int o = NEAREST_MIN_THREADS / 2; o; o >>= 1) {
        if ((int)threadIdx.x < o && nearest_less(sh[threadIdx.x + o], sh[threadIdx.x])) sh[threadIdx.x] = sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        m = sh[0];
        faces[2 * out] = m.fa; faces[2 * out + 1] = m.fb;
        ids[2 * out] = m.ida; ids[2 * out + 1] = m.idb;
        dist[out] = m.d;
        wleaf[out] = m.leaf;
        st->n_found = m.fa != NEAREST_NONE ? 1ull : 0ull;                // (the one row)
    }
}

}  // namespace cd
