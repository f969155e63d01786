// cd_rays.h -- ray queries against the mesh: closest hit and occlusion.  Not reference behaviour.
//   k_cast_rays<ANY>  : one lane per ray, in the order given (neighbouring rays share a wave: coherent rays should be neighbours).
//       The lane walks the records from the ROOT with the queries' stackless pre-order walk (RecCursor, cd_bvh.h: the walk, its
//       step bound and its guards are described there), entering the boxes the ray meets; n == 1 has no records and every lane
//       tests leaf 0.
//       At a leaf the exact FP64 test ray_tri (cd_math.h) runs INLINE -- the ray's upper end shrinks with every hit, so a candidate
//       queue would only carry boxes the next hit makes pointless.  Closest hit: the smallest (t, triangle ID, face index) wins, and a
//       subtree is skipped when its box is missed over [0, t_best], CLOSED, so that a triangle at the same t with a smaller ID is
//       still seen.  ANY: the lane stops at its first hit; which one that is depends on the tree, whether there is one does not.
//   The filter only filters.  The slab test is FP64 on the stored fp32 bounds read as [lo, prox_hi(hi)] (converted exactly), widened
//       by pad = 2^-20 max(M, |o|_inf), M the largest |coordinate| of the root box.  A hit of ray_tri has its computed point
//       P = o + t d within G = 2^-30 max(|o|_inf, the triangle's largest |coordinate|) <= 2^-10 pad of the triangle's box on every
//       axis (ray_tri's gate); every box on the leaf's root path contains that box; the quotients (bound - o_a) / d_a are IEEE
//       divisions of one rounded difference, off by a relative 2^-52 of values no larger than M + pad + |o|_inf: the pad covers gate
//       and rounding with a margin of about 2^10.  An axis with d_a == 0 tests o_a against the padded interval and divides nothing;
//       a NaN (there is none for finite input: no quotient has a zero divisor) would widen, never cull.
//   k_ray_tri_points  : ray_tri on explicit operands, the pin of the device function (cd_ray_tri_points).
#pragma once
#include "cd_proximity.h"

namespace cd {

constexpr int RAY_THREADS = 64;
constexpr uint32_t RAY_MISS = 0xffffffffu;
struct alignas(64) RayState { unsigned long long n_hits, node_visits, tri_tests, pad[5]; };

// does the ray meet the padded box over [0, tfar]?  (h0, h1: a record half, lo = h0.xyz, hi = (h0.w, h1.x, h1.y))
__device__ __forceinline__ bool ray_box(const float4 h0, const float4 h1, const d3 o, const d3 d, const double pad, const double tfar)
{
    double tn = 0.0, tf = tfar;
    bool ok = true;
#define CD_RAY_AXIS(LO, HI, O, D)                                                                              \
    {                                                                                                          \
        const double l = (double)(LO) - pad, h = (double)prox_hi(HI) + pad;                                    \
        if ((D) == 0.0) ok = ok && l <= (O) && (O) <= h;                                                       \
        else {                                                                                                 \
            const double a = (l - (O)) / (D), b = (h - (O)) / (D);                                             \
            const double nr = (D) > 0.0 ? a : b, fr = (D) > 0.0 ? b : a;                                       \
            if (nr > tn) tn = nr;                                          /* (a NaN changes nothing) */       \
            if (fr < tf) tf = fr;                                                                              \
        }                                                                                                      \
    }
    CD_RAY_AXIS(h0.x, h0.w, o.x, d.x)
    CD_RAY_AXIS(h0.y, h1.x, o.y, d.y)
    CD_RAY_AXIS(h0.z, h1.y, o.z, d.z)
#undef CD_RAY_AXIS
    return ok && tn <= tf;
}

// The per-item queries' counters (RayState, PointState: items answered, boxes visited, triangles tested): the wave's sums, one
// atomic per non-zero sum.  One wave per workgroup; every lane calls this.
__device__ __forceinline__ void item_counters_add(bool got, uint32_t visits, uint32_t tests, unsigned long long *__restrict__ n_got,
                                                  unsigned long long *__restrict__ node_visits, unsigned long long *__restrict__ tri_tests)
{
    const unsigned long long ng = wave_sum_u64(got ? 1ull : 0ull), nv = wave_sum_u64(visits), nt = wave_sum_u64(tests);
    if (threadIdx.x == 0) {
        if (ng) atomicAdd(n_got, ng);
        if (nv) atomicAdd(node_visits, nv);
        if (nt) atomicAdd(tri_tests, nt);
    }
}

template <bool ANY>
__global__ __launch_bounds__(RAY_THREADS) void k_cast_rays(const NodeRec32 *__restrict__ recs, const int32_t *__restrict__ root_name, const LeafTri *__restrict__ leaf,
                                                           const uint32_t *__restrict__ perm, const double *__restrict__ verts, const double *__restrict__ root_box, int n,
                                                           const double *__restrict__ rays, unsigned long long nr, RayState *__restrict__ st,
                                                           uint32_t *__restrict__ face, uint32_t *__restrict__ ids, double *__restrict__ t_out,
                                                           double *__restrict__ uv, uint8_t *__restrict__ side)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * RAY_THREADS + threadIdx.x;
    bool active = i < nr;
    d3 o{0.0, 0.0, 0.0}, d{0.0, 0.0, 0.0};
    double tbest = 0.0, pad = 0.0;                                       // closest hit: the ray's upper end so far; ANY: tmax
    if (active) {
        const double *r = rays + 7 * i;
        o = d3{r[0], r[1], r[2]}; d = d3{r[3], r[4], r[5]}; tbest = r[6];
        pad = dmax_abs3(root_max_abs(root_box), o) * PROX_SLACK;
    }
    uint32_t bface = RAY_MISS, bid = 0u, bside = 0u;
    double bu = 0.0, bv = 0.0;
    uint32_t visits = 0, tests = 0;
    RecCursor w{};
    const bool leaf_only = n == 1;                                       // no records: leaf 0 is the whole tree
    if (active && !leaf_only) active = w.start_root(recs, n, (uint32_t)*root_name);   // (no tree: nothing is read; the ray misses)
    while (active) {
        bool test = leaf_only;
        uint32_t k = 0;
        if (!leaf_only) {
            ++visits;
            const bool ov = ray_box(w.h0, w.h1, o, d, pad, tbest);
            if (ov && w.internal(n)) {
                if (!w.descend(recs, n)) break;
                continue;
            }
            if (ov && w.leaf(n)) { test = true; k = w.leaf_index(); }
        }
        if (test) {
            ++tests;
            const LeafTri lt = leaf[k];
            const RayHit h = ray_tri(o, d, tbest, load_vertex(verts, lt.v0), load_vertex(verts, lt.v1), load_vertex(verts, lt.v2));
            if (h.hit) {
                const uint32_t f = perm[k];
                if (ANY) { bface = f; break; }
                // (t <= tbest holds.)  the smallest (t, ID, face index)
                if (bface == RAY_MISS || h.t < tbest || lt.id < bid || (lt.id == bid && f < bface)) {
                    bface = f; bid = lt.id; tbest = h.t; bu = h.u; bv = h.v; bside = h.side;
                }
            }
        }
        if (leaf_only || !w.next(recs, n)) break;
    }
    if (i < nr) {
        const bool hit = bface != RAY_MISS;
        face[i] = bface;
        if (!ANY) {
            if (ids) ids[i] = hit ? bid : 0u;
            if (t_out) t_out[i] = hit ? tbest : __builtin_inf();
            if (uv) { uv[2 * i] = hit ? bu : 0.0; uv[2 * i + 1] = hit ? bv : 0.0; }
            if (side) side[i] = (uint8_t)(hit ? bside : 0u);
        }
    }
    item_counters_add(i < nr && bface != RAY_MISS, visits, tests, &st->n_hits, &st->node_visits, &st->tri_tests);
}

// cd_ray_tri_points: ray_tri on explicit operands, n x 7 doubles (o, d, tmax) and n x 9 (p0, p1, p2)
__global__ __launch_bounds__(256) void k_ray_tri_points(const double *__restrict__ ray, const double *__restrict__ tri, unsigned long long n,
                                                        uint8_t *__restrict__ hit, double *__restrict__ t, double *__restrict__ uv, uint8_t *__restrict__ side)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256) {
        const double *r = ray + 7 * i, *p = tri + 9 * i;
        const RayHit h = ray_tri(d3{r[0], r[1], r[2]}, d3{r[3], r[4], r[5]}, r[6], d3{p[0], p[1], p[2]}, d3{p[3], p[4], p[5]}, d3{p[6], p[7], p[8]});
        hit[i] = h.hit ? 1 : 0;
        if (t) t[i] = h.t;
        if (uv) { uv[2 * i] = h.u; uv[2 * i + 1] = h.v; }
        if (side) side[i] = (uint8_t)h.side;
    }
}

}  // namespace cd
