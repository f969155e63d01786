// cd_ccd.h -- continuous collision queries: every pair of triangles of the mesh with no shared vertex index that comes within
// `dist` while its vertices move linearly from x0 (the context's vertices, the tree's) to x1, with the time it does.  Not reference
// behaviour.  Per pair: conservative advancement with report threshold dist and target h = dist / 2
// (ccd_advance below, restated in tests/ccd_ref.py bit for bit).
//   k_ccd_links    : one lane per record s: copies the links of the static records (cd_bvh.h) into the swept records and scatters
//       each child's parent (s, side) into up[], so nothing depends on which build made the tree.
//   k_ccd_refit    : one lane per leaf: the FP64 box of the leaf's six points (x0 and x1) rounded outward to fp32 is written into
//       its parent's record half; the lane climbs while it is the second to arrive at a record (per-split arrival counter) and
//       writes the union of that record's two halves into ITS parent's half.  fp32 unions of outward-rounded boxes are true bounds.
//   k_ccd_descend  : k_prox_descend over the swept records (prox_walk with the records' hi read as they are); the query box is the
//       leaf's swept box widened by ccd_pad with directed rounding; candidates go through the same LDS queue to the same shards.
//   k_ccd_exact    : neighbour filter, FP64 swept-box gate, ccd_advance, append (IDs, toi, d) with one atomic per workgroup and round
//       (the exact stage's scaffold, cd_proximity.h).
//   k_ccd_points   : ccd_advance on explicit positions (cd_ccd_points): the pin of the device code.
#pragma once
#include "cd_proximity.h"

namespace cd {

constexpr int CCD_MAX_EVALS = 1024;                   // tri_distance evaluations a pair may take; a pair still > dist after the last: unresolved
constexpr double CCD_L_SLACK = 1.0 + 1.0 / 1048576.0; // the rate bound L is scaled by 1 + 2^-20 (covers its own rounding)
constexpr int CCD_THREADS = 256;                      // k_ccd_links / k_ccd_refit / k_ccd_points
struct alignas(128) CcdState {
    unsigned long long shard[NSHARD * PROX_SHARD_STRIDE];   // candidates reserved in shard s: shard[s * PROX_SHARD_STRIDE] (may exceed the capacity)
    unsigned long long n_pairs, n_tested, n_evals, n_unresolved;
    uint32_t m_bits, pad32;                           // fp32 bits of the largest |coordinate| of x0 and x1 over the leaves (rounded up)
    unsigned long long pad[11];
};

// ---------------------------------------------------------------- the per-pair function
// Vertex k of the pair (0..2: A's, 3..5: B's) at x0 and x1.  (k is a constant after unrolling: no private arrays, no scratch.)
struct CcdMeshSrc {
    const double *__restrict__ x0; const double *__restrict__ x1; uint32_t a0, a1, a2, b0, b1, b2;
    __device__ __forceinline__ uint32_t vid(int k) const { return k == 0 ? a0 : (k == 1 ? a1 : (k == 2 ? a2 : (k == 3 ? b0 : (k == 4 ? b1 : b2)))); }
    __device__ __forceinline__ d3 p0(int k) const { return load_vertex(x0, vid(k)); }
    __device__ __forceinline__ d3 p1(int k) const { return load_vertex(x1, vid(k)); }
    __device__ __forceinline__ void launder() { asm volatile("" : "+v"(x0), "+v"(x1)); }
};
struct CcdPointSrc {                                  // 36 doubles: A0 A1 A2 B0 B1 B2 at x0, then the same at x1
    const double *__restrict__ t;
    __device__ __forceinline__ d3 p0(int k) const { return d3{t[3 * k], t[3 * k + 1], t[3 * k + 2]}; }
    __device__ __forceinline__ d3 p1(int k) const { return d3{t[18 + 3 * k], t[18 + 3 * k + 1], t[18 + 3 * k + 2]}; }
    __device__ __forceinline__ void launder() { asm volatile("" : "+v"(t)); }
};

// L = (max_i |dA_i - g| + max_j |dB_j - g|) (1 + 2^-20), d = p1 - p0, g the mean of the six d (summed A0 .. B2, then / 6),
// |v| = sqrt((x x + y y) + z z): a bound on how fast the distance of the two linearly moving triangles can change.
template <class S> __device__ __forceinline__ double ccd_rate(const S &s)
{
    d3 g = d3{0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 6; ++k) { const d3 d = sub(s.p1(k), s.p0(k)); g = d3{g.x + d.x, g.y + d.y, g.z + d.z}; }
    g = d3{g.x / 6.0, g.y / 6.0, g.z / 6.0};
    double ma = 0.0, mb = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const d3 v = sub(sub(s.p1(k), s.p0(k)), g);
        const double l = __builtin_sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
        if (k < 3) ma = l > ma ? l : ma; else mb = l > mb ? l : mb;
    }
    return (ma + mb) * CCD_L_SLACK;
}

// vertex k where the advancement evaluates: x0 itself (stage 0), p(t) = p0 + t (p1 - p0) (stage 1), x1 itself (stage 2)
template <class S> __device__ __forceinline__ d3 ccd_at(const S &s, int k, int stage, double t)
{
    const d3 a = s.p0(k);
    if (stage == 0) return a;
    const d3 b = s.p1(k);
    if (stage == 2) return b;
    return d3{a.x + t * (b.x - a.x), a.y + t * (b.y - a.y), a.z + t * (b.z - a.z)};
}

// Conservative advancement.  Reported: toi finite; d <= dist, or d > dist for a pair left unresolved after
// CCD_MAX_EVALS evaluations (toi = the t of the last one).  Not reported: toi = +inf, d = the last distance evaluated.
template <class S> __device__ inline void ccd_advance(const S &src, double dist, double &toi, double &dout, uint32_t &evals)
{
    S s = src;
    const double h = dist * 0.5, L = ccd_rate(s);
    double t = 0.0, d = 0.0, res = __builtin_inf();
    int stage = 0;
    uint32_t n = 0;
    for (;;) {                                        // one tri_distance call site (inlined once)
        s.launder();                                  // (the positions are loaded again each round, not held in 72 registers across the loop)
        d = tri_distance(ccd_at(s, 0, stage, t), ccd_at(s, 1, stage, t), ccd_at(s, 2, stage, t),
                         ccd_at(s, 3, stage, t), ccd_at(s, 4, stage, t), ccd_at(s, 5, stage, t));
        ++n;
        if (d <= dist) { res = stage == 2 ? 1.0 : t; break; }
        if (stage == 2 || L == 0.0) break;            // apart at x1, or a rigid translation apart at x0: not reported
        if (n >= (uint32_t)CCD_MAX_EVALS) { res = t; break; }   // unresolved (d > dist)
        const double tn = t + (d - h) / L;
        if (tn >= 1.0) stage = 2; else { t = tn; stage = 1; }
    }
    toi = res; dout = d; evals = n;
}

// The FP64 swept-box gate: the boxes of each triangle's six points, widened by dist (lo - dist, hi + dist), overlap (closed).
template <class S> __device__ __forceinline__ Box swept_box(const S &s, int k0)
{
    Box b = box_set(s.p0(k0), s.p0(k0 + 1), s.p0(k0 + 2));
    const Box e = box_set(s.p1(k0), s.p1(k0 + 1), s.p1(k0 + 2));
    b.x1 = fmin2(b.x1, e.x1); b.y1 = fmin2(b.y1, e.y1); b.z1 = fmin2(b.z1, e.z1);
    b.x2 = fmax2(b.x2, e.x2); b.y2 = fmax2(b.y2, e.y2); b.z2 = fmax2(b.z2, e.z2);
    return b;
}
template <class S> __device__ __forceinline__ bool ccd_gate(const S &s, double dist)
{
    const Box a = swept_box(s, 0), b = swept_box(s, 3);
    return (a.x1 - dist) <= (b.x2 + dist) && (b.x1 - dist) <= (a.x2 + dist) && (a.y1 - dist) <= (b.y2 + dist) &&
           (b.y1 - dist) <= (a.y2 + dist) && (a.z1 - dist) <= (b.z2 + dist) && (b.z1 - dist) <= (a.z2 + dist);
}

// ---------------------------------------------------------------- swept records
// up[j] (leaf j) and up[n + s] (internal node named by split s): (parent split << 1) | side (0 left, 1 right); -1 (the host's memset)
// for the root.  Both kernels check the sort flags first (sort_failed, cd_traverse.h), as k_prox_descend does: after a failed sort the records are not a tree
// (the host redoes the build), and nothing is read from them or written through them.  Links outside [0, n) are skipped and the
// climb is bounded by n steps, so not even a broken tree can send a lane out of bounds.
__global__ __launch_bounds__(CCD_THREADS) void k_ccd_links(const NodeRec32 *__restrict__ recs, int n, const uint32_t *__restrict__ sort_flags /* 9 words */,
                                                           NodeRec32 *__restrict__ swept, int32_t *__restrict__ up, uint32_t *__restrict__ arrive)
{
    const uint32_t s = blockIdx.x * CCD_THREADS + threadIdx.x;
    if ((int)s >= n - 1 || sort_failed(sort_flags)) return;
    const float4 l1 = rec_left(recs, n, s)[1], r1 = rec_right(recs, n, s)[1];
    const_cast<float4 *>(rec_left(swept, n, s))[1] = l1;                // links and range words; the box floats are the refit's
    const_cast<float4 *>(rec_right(swept, n, s))[1] = r1;
    arrive[s] = 0u;
    const int32_t cl = (int32_t)__float_as_uint(l1.z), cr = (int32_t)__float_as_uint(r1.z);
    const int32_t il = cl >= 0 ? n + cl : ~cl, ir = cr >= 0 ? n + cr : ~cr;   // (cl < n - 1 and ~cl < n in a tree)
    if (il < 2 * n - 1) up[il] = (int32_t)(s << 1);
    if (ir < 2 * n - 1) up[ir] = (int32_t)(s << 1) | 1;
}

// A record half's six box floats, handed from one lane to the lane that arrives second at the record: agent-scope atomic stores and
// loads (write-through / L2-coherent, 8 bytes each), the stores drained before the arrival's atomic add.
__device__ __forceinline__ unsigned long long pack2(float a, float b) { return (unsigned long long)__float_as_uint(a) | ((unsigned long long)__float_as_uint(b) << 32); }
__device__ __forceinline__ void half_store(NodeRec32 *swept, int n, uint32_t s, int side, const float lo[3], const float hi[3])
{
    unsigned long long *p = reinterpret_cast<unsigned long long *>(const_cast<float4 *>(side ? rec_right(swept, n, s) : rec_left(swept, n, s)));
    __hip_atomic_store(p + 0, pack2(lo[0], lo[1]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p + 1, pack2(lo[2], hi[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p + 2, pack2(hi[1], hi[2]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void half_load(const NodeRec32 *swept, int n, uint32_t s, int side, float lo[3], float hi[3])
{
    unsigned long long *p = reinterpret_cast<unsigned long long *>(const_cast<float4 *>(side ? rec_right(swept, n, s) : rec_left(swept, n, s)));
    const unsigned long long u0 = __hip_atomic_load(p + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long u1 = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const unsigned long long u2 = __hip_atomic_load(p + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    lo[0] = __uint_as_float((uint32_t)u0); lo[1] = __uint_as_float((uint32_t)(u0 >> 32)); lo[2] = __uint_as_float((uint32_t)u1);
    hi[0] = __uint_as_float((uint32_t)(u1 >> 32)); hi[1] = __uint_as_float((uint32_t)u2); hi[2] = __uint_as_float((uint32_t)(u2 >> 32));
}

__global__ __launch_bounds__(CCD_THREADS) void k_ccd_refit(const LeafTri *__restrict__ leaf, const double *__restrict__ x0, const double *__restrict__ x1, int n,
                                                           const uint32_t *__restrict__ sort_flags /* 9 words */, const int32_t *__restrict__ up,
                                                           uint32_t *__restrict__ arrive, NodeRec32 *__restrict__ swept, CcdState *__restrict__ st)
{
    const uint32_t j = blockIdx.x * CCD_THREADS + threadIdx.x;
    if (sort_failed(sort_flags)) return;
    uint32_t mbits = 0u;
    if ((int)j < n) {
        const LeafTri lt = leaf[j];
        const CcdMeshSrc src{x0, x1, lt.v0, lt.v1, lt.v2, 0u, 0u, 0u};
        const Box b = swept_box(src, 0);
        float lo[3] = {__double2float_rd(b.x1), __double2float_rd(b.y1), __double2float_rd(b.z1)};
        float hi[3] = {__double2float_ru(b.x2), __double2float_ru(b.y2), __double2float_ru(b.z2)};
        double m = fmax2(fmax2(dabs(b.x1), dabs(b.x2)), fmax2(fmax2(dabs(b.y1), dabs(b.y2)), fmax2(dabs(b.z1), dabs(b.z2))));
        mbits = __float_as_uint(__double2float_ru(m)) & 0x7fffffffu;         // (dabs(-0.0) is -0.0: without its sign bit, which would win the unsigned max below)
        int32_t u = up[j];
        for (int steps = 0; u >= 0 && ((uint32_t)u >> 1) < (uint32_t)(n - 1) && steps < n; ++steps) {
            const uint32_t s = (uint32_t)u >> 1;
            const int side = u & 1;
            half_store(swept, n, s, side, lo, hi);
            __builtin_amdgcn_s_waitcnt(0);                                   // (the half is written before the arrival is counted)
            if (__hip_atomic_fetch_add(&arrive[s], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) break;   // first: the sibling goes on
            float olo[3], ohi[3];
            half_load(swept, n, s, side ^ 1, olo, ohi);
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = olo[a] < lo[a] ? olo[a] : lo[a]; hi[a] = ohi[a] > hi[a] ? ohi[a] : hi[a]; }
            u = up[n + s];
        }
    }
    for (int o = 32; o; o >>= 1) { const uint32_t v = __shfl_xor(mbits, o); mbits = v > mbits ? v : mbits; }   // (non-negative floats: bits order as values)
    if ((threadIdx.x & 63) == 0 && mbits) atomicMax(&st->m_bits, mbits);
}

// the query pad: 2 dist + 2 dist 2^-20 + M 2^-20 rounded up, M the largest |coordinate| of x0 and x1 (the gate widens BOTH boxes by dist)
__device__ __forceinline__ float ccd_pad(const CcdState *__restrict__ st, double dist)
{
    const double m = (double)__uint_as_float(st->m_bits);
    return __double2float_ru(2.0 * dist + 2.0 * dist * PROX_SLACK + m * PROX_SLACK);
}

// k_prox_descend over the swept records (whose boxes are true bounds: no next_up), the query box the leaf's swept box
__global__ __launch_bounds__(PROX_DESC_THREADS) void k_ccd_descend(const NodeRec32 *__restrict__ recs, const LeafTri *__restrict__ leaf,
                                                                   const double *__restrict__ x0, const double *__restrict__ x1, int n, double dist,
                                                                   const uint32_t *__restrict__ sort_flags /* 9 words */, CcdState *__restrict__ st,
                                                                   uint2 *__restrict__ cand, unsigned long long shard_cap)
{
    if (sort_failed(sort_flags)) return;                                 // the records are not a tree (the host redoes the build)
    const uint32_t j = blockIdx.x * PROX_DESC_THREADS + threadIdx.x;
    const float pad = ccd_pad(st, dist);
    const bool active = (int)j < n - 1;
    QueryBox32 q{};
    RecCursor w{};
    if (active) {
        const LeafTri lt = leaf[j];
        q = query_box32(swept_box(CcdMeshSrc{x0, x1, lt.v0, lt.v1, lt.v2, 0u, 0u, 0u}, 0), pad);
        w.start_behind(recs, n, j);
    }
    prox_walk(recs, n, j, active, w, BoxFilter<HiTrue>{q}, st->shard, cand, shard_cap);
}

template <bool WIT>                                    // (the witness calls: wleaf[at] = the hit's leaf positions, A's first, as k_prox_exact)
__global__ __launch_bounds__(PROX_EXACT_THREADS) void k_ccd_exact(const uint2 *__restrict__ cand, unsigned long long shard_cap, const LeafTri *__restrict__ leaf,
                                                                 const uint32_t *__restrict__ perm, const double *__restrict__ x0, const double *__restrict__ x1,
                                                                 double dist, CcdState *__restrict__ st, uint32_t *__restrict__ pairs, double *__restrict__ toi_out,
                                                                 double *__restrict__ dists, unsigned long long cap, uint2 *__restrict__ wleaf)
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
            LeafTri A = leaf[c.x], B = leaf[c.y];
            lv = c;
            if (neighbor_count(A.v0, A.v1, A.v2, B.v0, B.v1, B.v2) < 1) {                 // collision.cuh:38
                if (B.id < A.id || (B.id == A.id && perm[c.y] < perm[c.x])) { const LeafTri t = A; A = B; B = t; lv = make_uint2(c.y, c.x); }   // A: the smaller ID (then face index)
                const CcdMeshSrc src{x0, x1, A.v0, A.v1, A.v2, B.v0, B.v1, B.v2};
                if (ccd_gate(src, dist)) {
                    ++sums[0];
                    uint32_t ne = 0;
                    ccd_advance(src, dist, toi, d, ne);
                    sums[1] += ne;
                    hit = toi <= 1.0;
                    sums[2] += (hit && !(d <= dist)) ? 1u : 0u;
                    ida = A.id; idb = B.id;
                }
            }
        }
        pair_append(hit, &st->n_pairs, cap, [&](unsigned long long at) { pairs[2 * at] = ida; pairs[2 * at + 1] = idb; toi_out[at] = toi; dists[at] = d; if (WIT) wleaf[at] = lv; });
    }
    group_counters_add<3>(sums, &st->n_tested, &st->n_evals, &st->n_unresolved);
}

// cd_ccd_points: ccd_advance on explicit positions, n x 36 doubles
__global__ __launch_bounds__(CCD_THREADS) void k_ccd_points(const double *__restrict__ tri, unsigned long long n, double dist, double *__restrict__ toi,
                                                            double *__restrict__ dists, uint32_t *__restrict__ evals)
{
    for (unsigned long long i = (unsigned long long)blockIdx.x * CCD_THREADS + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * CCD_THREADS) {
        double t, d; uint32_t e;
        ccd_advance(CcdPointSrc{tri + 36 * i}, dist, t, d, e);
        toi[i] = t; dists[i] = d; evals[i] = e;
    }
}

}  // namespace cd
