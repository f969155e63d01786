// cd_math.h -- device arithmetic of the collision path: every FP64 operation is written in the
// reference's operand order and the TU is compiled with -ffp-contract=off, so each compare sees
// bit-identical operands to the reference's host twin (cpu.cuh) and to oracle/cd_oracle.c.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cd {

struct d3 { double x, y, z; };

// mathop.cuh:17-44 -- compare-select, NOT fmin/fmax (NaN-asymmetric on purpose)
__device__ __forceinline__ double fmax2(double a, double b) { return (a > b) ? a : b; }
__device__ __forceinline__ double fmin2(double a, double b) { return (a < b) ? a : b; }
__device__ __forceinline__ double fmax3(double a, double b, double c) { double t = a; if (b > t) t = b; if (c > t) t = c; return t; }
__device__ __forceinline__ double fmin3(double a, double b, double c) { double t = a; if (b < t) t = b; if (c < t) t = c; return t; }

// vec3f.cuh:100-103, 118-125
__device__ __forceinline__ d3 sub(const d3 a, const d3 b) { return d3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ d3 neg(const d3 a) { return d3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ d3 cross(const d3 a, const d3 b)
{ return d3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double dot(const d3 a, const d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// Box = {x1,x2,y1,y2,z1,z2}, box.cuh:9
struct Box { double x1, x2, y1, y2, z1, z2; };

// box.cuh:13-22
__device__ __forceinline__ Box box_set(const d3 a, const d3 b, const d3 c)
{
    Box r;
    r.x1 = fmin3(a.x, b.x, c.x); r.x2 = fmax3(a.x, b.x, c.x);
    r.y1 = fmin3(a.y, b.y, c.y); r.y2 = fmax3(a.y, b.y, c.y);
    r.z1 = fmin3(a.z, b.z, c.z); r.z2 = fmax3(a.z, b.z, c.z);
    return r;
}
// box.cuh:24-32
__device__ __forceinline__ Box box_merge(const Box &a, const Box &b)
{
    Box r;
    r.x1 = fmin2(a.x1, b.x1); r.x2 = fmax2(a.x2, b.x2);
    r.y1 = fmin2(a.y1, b.y1); r.y2 = fmax2(a.y2, b.y2);
    r.z1 = fmin2(a.z1, b.z1); r.z2 = fmax2(a.z2, b.z2);
    return r;
}
// box.cuh:40-43 -- strict overlap, product form
__device__ __forceinline__ bool box_overlap(const Box &a, const Box &b)
{
    return (a.x1 - b.x2) * (b.x1 - a.x2) > 0 && (a.y1 - b.y2) * (b.y1 - a.y2) > 0 &&
           (a.z1 - b.z2) * (b.z1 - a.z2) > 0;
}

// triangle.cuh:18-30
__device__ __forceinline__ int neighbor_count(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2)
{
    return (a0 == b0) + (a0 == b1) + (a0 == b2) + (a1 == b0) + (a1 == b1) + (a1 == b2) +
           (a2 == b0) + (a2 == b1) + (a2 == b2);
}

// vec3f.cuh:257-270
__device__ __forceinline__ bool project3(const d3 ax, const d3 p1, const d3 p2, const d3 p3)
{
    const double P1 = dot(ax, p1), P2 = dot(ax, p2), P3 = dot(ax, p3);
    const double mx1 = fmax3(P1, P2, P3), mn1 = fmin3(P1, P2, P3);
    if (mn1 > 0) return false;
    if (0 > mx1) return false;
    return true;
}
// vec3f.cuh:272-291
__device__ __forceinline__ bool project6(const d3 ax, const d3 p1, const d3 p2, const d3 p3,
                                         const d3 q1, const d3 q2, const d3 q3)
{
    const double P1 = dot(ax, p1), P2 = dot(ax, p2), P3 = dot(ax, p3);
    const double Q1 = dot(ax, q1), Q2 = dot(ax, q2), Q3 = dot(ax, q3);
    const double mx1 = fmax3(P1, P2, P3), mn1 = fmin3(P1, P2, P3);
    const double mx2 = fmax3(Q1, Q2, Q3), mn2 = fmin3(Q1, Q2, Q3);
    if (mn1 > mx2) return false;
    if (mn2 > mx1) return false;
    return true;
}

// tri_contact.cuh:19-78: 17-axis SAT.  The verdict is a pure conjunction of the 17 interval tests,
// so evaluating axes lazily (cross product only when its test is reached) returns the same value
// as the reference's eager evaluation; each axis itself is computed with the reference's operations.
__device__ __forceinline__ bool tri_contact(const d3 P1, const d3 P2, const d3 P3, const d3 Q1, const d3 Q2, const d3 Q3)
{
    const d3 p1 = d3{0.0, 0.0, 0.0};
    const d3 p2 = sub(P2, P1), p3 = sub(P3, P1);
    const d3 q1 = sub(Q1, P1), q2 = sub(Q2, P1), q3 = sub(Q3, P1);
    const d3 e1 = sub(p2, p1), e2 = sub(p3, p2), e3 = sub(p1, p3);
    const d3 f1 = sub(q2, q1), f2 = sub(q3, q2), f3 = sub(q1, q3);
    const d3 n1 = cross(e1, e2);
    if (!project3(n1, q1, q2, q3)) return false;
    const d3 m1 = cross(f1, f2);
    if (!project3(m1, neg(q1), sub(p2, q1), sub(p3, q1))) return false;
    if (!project6(cross(e1, f1), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e1, f2), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e1, f3), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e2, f1), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e2, f2), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e2, f3), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e3, f1), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e3, f2), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e3, f3), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e1, n1), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e2, n1), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(e3, n1), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(f1, m1), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(f2, m1), p1, p2, p3, q1, q2, q3)) return false;
    if (!project6(cross(f3, m1), p1, p2, p3, q1, q2, q3)) return false;
    return true;
}

// The same verdict with the hardware's FP64 max / min (k_exact: the SAT of ~100 k survivors is 6.8 of its 14.6 us, and a third of an axis' ~65 instructions
// are the compare + two selects + wait states of each of its eight compare-selects).  v_max_f64 / v_min_f64 return what mathop.cuh's compare-selects return whenever
// neither operand is a NaN -- up to the SIGN of a zero (max(+0, -0)) and which of two EQUAL operands comes back, and the projections' results only ever meet a `>`,
// which sees neither.  With a NaN among an axis' dot products (non-finite vertices, or products that overflow to inf - inf) the two differ, on purpose in the
// reference (mathop.cuh:17-44 is NaN-asymmetric): `nan` says whether any evaluated axis had one, and tri_contact_fast then takes the verdict from tri_contact itself.
// (inline asm: fmax() would be canonicalised -- an extra v_max_f64 x, x per loaded operand under IEEE mode)
__device__ __forceinline__ double hw_max64(double a, double b) { double r; asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ double hw_min64(double a, double b) { double r; asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ bool project3_hw(const d3 ax, const d3 p1, const d3 p2, const d3 p3, bool &nan)
{
    const double P1 = dot(ax, p1), P2 = dot(ax, p2), P3 = dot(ax, p3);
    nan |= __builtin_isunordered(P1, P2) | __builtin_isunordered(P3, P3);
    const double mx1 = hw_max64(hw_max64(P1, P2), P3), mn1 = hw_min64(hw_min64(P1, P2), P3);
    if (mn1 > 0) return false;
    if (0 > mx1) return false;
    return true;
}
__device__ __forceinline__ bool project6_hw(const d3 ax, const d3 p1, const d3 p2, const d3 p3, const d3 q1, const d3 q2, const d3 q3, bool &nan)
{
    const double P1 = dot(ax, p1), P2 = dot(ax, p2), P3 = dot(ax, p3);
    const double Q1 = dot(ax, q1), Q2 = dot(ax, q2), Q3 = dot(ax, q3);
    nan |= __builtin_isunordered(P1, P2) | __builtin_isunordered(P3, Q1) | __builtin_isunordered(Q2, Q3);
    const double mx1 = hw_max64(hw_max64(P1, P2), P3), mn1 = hw_min64(hw_min64(P1, P2), P3);
    const double mx2 = hw_max64(hw_max64(Q1, Q2), Q3), mn2 = hw_min64(hw_min64(Q1, Q2), Q3);
    if (mn1 > mx2) return false;
    if (mn2 > mx1) return false;
    return true;
}
__device__ __forceinline__ bool tri_contact_hw(const d3 P1, const d3 P2, const d3 P3, const d3 Q1, const d3 Q2, const d3 Q3, bool &nan)
{
    const d3 p1 = d3{0.0, 0.0, 0.0};
    const d3 p2 = sub(P2, P1), p3 = sub(P3, P1);
    const d3 q1 = sub(Q1, P1), q2 = sub(Q2, P1), q3 = sub(Q3, P1);
    const d3 e1 = sub(p2, p1), e2 = sub(p3, p2), e3 = sub(p1, p3);
    const d3 f1 = sub(q2, q1), f2 = sub(q3, q2), f3 = sub(q1, q3);
    const d3 n1 = cross(e1, e2);
    if (!project3_hw(n1, q1, q2, q3, nan)) return false;
    const d3 m1 = cross(f1, f2);
    if (!project3_hw(m1, neg(q1), sub(p2, q1), sub(p3, q1), nan)) return false;
    if (!project6_hw(cross(e1, f1), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e1, f2), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e1, f3), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e2, f1), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e2, f2), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e2, f3), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e3, f1), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e3, f2), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e3, f3), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e1, n1), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e2, n1), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(e3, n1), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(f1, m1), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(f2, m1), p1, p2, p3, q1, q2, q3, nan)) return false;
    if (!project6_hw(cross(f3, m1), p1, p2, p3, q1, q2, q3, nan)) return false;
    return true;
}
__device__ __forceinline__ bool tri_contact_fast(const d3 P1, const d3 P2, const d3 P3, const d3 Q1, const d3 Q2, const d3 Q3)
{
    bool nan = false;
    bool c = tri_contact_hw(P1, P2, P3, Q1, Q2, Q3, nan);
    if (nan) c = tri_contact(P1, P2, P3, Q1, Q2, Q3);                    // (a lane at a time, and rare: a NaN among the projections)
    return c;
}

// ---------------------------------------------------------------- triangle-triangle distance (cd_find_proximity; not reference behaviour)
// tri_distance(A, B) = 0 when the pair is IN CONTACT as the collision path decides it -- the FP64 boxes overlap strictly (box.cuh:40-43,
// box_overlap) and tri_contact(A, B) holds -- else sqrt of the minimum squared distance over the feature pairs: every vertex against
// the other triangle's face interior (pt_face2) and its three edges (pt_seg2), and every edge pair's interior critical point (seg_seg2).
// Each term is |P - Q|^2 for two points P, Q that lie on the two triangles up to the rounding of forming them (a clamped or range-checked
// parameter, never an extrapolation), so the result is never below the true distance by more than a few ulps of the coordinates
// (DESIGN.md section 10).  A face whose barycentric denominator is not > 0 (zero area, collinear, a point) and an edge pair that is parallel
// contribute nothing of their own: their edges' and vertices' terms remain, and those cover every pair of points of a segment or a point,
// so a degenerate triangle gets the distance of the point set it is.  The one exception is a pair the collision path calls in contact:
// the 17-axis test has only zero axes between two degenerate triangles (and no in-plane normal of a segment lying in a triangle's plane),
// so such a pair can be apart and still reported by cd_find_collisions -- here it is at 0, as every pair in contact is.  Without the box
// condition the test's verdict alone would put two points 5 apart at 0 although their boxes are disjoint.
// The coordinates are translated to A's first vertex and scaled by a power of two (exact) so that products of squares neither overflow
// nor underflow for |coordinates| anywhere in 1e-300 .. 1e300.  Fixed operation order, -ffp-contract=off, IEEE divide and sqrt: the
// numpy restatement (tests/proximity_ref.py) reproduces it bit for bit.  Non-finite vertices: undefined.
__device__ __forceinline__ double dmin2(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ d3 dscale(const d3 a, double s) { return d3{a.x * s, a.y * s, a.z * s}; }
// squared distance from p to the segment [a, b]; t: the clamped parameter of the closest point a + t (b - a) (0 for a == b)
__device__ __forceinline__ double pt_seg2_t(const d3 p, const d3 a, const d3 b, double &t)
{
    const d3 ab = sub(b, a), ap = sub(p, a);
    const double den = dot(ab, ab);
    t = 0.0;
    if (den > 0.0) { t = dot(ap, ab) / den; t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t); }
    const d3 q = d3{a.x + t * ab.x, a.y + t * ab.y, a.z + t * ab.z};
    const d3 d = sub(p, q);
    return dot(d, d);
}
__device__ __forceinline__ double pt_seg2(const d3 p, const d3 a, const d3 b) { double t; return pt_seg2_t(p, a, b, t); }
// squared distance from p to its projection a + v (b - a) + w (c - a) onto the plane of (a, b, c) when that projection lies in the
// triangle, else +inf (and v = w = 0)
__device__ __forceinline__ double pt_face2_vw(const d3 p, const d3 a, const d3 b, const d3 c, double &v, double &w)
{
    v = 0.0; w = 0.0;
    const d3 ab = sub(b, a), ac = sub(c, a), ap = sub(p, a);
    const double d00 = dot(ab, ab), d01 = dot(ab, ac), d11 = dot(ac, ac), d20 = dot(ap, ab), d21 = dot(ap, ac);
    const double den = d00 * d11 - d01 * d01;
    if (!(den > 0.0)) return __builtin_inf();
    const double fv = (d11 * d20 - d01 * d21) / den, fw = (d00 * d21 - d01 * d20) / den;
    if (!(fv >= 0.0 && fw >= 0.0 && fv + fw <= 1.0)) return __builtin_inf();
    const d3 q = d3{(a.x + fv * ab.x) + fw * ac.x, (a.y + fv * ab.y) + fw * ac.y, (a.z + fv * ab.z) + fw * ac.z};
    const d3 d = sub(p, q);
    v = fv; w = fw;
    return dot(d, d);
}
__device__ __forceinline__ double pt_face2(const d3 p, const d3 a, const d3 b, const d3 c) { double v, w; return pt_face2_vw(p, a, b, c, v, w); }
// squared distance between the segments [p1, q1], [p2, q2] at their interior critical point when it lies on both, else +inf
// (the endpoints' terms are pt_seg2's); s, t: the parameters of the two points p1 + s (q1 - p1), p2 + t (q2 - p2) (0 with +inf)
__device__ __forceinline__ double seg_seg2_st(const d3 p1, const d3 q1, const d3 p2, const d3 q2, double &s, double &t)
{
    s = 0.0; t = 0.0;
    const d3 d1 = sub(q1, p1), d2 = sub(q2, p2), r = sub(p1, p2);
    const double a = dot(d1, d1), e = dot(d2, d2), b = dot(d1, d2), c = dot(d1, r), f = dot(d2, r);
    const double den = a * e - b * b;
    if (!(den > 0.0)) return __builtin_inf();
    const double fs = (b * f - c * e) / den, ft = (a * f - b * c) / den;
    if (!(fs >= 0.0 && fs <= 1.0 && ft >= 0.0 && ft <= 1.0)) return __builtin_inf();
    const d3 P = d3{p1.x + fs * d1.x, p1.y + fs * d1.y, p1.z + fs * d1.z}, Q = d3{p2.x + ft * d2.x, p2.y + ft * d2.y, p2.z + ft * d2.z};
    const d3 d = sub(P, Q);
    s = fs; t = ft;
    return dot(d, d);
}
__device__ __forceinline__ double seg_seg2(const d3 p1, const d3 q1, const d3 p2, const d3 q2) { double s, t; return seg_seg2_st(p1, q1, p2, q2, s, t); }
constexpr int TRI_DIST_EXP_MAX = 1000;                  // |scale exponent| clamp: 2^+-1000 are normal numbers
__device__ __forceinline__ double dabs(double x) { return x < 0.0 ? -x : x; }
__device__ __forceinline__ double dmax_abs3(double m, const d3 v) { m = fmax2(m, dabs(v.x)); m = fmax2(m, dabs(v.y)); return fmax2(m, dabs(v.z)); }
__device__ __forceinline__ double pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }
__device__ inline double tri_distance(const d3 P1, const d3 P2, const d3 P3, const d3 Q1, const d3 Q2, const d3 Q3)
{
    if (box_overlap(box_set(P1, P2, P3), box_set(Q1, Q2, Q3)) && tri_contact_fast(P1, P2, P3, Q1, Q2, Q3)) return 0.0;   // in contact (collision.cuh:31-39)
    d3 p2 = sub(P2, P1), p3 = sub(P3, P1), q1 = sub(Q1, P1), q2 = sub(Q2, P1), q3 = sub(Q3, P1);
    double m = 0.0;
    m = dmax_abs3(m, p2); m = dmax_abs3(m, p3); m = dmax_abs3(m, q1); m = dmax_abs3(m, q2); m = dmax_abs3(m, q3);
    if (!(m > 0.0)) return 0.0;                                           // (six coincident points: tri_contact holds already)
    int ex = (int)((__double_as_longlong(m) >> 52) & 0x7ff) - 1022;     // m = f 2^ex, f in [0.5, 1) (frexp; a subnormal m is clamped below)
    ex = ex < -TRI_DIST_EXP_MAX ? -TRI_DIST_EXP_MAX : (ex > TRI_DIST_EXP_MAX ? TRI_DIST_EXP_MAX : ex);
    const double sc = pow2(-ex);
    const d3 p1 = d3{0.0, 0.0, 0.0};
    p2 = dscale(p2, sc); p3 = dscale(p3, sc); q1 = dscale(q1, sc); q2 = dscale(q2, sc); q3 = dscale(q3, sc);
    // the 33 terms, a vertex / edge index of each triangle at a time (a rolled loop: unrolled, the compiler keeps every term's operands
    // live at once: 250 VGPRs against 188); the minimum of exact values does not depend on the order they are taken in
    double best = __builtin_inf();
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
        const d3 pi = i == 0 ? p1 : (i == 1 ? p2 : p3), pn = i == 0 ? p2 : (i == 1 ? p3 : p1);     // vertex i of A, edge (i, i+1) of A
        const d3 qi = i == 0 ? q1 : (i == 1 ? q2 : q3);
        best = dmin2(best, pt_face2(pi, q1, q2, q3));
        best = dmin2(best, pt_face2(qi, p1, p2, p3));
        best = dmin2(best, pt_seg2(pi, q1, q2)); best = dmin2(best, pt_seg2(pi, q2, q3)); best = dmin2(best, pt_seg2(pi, q3, q1));
        best = dmin2(best, pt_seg2(qi, p1, p2)); best = dmin2(best, pt_seg2(qi, p2, p3)); best = dmin2(best, pt_seg2(qi, p3, p1));
        best = dmin2(best, seg_seg2(pi, pn, q1, q2)); best = dmin2(best, seg_seg2(pi, pn, q2, q3)); best = dmin2(best, seg_seg2(pi, pn, q3, q1));
    }
    return __builtin_sqrt(best) * pow2(ex);
}

// ---------------------------------------------------------------- where tri_distance is attained (not reference behaviour)
// tri_witness(A, B) -> (dist, feature_a, feature_b, ua, va, ub, vb, qa, qb): tri_distance's value, bit for bit, and the two points it is
// the distance of.  tri_distance's frame (translate to A's first vertex, scale by 2^-ex, |ex| clamped at TRI_DIST_EXP_MAX), its blocks and
// its operation order; no contraction, IEEE divide and sqrt.
//   dist = tri_distance(A, B) = sqrt(best) 2^ex -- NOT |qa - qb| recomputed.
//   Early-outs: a pair tri_distance puts at 0 through its early-outs -- strict FP64 box overlap and tri_contact, or six coincident points --
//   has NO witness: feature_a = feature_b = 7 and every other output except dist is 0.  (Interpenetration is CCD's to prevent; a pair in
//   contact has no closest points.)
//   Otherwise the 33 terms are taken in tri_distance's loop order, term 11 i + k for i = 0, 1, 2 (P = A, Q = B, scaled):
//     k = 0        pt_face2(P_i; Q)                           A: vertex i          B: the face
//     k = 1        pt_face2(Q_i; P)                           A: the face          B: vertex i
//     k = 2, 3, 4  pt_seg2(P_i; Q's edges 01, 12, 20)         A: vertex i          B: edge k - 2
//     k = 5, 6, 7  pt_seg2(Q_i; P's edges 01, 12, 20)         A: edge k - 5        B: vertex i
//     k = 8, 9, 10 seg_seg2(P's edge (i, i+1); Q's edges)     A: edge i            B: edge k - 8
//   and a later term replaces the running minimum only when it is STRICTLY smaller: an earlier term keeps a tie.  The distance does not
//   depend on that order; the witness does, so the order and the tie rule are part of the contract.  The winning term is evaluated
//   once more for its parameters, which give, in pt_tri's coding (0 face, 1 / 2 / 3 edge 01 / 12 / 20, 4 / 5 / 6 vertex 0 / 1 / 2):
//     vertex i          (u, v) = (0, 0), (1, 0), (0, 1)                          feature 4 + i
//     the face          (u, v) = (fv, fw) of pt_face2_vw                         feature 0
//     edge e, t from vertex e (pt_seg2_t's t; seg_seg2_st's s on A's edge (i, i+1) from vertex i, its t on B's edge):
//       edge 01: (t, 0);  edge 12: (1 - t, t);  edge 20: (0, 1 - t)              feature 1 + e; t == 0: vertex e; t == 1: vertex e + 1
//   q = (w X0 + u X1) + v X2 per coordinate with w = (1 - u) - v, on the ORIGINAL vertices, as pt_tri forms its q.
// Finite input gives no NaN.  Both points lie on their triangles: u, v >= 0 and u + v <= 1 up to the rounding of 1 - t.
// | |qa - qb| - dist | <= 2^-48 M, M the largest |coordinate| of the six vertices (measured: at most 2^-50.4 M over 1.2 M pairs --
// unit soups, near pairs, pairs offset by 1e6 and 2^40, integer-grid ties, slivers; tests/test_witness_ref.py re-checks it on every
// input the tests use).  Scaling all six vertices by 2^k scales dist, qa and qb exactly and changes nothing in the features or (u, v)
// over cd_find_proximity's band.  Restated in tests/witness_ref.py bit for bit.
struct TriWitness { double dist, ua, va, ub, vb; d3 qa, qb; uint32_t fa, fb; };
__device__ __forceinline__ d3 sel3(int i, const d3 a, const d3 b, const d3 c) { return i == 0 ? a : (i == 1 ? b : c); }
__device__ __forceinline__ void vertex_bary(int i, double &u, double &v, uint32_t &f) { u = i == 1 ? 1.0 : 0.0; v = i == 2 ? 1.0 : 0.0; f = 4u + (uint32_t)i; }
__device__ __forceinline__ void edge_bary(int e, double t, double &u, double &v, uint32_t &f)
{
    f = t > 0.0 ? (t < 1.0 ? 1u + (uint32_t)e : 4u + (uint32_t)(e == 2 ? 0 : e + 1)) : 4u + (uint32_t)e;
    u = e == 0 ? t : (e == 1 ? 1.0 - t : 0.0);
    v = e == 0 ? 0.0 : (e == 1 ? t : 1.0 - t);
}
__device__ __forceinline__ d3 bary_point(double u, double v, const d3 x0, const d3 x1, const d3 x2)
{
    const double w = (1.0 - u) - v;
    return d3{(w * x0.x + u * x1.x) + v * x2.x, (w * x0.y + u * x1.y) + v * x2.y, (w * x0.z + u * x1.z) + v * x2.z};
}
__device__ inline TriWitness tri_witness(const d3 P1, const d3 P2, const d3 P3, const d3 Q1, const d3 Q2, const d3 Q3)
{
    const d3 zero = d3{0.0, 0.0, 0.0};
    TriWitness r{0.0, 0.0, 0.0, 0.0, 0.0, zero, zero, 7u, 7u};
    if (box_overlap(box_set(P1, P2, P3), box_set(Q1, Q2, Q3)) && tri_contact_fast(P1, P2, P3, Q1, Q2, Q3)) return r;   // in contact: no witness
    d3 p2 = sub(P2, P1), p3 = sub(P3, P1), q1 = sub(Q1, P1), q2 = sub(Q2, P1), q3 = sub(Q3, P1);
    double m = 0.0;
    m = dmax_abs3(m, p2); m = dmax_abs3(m, p3); m = dmax_abs3(m, q1); m = dmax_abs3(m, q2); m = dmax_abs3(m, q3);
    if (!(m > 0.0)) return r;                                             // six coincident points
    int ex = (int)((__double_as_longlong(m) >> 52) & 0x7ff) - 1022;     // (as tri_distance)
    ex = ex < -TRI_DIST_EXP_MAX ? -TRI_DIST_EXP_MAX : (ex > TRI_DIST_EXP_MAX ? TRI_DIST_EXP_MAX : ex);
    const double sc = pow2(-ex);
    const d3 p1 = zero;
    p2 = dscale(p2, sc); p3 = dscale(p3, sc); q1 = dscale(q1, sc); q2 = dscale(q2, sc); q3 = dscale(q3, sc);
    // tri_distance's loop, keeping only which term won (the parameters of the other 32 are never formed)
    double best = __builtin_inf();
    int win = 0;
    auto take = [&](double d, int idx) { if (d < best) { best = d; win = idx; } };
#pragma unroll 1
    for (int i = 0; i < 3; ++i) {
        const d3 pi = sel3(i, p1, p2, p3), pn = sel3(i, p2, p3, p1), qi = sel3(i, q1, q2, q3);
        const int b = 11 * i;
        take(pt_face2(pi, q1, q2, q3), b);
        take(pt_face2(qi, p1, p2, p3), b + 1);
        take(pt_seg2(pi, q1, q2), b + 2); take(pt_seg2(pi, q2, q3), b + 3); take(pt_seg2(pi, q3, q1), b + 4);
        take(pt_seg2(qi, p1, p2), b + 5); take(pt_seg2(qi, p2, p3), b + 6); take(pt_seg2(qi, p3, p1), b + 7);
        take(seg_seg2(pi, pn, q1, q2), b + 8); take(seg_seg2(pi, pn, q2, q3), b + 9); take(seg_seg2(pi, pn, q3, q1), b + 10);
    }
    // the winning term once more, for its parameters
    const int i = win / 11, k = win - 11 * i;
    const d3 pi = sel3(i, p1, p2, p3), pn = sel3(i, p2, p3, p1), qi = sel3(i, q1, q2, q3);
    double t = 0.0, s = 0.0;
    if (k == 0) { vertex_bary(i, r.ua, r.va, r.fa); pt_face2_vw(pi, q1, q2, q3, r.ub, r.vb); r.fb = 0u; }
    else if (k == 1) { vertex_bary(i, r.ub, r.vb, r.fb); pt_face2_vw(qi, p1, p2, p3, r.ua, r.va); r.fa = 0u; }
    else if (k < 5) { const int e = k - 2; vertex_bary(i, r.ua, r.va, r.fa); pt_seg2_t(pi, sel3(e, q1, q2, q3), sel3(e, q2, q3, q1), t); edge_bary(e, t, r.ub, r.vb, r.fb); }
    else if (k < 8) { const int e = k - 5; vertex_bary(i, r.ub, r.vb, r.fb); pt_seg2_t(qi, sel3(e, p1, p2, p3), sel3(e, p2, p3, p1), t); edge_bary(e, t, r.ua, r.va, r.fa); }
    else { const int e = k - 8; seg_seg2_st(pi, pn, sel3(e, q1, q2, q3), sel3(e, q2, q3, q1), s, t); edge_bary(i, s, r.ua, r.va, r.fa); edge_bary(e, t, r.ub, r.vb, r.fb); }
    r.dist = __builtin_sqrt(best) * pow2(ex);
    r.qa = bary_point(r.ua, r.va, P1, P2, P3);
    r.qb = bary_point(r.ub, r.vb, Q1, Q2, Q3);
    return r;
}

__device__ __forceinline__ d3 load_vertex(const double *__restrict__ verts, uint32_t i)
{
    const double *p = verts + 3 * (size_t)i;
    return d3{p[0], p[1], p[2]};
}

// ---------------------------------------------------------------- ray against triangle (not reference behaviour)
// The ray o + t d, t in [0, tmax] (d not normalised: t is in units of d; 0 <= tmax <= +inf), against the triangle (p0, p1, p2), in
// FP64 with this operation order, IEEE divide, no contraction.  No face culling; det == 0 (a parallel ray, a degenerate triangle)
// is a miss; every comparison is written so that a NaN fails it, so any NaN on the way is a miss.
//   e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1 . pv, inv = 1 / det, tv = o - p0, qv = tv x e1,
//   u = (tv . pv) inv in [0, 1];  v = (d . qv) inv >= 0, u + v <= 1;  t = (e2 . qv) inv in [0, tmax];
//   gate: P_a = o_a + t d_a within [lo_a - G, hi_a + G] on every axis, lo / hi the triangle's box (box_set) and
//         G = 2^-30 max(|o_x|, |o_y|, |o_z|, the triangle's largest |coordinate|).
// The gate is to this predicate what the strict box overlap is to tri_distance: on a sliver the computed (t, u, v) can be rounding
// noise that passes the range checks at a point nowhere near the triangle; a hit the gate lets through has its computed point
// within G of the triangle's box, which is what lets the walk's box filter only filter (cd_rays.h).
// side = 1 when det > 0: the ray meets the face whose vertices run counter-clockwise as seen from the ray's origin.
// Band: scaling o, d and the triangle by 2^k scales nothing in (t, u, v) (t is scale-free when o and d scale together) while no
// nonzero intermediate -- products of up to three coordinate differences, so magnitudes around m^3 -- leaves the normal FP64 range:
// for inputs whose largest |coordinate| m is of order 1 .. 16 with features down to about 2^-20 m, |k| <= 300 (m within about
// 2^-300 .. 2^300; tests/test_ray_ref.py, tests/test_rays_gpu.py).  Outside it the result follows this arithmetic, overflow included.
constexpr double RAY_GATE = 1.0 / 1073741824.0;        // 2^-30
struct RayHit { bool hit; double t, u, v; uint32_t side; };
__device__ __forceinline__ RayHit ray_tri(const d3 o, const d3 d, const double tmax, const d3 p0, const d3 p1, const d3 p2)
{
    RayHit r{false, 0.0, 0.0, 0.0, 0u};
    const d3 e1 = sub(p1, p0), e2 = sub(p2, p0);
    const d3 pv = cross(d, e2);
    const double det = dot(e1, pv);
    if (!(det > 0.0 || det < 0.0)) return r;
    const double inv = 1.0 / det;
    const d3 tv = sub(o, p0);
    const double u = dot(tv, pv) * inv;
    if (!(u >= 0.0 && u <= 1.0)) return r;
    const d3 qv = cross(tv, e1);
    const double v = dot(d, qv) * inv;
    if (!(v >= 0.0 && u + v <= 1.0)) return r;
    const double t = dot(e2, qv) * inv;
    if (!(t >= 0.0 && t <= tmax)) return r;
    double m = 0.0;
    m = dmax_abs3(m, o); m = dmax_abs3(m, p0); m = dmax_abs3(m, p1); m = dmax_abs3(m, p2);
    const double G = RAY_GATE * m;
    const Box b = box_set(p0, p1, p2);
    const double Px = o.x + t * d.x, Py = o.y + t * d.y, Pz = o.z + t * d.z;
    if (!(b.x1 - G <= Px && Px <= b.x2 + G && b.y1 - G <= Py && Py <= b.y2 + G && b.z1 - G <= Pz && Pz <= b.z2 + G)) return r;
    r.hit = true; r.t = t; r.u = u; r.v = v; r.side = det > 0.0 ? 1u : 0u;
    return r;
}

// ---------------------------------------------------------------- the segment two triangles cut each other in (not reference behaviour)
// tri_isect(A, B): six ray_tri evaluations in a fixed order and a selection rule -- no arithmetic of its own beyond d = end - start,
// x = o + t d and the squared distance of two such points, all FP64, this operation order, no contraction; a NaN fails every comparison.
//   term k = 0, 1, 2: A's edge from A_k to A_(k+1 mod 3) against B's face (B0, B1, B2);
//   term k = 3, 4, 5: B's edge from B_(k-3) to B_(k-2 mod 3) against A's face (A0, A1, A2);
//   r_k = ray_tri(o, d, 1.0, p0, p1, p2) with o the edge's start and d = end - start per coordinate (one rounding); on a hit
//   x_k = o + t d per coordinate, the product rounded and then the sum: the P of ray_tri's gate.
//   mask: bit k set when term k hit.
//   No hit: n = 0, both terms 7, everything else 0 (coplanar pairs; touching pairs the gate or the range checks reject; degenerate triangles).
//   One hit: n = 1, endpoint 0 is that term, endpoint 1 has term 7 and zeros.
//   Two or more: n = 2.  The pairs (i, j), i < j, of hit terms are taken in lexicographic order with D = (dx dx + dy dy) + dz dz of
//   x_i - x_j; a later pair replaces the kept one only when its D is STRICTLY larger (an earlier pair keeps a tie; a NaN D never replaces).
//   Endpoint 0 is i, endpoint 1 is j.  With exactly two hits these are the two hits in term order.
//   Per endpoint: the term (0..5), ray_tri's t (along the piercing edge from its start), (u, v) (barycentrics on the pierced face), side, x.
// Properties (tests/test_isect_ref.py on the numpy restatement, tests/test_contour_gpu.py bit for bit on this code):
//   Finite input gives no NaN in any output (a hit has passed ray_tri's comparisons, so t, u, v are numbers and t is in [0, 1]).
//   Scaling all six vertices by 2^k scales x exactly and changes nothing else while the coordinates stay inside ray_tri's band.
//   tri_isect(B, A) hits exactly the terms (k + 3) mod 6 with bit-identical t, u, v, side, x -- each term is the same ray_tri call; only
//   the order of the two endpoints may differ.
//   Both endpoints lie on both triangles within 2^-42 M, M the pair's largest |coordinate| -- a condition on the inputs, as the witness's
//   bound: measured on the restatement over every input the tests use (worst 2^-44.58 M, on a sliver).
// The six terms are evaluated once for their points and the two winners once more for their parameters (the same call on the same
// operands: the same bits), which keeps the six terms' t, u, v out of the registers.
constexpr uint32_t ISECT_NONE = 7u;
struct IsectEnd { uint32_t term, side; double t, u, v; d3 x; };
struct TriIsect { uint32_t n, mask; IsectEnd e[2]; };
__device__ __forceinline__ d3 isect_sel3(int i, const d3 a, const d3 b, const d3 c) { return i == 0 ? a : (i == 1 ? b : c); }
// term k of tri_isect: hit, t, u, v, side from ray_tri; x = o + t d (zeros on a miss).  (One ray_tri for both sides: the operands are
// picked by k, a constant in tri_isect's unrolled loop and a run-time value for the two winners.)
__device__ __forceinline__ RayHit isect_term(uint32_t k, const d3 A0, const d3 A1, const d3 A2, const d3 B0, const d3 B1, const d3 B2, d3 &x)
{
    const bool ea = k < 3u;
    const int i = (int)(ea ? k : k - 3u), j = i == 2 ? 0 : i + 1;
    const d3 o = ea ? isect_sel3(i, A0, A1, A2) : isect_sel3(i, B0, B1, B2);
    const d3 e = ea ? isect_sel3(j, A0, A1, A2) : isect_sel3(j, B0, B1, B2);
    const d3 d = sub(e, o);
    const RayHit r = ray_tri(o, d, 1.0, ea ? B0 : A0, ea ? B1 : A1, ea ? B2 : A2);
    x = r.hit ? d3{o.x + r.t * d.x, o.y + r.t * d.y, o.z + r.t * d.z} : d3{0.0, 0.0, 0.0};
    return r;
}
__device__ __forceinline__ IsectEnd isect_end(uint32_t k, const d3 A0, const d3 A1, const d3 A2, const d3 B0, const d3 B1, const d3 B2)
{
    IsectEnd e{ISECT_NONE, 0u, 0.0, 0.0, 0.0, d3{0.0, 0.0, 0.0}};
    if (k == ISECT_NONE) return e;
    const RayHit r = isect_term(k, A0, A1, A2, B0, B1, B2, e.x);
    e.term = k; e.side = r.side; e.t = r.t; e.u = r.u; e.v = r.v;
    return e;
}
__device__ __forceinline__ TriIsect tri_isect(const d3 A0, const d3 A1, const d3 A2, const d3 B0, const d3 B1, const d3 B2)
{
    d3 x[6];
    uint32_t mask = 0u;
#pragma unroll
    for (int k = 0; k < 6; ++k) mask |= isect_term((uint32_t)k, A0, A1, A2, B0, B1, B2, x[k]).hit ? 1u << k : 0u;
    uint32_t e0 = ISECT_NONE, e1 = ISECT_NONE;
    bool have = false;
    double best = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i + 1; j < 6; ++j) {
            const bool both = ((mask >> i) & (mask >> j) & 1u) != 0u;
            const double dx = x[i].x - x[j].x, dy = x[i].y - x[j].y, dz = x[i].z - x[j].z;
            const double D = (dx * dx + dy * dy) + dz * dz;
            if (both && (!have || D > best)) { best = D; e0 = (uint32_t)i; e1 = (uint32_t)j; }
            have = have || both;
        }
    }
    const uint32_t nh = (uint32_t)__popc(mask);
    if (nh == 1u) e0 = (uint32_t)__ffs((int)mask) - 1u;
    TriIsect r;
    r.n = nh < 2u ? nh : 2u; r.mask = mask;
    r.e[0] = isect_end(e0, A0, A1, A2, B0, B1, B2);
    r.e[1] = isect_end(e1, A0, A1, A2, B0, B1, B2);
    return r;
}

// ---------------------------------------------------------------- point against triangle (not reference behaviour)
// pt_tri(p; p0, p1, p2): the distance from p to the triangle, the closest point q on it and where on the triangle q lies, in FP64 with
// this operation order, IEEE divide and sqrt, no contraction; tri_distance's blocks and tri_distance's frame, so its band (above):
//   a = p0 - p, b = p1 - p, c = p2 - p (the query point becomes the origin O);  m = the largest |component| of a, b, c;
//   m == 0 (three coincident vertices at p): dist = 0, u = v = 0, feature = 4, side = 0, q = p0;
//   else m = f 2^ex (f in [0.5, 1), |ex| clamped at 1000), a, b, c times 2^-ex (exact), and the minimum of four terms taken in this
//   order, a later term replacing an earlier one only when it is strictly smaller (an earlier term keeps a tie):
//     face     pt_face2_vw(O, a, b, c)         u = v_face, v = w_face                 feature 0
//     edge 01  pt_seg2_t(O, a, b) -> t         u = t,      v = 0                      feature 1; t == 0: 4 (vertex 0); t == 1: 5 (vertex 1)
//     edge 12  pt_seg2_t(O, b, c) -> t         u = 1 - t,  v = t                      feature 2; t == 0: 5;            t == 1: 6 (vertex 2)
//     edge 20  pt_seg2_t(O, c, a) -> t         u = 0,      v = 1 - t                  feature 3; t == 0: 6;            t == 1: 4
//   dist = sqrt(best) 2^ex;   side = (O - a) . ((b - a) x (c - a)) > 0, on the scaled operands;
//   q_k = (w p0_k + u p1_k) + v p2_k with w = (1 - u) - v, on the ORIGINAL vertices, per coordinate k.
// (u, v) are the barycentrics of q: q = (1 - u - v) p0 + u p1 + v p2; on an edge or a vertex they are the 0 / t / 1 - t the term implies
// (a clamped t may be -0.0: it compares equal to 0).  feature 0 means the face term won: the projection onto the plane lies in the
// CLOSED triangle, so a point whose projection falls exactly on an edge reports 0, not the edge.  A face whose barycentric denominator
// is not > 0 contributes +inf, so a degenerate triangle has the distance of the segment or point it is, from its edges' terms.
// side = 1: p lies on the side of the triangle's PLANE that sees the vertices counter-clockwise.  On an edge or vertex feature this is
// NOT an inside / outside test of a closed surface (the neighbouring face may see p from its other side).
// Finite input gives no NaN: every division has a denominator > 0 and the scaled operands lie in [-1, 1].  Non-finite vertices: undefined.
struct PtTri { double dist, u, v; d3 q; uint32_t feature, side; };
__device__ __forceinline__ PtTri pt_tri(const d3 p, const d3 p0, const d3 p1, const d3 p2)
{
    PtTri r{0.0, 0.0, 0.0, p0, 4u, 0u};
    d3 a = sub(p0, p), b = sub(p1, p), c = sub(p2, p);
    double m = 0.0;
    m = dmax_abs3(m, a); m = dmax_abs3(m, b); m = dmax_abs3(m, c);
    if (!(m > 0.0)) return r;
    int ex = (int)((__double_as_longlong(m) >> 52) & 0x7ff) - 1022;     // m = f 2^ex, f in [0.5, 1) (as tri_distance)
    ex = ex < -TRI_DIST_EXP_MAX ? -TRI_DIST_EXP_MAX : (ex > TRI_DIST_EXP_MAX ? TRI_DIST_EXP_MAX : ex);
    const double sc = pow2(-ex);
    a = dscale(a, sc); b = dscale(b, sc); c = dscale(c, sc);
    const d3 o = d3{0.0, 0.0, 0.0};
    double u, v, t;
    double best = pt_face2_vw(o, a, b, c, u, v);
    uint32_t f = 0u;
    double d = pt_seg2_t(o, a, b, t);
    if (d < best) { best = d; u = t; v = 0.0; f = t > 0.0 ? (t < 1.0 ? 1u : 5u) : 4u; }
    d = pt_seg2_t(o, b, c, t);
    if (d < best) { best = d; u = 1.0 - t; v = t; f = t > 0.0 ? (t < 1.0 ? 2u : 6u) : 5u; }
    d = pt_seg2_t(o, c, a, t);
    if (d < best) { best = d; u = 0.0; v = 1.0 - t; f = t > 0.0 ? (t < 1.0 ? 3u : 4u) : 6u; }
    r.side = dot(sub(o, a), cross(sub(b, a), sub(c, a))) > 0.0 ? 1u : 0u;
    r.dist = __builtin_sqrt(best) * pow2(ex);
    r.u = u; r.v = v; r.feature = f;
    const double w = (1.0 - u) - v;
    r.q = d3{(w * p0.x + u * p1.x) + v * p2.x, (w * p0.y + u * p1.y) + v * p2.y, (w * p0.z + u * p1.z) + v * p2.z};
    return r;
}

// ---------------------------------------------------------------- segment against triangle (not reference behaviour)
// seg_tri(a, b; p0, p1, p2): the distance from the segment a + s (b - a), s in [0, 1], to the triangle, the two closest points and where
// on the segment and on the triangle they lie.  FP64 with this operation order, IEEE divide and sqrt, no contraction.
//   d = b - a per coordinate (one rounding).
//   1. Crossing: h = ray_tri(a, d, 1.0, p0, p1, p2), the call tri_isect makes for an edge.  On a hit cross = 1, dist = 0, s = h.t,
//      (u, v) = (h.u, h.v), feature = 0, side = h.side, qs = a + s d per coordinate (the product rounded, then the sum: the P of
//      ray_tri's gate), qt = bary_point(u, v, p0, p1, p2).  An all-zero d has det == 0 and misses by ray_tri's own arithmetic.
//   2. Otherwise cross = 0, in tri_distance's frame translated to a:  B = b - a (= d), T_i = p_i - a;  m = the largest |component| of
//      B, T0, T1, T2;  m == 0 (five coincident points): pt_tri's all-coincident result -- dist 0, s = u = v = 0, feature 4, end 1,
//      side 0, qs = a, qt = p0;  else m = f 2^ex (f in [0.5, 1), |ex| clamped at TRI_DIST_EXP_MAX), B and T_i times 2^-ex (exact),
//      A = O the origin, and the minimum of 14 squared distances taken in this order, a later term replacing the running minimum only
//      when it is STRICTLY smaller (an earlier term keeps a tie):
//        k = 0          pt_face2_vw(A; T)                          s = 0               the face, (u, v) = (fv, fw), feature 0
//        k = 1, 2, 3    pt_seg2_t(A; T's edges 01, 12, 20)         s = 0               edge_bary(k - 1, t)
//        k = 4          pt_face2_vw(B; T)                          s = 1               the face
//        k = 5, 6, 7    pt_seg2_t(B; edges)                        s = 1               edge_bary(k - 5, t)
//        k = 8, 9, 10   pt_seg2_t(T_(k-8); A, B)                   s = its clamped t   vertex_bary(k - 8)
//        k = 11, 12, 13 seg_seg2_st(A, B; edge k - 11)             s = its s           edge_bary(k - 11, its t)
//      When d is all-zero ONLY terms 0..3 are taken: they are pt_tri(a)'s four terms in pt_tri's order and frame (B = 0 adds nothing
//      to m), so a segment with a == b is pt_tri(a) bit for bit -- dist, (u, v), feature, side, qt -- by construction.
//      dist = sqrt(best) 2^ex;  side = (O - T0) . ((T1 - T0) x (T2 - T0)) > 0 on the scaled operands: pt_tri's side of endpoint a;
//      qs = a for s == 0, b for s == 1, else a + s d;  qt = bary_point(u, v, p0, p1, p2) on the ORIGINAL vertices.
//   end = 1 when s == 0, 2 when s == 1, else 0 (both branches; a clamped s may be -0.0: it compares equal to 0).
// As in tri_witness only WHICH term won is kept; the winner is evaluated once more for its parameters (the same call on the same
// operands: the same bits), and the term loop stays rolled (tri_distance's comment: unrolled, every term's operands are live at once).
// The 14 terms are complete.  A closest pair (x on the segment, y on the triangle) without a crossing: if x is a segment end, terms
// 0..7 hold it (the end against the face's interior projection and the three edges, which cover the closed triangle); if y lies on the
// triangle's boundary and x inside the segment, y is on an edge and the pair is that edge's against the segment -- its interior
// critical point (11..13) or an end of one of the two, which is a vertex against the segment (8..10) or a segment end again; if x is
// inside the segment AND y inside the face, x - y is normal to the plane and to d, so the segment is parallel to the plane there and
// the pair slides along d, at the same distance, until x reaches a segment end or y the boundary: a case above.
// Band: ray_tri's (about 2^-300 .. 2^300), because the crossing term is ray_tri.  Finite input gives no NaN: a hit has passed ray_tri's
// comparisons, every division of the distance terms has a denominator > 0 and the scaled operands lie in [-1, 1].  A triangle of no
// area (ray_tri: det == 0, a miss; pt_face2: +inf) gets the distance of the segment or point it is, from its edges' terms.  A crossing's
// two points are ray_tri's: within rounding of the face's plane, or through a sliver, they carry its noise.
// dist is never above the true distance by more than rounding and never below it by more than a few 2^-52 M (every term is |P - Q|^2
// of two points on the two sets up to the rounding of forming them).  Restated in tests/segment_ref.py bit for bit.
struct SegTri { double dist, s, u, v; d3 qs, qt; uint32_t feature, end, cross, side; };
// term k on the scaled operands (A = O): the squared distance and the term's one or two parameters
__device__ __forceinline__ double seg_tri_term(int k, const d3 B, const d3 t0, const d3 t1, const d3 t2, double &p, double &q)
{
    const d3 O = d3{0.0, 0.0, 0.0};
    p = 0.0; q = 0.0;
    if (k >= 11) { const int e = k - 11; return seg_seg2_st(O, B, sel3(e, t0, t1, t2), sel3(e, t1, t2, t0), p, q); }
    const bool ends = k < 8;
    if (ends && (k & 3) == 0) return pt_face2_vw(k == 0 ? O : B, t0, t1, t2, p, q);
    const int e = ends ? (k & 3) - 1 : k - 8;
    const d3 te = sel3(e, t0, t1, t2);
    return pt_seg2_t(ends ? (k < 4 ? O : B) : te, ends ? te : O, ends ? sel3(e, t1, t2, t0) : B, p);
}
__device__ inline SegTri seg_tri(const d3 a, const d3 b, const d3 p0, const d3 p1, const d3 p2)
{
    const d3 zero = d3{0.0, 0.0, 0.0};
    SegTri r{0.0, 0.0, 0.0, 0.0, a, p0, 4u, 1u, 0u, 0u};
    const d3 d = sub(b, a);
    const RayHit h = ray_tri(a, d, 1.0, p0, p1, p2);
    if (h.hit) {
        r.s = h.t; r.u = h.u; r.v = h.v; r.feature = 0u; r.cross = 1u; r.side = h.side;
        r.end = h.t == 0.0 ? 1u : (h.t == 1.0 ? 2u : 0u);
        r.qs = d3{a.x + h.t * d.x, a.y + h.t * d.y, a.z + h.t * d.z};
        r.qt = bary_point(h.u, h.v, p0, p1, p2);
        return r;
    }
    d3 B = d, t0 = sub(p0, a), t1 = sub(p1, a), t2 = sub(p2, a);
    double m = 0.0;
    m = dmax_abs3(m, B); m = dmax_abs3(m, t0); m = dmax_abs3(m, t1); m = dmax_abs3(m, t2);
    if (!(m > 0.0)) return r;                                             // five coincident points
    int ex = (int)((__double_as_longlong(m) >> 52) & 0x7ff) - 1022;     // m = f 2^ex, f in [0.5, 1) (as tri_distance)
    ex = ex < -TRI_DIST_EXP_MAX ? -TRI_DIST_EXP_MAX : (ex > TRI_DIST_EXP_MAX ? TRI_DIST_EXP_MAX : ex);
    const double sc = pow2(-ex);
    B = dscale(B, sc); t0 = dscale(t0, sc); t1 = dscale(t1, sc); t2 = dscale(t2, sc);
    const int nterms = (d.x == 0.0 && d.y == 0.0 && d.z == 0.0) ? 4 : 14;
    double best = __builtin_inf(), p, q;
    int win = 0;
#pragma unroll 1
    for (int k = 0; k < nterms; ++k) {
        const double x = seg_tri_term(k, B, t0, t1, t2, p, q);
        if (x < best) { best = x; win = k; }
    }
    seg_tri_term(win, B, t0, t1, t2, p, q);                               // the winning term once more, for its parameters
    double s = win < 4 ? 0.0 : 1.0;
    if (win >= 11) { s = p; edge_bary(win - 11, q, r.u, r.v, r.feature); }
    else if (win >= 8) { s = p; vertex_bary(win - 8, r.u, r.v, r.feature); }
    else if ((win & 3) == 0) { r.u = p; r.v = q; r.feature = 0u; }
    else edge_bary((win & 3) - 1, p, r.u, r.v, r.feature);
    r.s = s;
    r.end = s == 0.0 ? 1u : (s == 1.0 ? 2u : 0u);
    r.side = dot(sub(zero, t0), cross(sub(t1, t0), sub(t2, t0))) > 0.0 ? 1u : 0u;
    r.dist = __builtin_sqrt(best) * pow2(ex);
    r.qs = r.end == 1u ? a : (r.end == 2u ? b : d3{a.x + s * d.x, a.y + s * d.y, a.z + s * d.z});
    r.qt = bary_point(r.u, r.v, p0, p1, p2);
    return r;
}

// ---------------------------------------------------------------- column against triangle (not reference behaviour)
// column_tri(p, c; v0, v1, v2): does the line through p parallel to axis c (the COLUMN) cross the triangle, with which orientation, and
// above or below p?  FP64 with this operation order, no contraction; every difference, product and sum is rounded on its own.
// With a = (c + 1) % 3, b = (c + 2) % 3 the triangle is projected onto the (a, b) plane:
//   gate : p_a within [min, max] of the three v_a and p_b within those of v_b, CLOSED, exact comparisons of the inputs; else no cover.
//   edge l -> h : la = l_a - p_a, lb = l_b - p_b, ha = h_a - p_a, hb = h_b - p_b, E = la hb - lb ha  (swapping l and h negates E exactly:
//          the two faces on a shared edge see opposite values, with no canonical order of the edge's ends);
//          E0 = E(v1 -> v2), E1 = E(v2 -> v0), E2 = E(v0 -> v1): E_i over their sum is v_i's barycentric weight of p's projection.
//   sign of an edge: the sign of E where E != 0; else the sign of l_b - h_b (the ORIGINAL coordinates, an exact comparison); else the
//          sign of h_a - l_a; else 0.  That is the sign E would have with p moved by (eps, eps^2) in (a, b), eps > 0 as small as needed:
//          E(p + (eps, eps^2)) = E + eps (l_b - h_b) + eps^2 (h_a - l_a).  The moved point lies on no edge and under no vertex, so of
//          the faces around an edge or a vertex under p exactly those it really lies under cover: ONE owner per crossing of a surface.
//   cover: o = +1 when the three signs are +, o = -1 when they are -, else 0 (a face whose projection is a line or a point has two
//          edges of opposite sign, or a 0: it never covers).
//   height: z_i = v_i,c - p_c, S = (E0 + E1) + E2, zc = (E0 z0 + E1 z1) + E2 z2: zc / S is the face's height over p on the column.
//          S == 0: not counted.  above when (zc > 0 and S > 0) or (zc < 0 and S < 0); else below -- zc == 0 (p on the face) is below.
// Every comparison is written so that a NaN fails it: a NaN in E gives the sign 0, a NaN in S or zc a face that is not counted.
// Where every computed E has its true sign or is a true zero the result is exactly the moved point's; a wrong sign -- possible only
// for a point within rounding of an edge's projection -- can put a count off by one.  Exact (adaptive) arithmetic is not attempted.
// Scaling p and the triangle by 2^k changes nothing while no nonzero product or sum leaves the normal range.
struct ColumnTri { int o; bool counted, above; double e0, e1, e2, zc, s; };
__device__ __forceinline__ double axis3(const d3 v, const int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }
__device__ __forceinline__ int column_edge_sign(const double la, const double lb, const double ha, const double hb, const double pa, const double pb, double &E)
{
    const double dla = la - pa, dlb = lb - pb, dha = ha - pa, dhb = hb - pb;
    E = dla * dhb - dlb * dha;
    if (E > 0.0) return 1;
    if (E < 0.0) return -1;
    if (!(E == 0.0)) return 0;
    if (lb > hb) return 1;
    if (lb < hb) return -1;
    if (ha > la) return 1;
    if (ha < la) return -1;
    return 0;
}
__device__ __forceinline__ ColumnTri column_tri(const d3 p, const int c, const d3 v0, const d3 v1, const d3 v2)
{
    ColumnTri r{0, false, false, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int a = c == 2 ? 0 : c + 1, b = c == 0 ? 2 : c - 1;
    const double pa = axis3(p, a), pb = axis3(p, b);
    const double a0 = axis3(v0, a), a1 = axis3(v1, a), a2 = axis3(v2, a), b0 = axis3(v0, b), b1 = axis3(v1, b), b2 = axis3(v2, b);
    // min <= p <= max without forming min and max: a NaN vertex coordinate takes no part here (its edges' E are NaN: no cover)
    const bool gate = (a0 <= pa || a1 <= pa || a2 <= pa) && (a0 >= pa || a1 >= pa || a2 >= pa) && (b0 <= pb || b1 <= pb || b2 <= pb) && (b0 >= pb || b1 >= pb || b2 >= pb);
    const int s0 = column_edge_sign(a1, b1, a2, b2, pa, pb, r.e0);
    const int s1 = column_edge_sign(a2, b2, a0, b0, pa, pb, r.e1);
    const int s2 = column_edge_sign(a0, b0, a1, b1, pa, pb, r.e2);
    const double pc = axis3(p, c);
    const double z0 = axis3(v0, c) - pc, z1 = axis3(v1, c) - pc, z2 = axis3(v2, c) - pc;
    r.s = (r.e0 + r.e1) + r.e2;
    r.zc = (r.e0 * z0 + r.e1 * z1) + r.e2 * z2;
    if (!gate) return r;
    r.o = (s0 > 0 && s1 > 0 && s2 > 0) ? 1 : ((s0 < 0 && s1 < 0 && s2 < 0) ? -1 : 0);
    r.counted = r.o != 0 && (r.s > 0.0 || r.s < 0.0) && r.zc == r.zc;
    r.above = r.counted && ((r.zc > 0.0 && r.s > 0.0) || (r.zc < 0.0 && r.s < 0.0));
    return r;
}

// ---------------------------------------------------------------- box against triangle (not reference behaviour)
// box_tri(box; p0, p1, p2): does the triangle meet the CLOSED axis-aligned box {x1, x2, y1, y2, z1, z2} (touching counts; lo == hi on
// an axis is allowed: a slab, a line, a point), and do all three vertices lie in it?  FP64 with this operation order, no contraction;
// every difference, product and sum is rounded on its own.  The separating-axis test of a box and a triangle in a fixed order:
//   1 gate  : per axis a = x, y, z, exact comparisons of the inputs: all three p_a < lo_a, or all three > hi_a: miss, code 1 + a.
//   2 inside: all nine coordinates in the closed box (exact comparisons): hit, inside = 1, code 0.  Nothing further is evaluated --
//             "a triangle wholly in the box is a hit" is a statement about comparisons, not about rounded arithmetic, and
//             cd_boxes_count's contained subtrees rest on it (cd_boxes.h).
//   2b vertex: any vertex in the closed box (exact comparisons): hit, inside = 0, code 0.  Nothing further is evaluated.  In exact
//             arithmetic steps 3 and 4 separate no such triangle, so this changes no true answer; in FP64 it keeps a box that TOUCHES
//             a vertex from losing the face to rounding.  A point box on vertex p1 has the true plane value d = n . (p0 - p1) = 0 and
//             r = 0, and the rounded d is nonzero for about a third of a mesh's faces (3250 of 10 000 in the 10 k soup), which step 4
//             would report as separated.
//   3 edges : c_a = 0.5 lo_a + 0.5 hi_a, h_a = 0.5 hi_a - 0.5 lo_a, v_i = p_i - c, f0 = p1 - p0, f1 = p2 - p1, f2 = p0 - p2 (the input
//             vertices).  Edge k = 0, 1, 2 and box axis j = 0, 1, 2 in lexicographic (k, j) order, a = (j + 1) % 3, b = (j + 2) % 3:
//             q_i = v_i[b] f_k[a] - v_i[a] f_k[b],  r = h[a] |f_k[b]| + h[b] |f_k[a]|;  all three q_i > r, or all three < -r: miss,
//             code 4 + 3 k + j.
//   4 plane : n = f0 x f1, d = (n_x v0_x + n_y v0_y) + n_z v0_z, r = (h_x |n_x| + h_y |n_y|) + h_z |n_z|;  d > r or d < -r: miss,
//             code 13.  Otherwise hit, inside = 0, code 0.
// A miss reports the FIRST separating test in this order: the code is part of the contract.  Every comparison is written so that a NaN
// separates nothing.  A degenerate triangle needs no special case: its zero edges and zero normal give 0 > 0, which is false, the
// remaining axes are the complete set for the segment it is, and the gate alone is exact for the point it is.
// Band: scaling box and triangle by 2^k changes nothing while no nonzero intermediate -- products of up to three coordinate
// differences, so magnitudes around m^3 -- leaves the normal FP64 range: as ray_tri's, for inputs whose largest |coordinate| m is of
// order 1 .. 16 with features down to about 2^-20 m, |k| <= 300.  Outside it the result follows this arithmetic, overflow included.
struct BoxTri { bool hit, inside; uint32_t code; };
// one edge axis: the three q and r of step 3 from the (a, b) coordinates; true: separated
__device__ __forceinline__ bool box_tri_axis(const double v0a, const double v0b, const double v1a, const double v1b, const double v2a, const double v2b,
                                             const double fa, const double fb, const double ha, const double hb)
{
    const double q0 = v0b * fa - v0a * fb, q1 = v1b * fa - v1a * fb, q2 = v2b * fa - v2a * fb;
    const double r = ha * dabs(fb) + hb * dabs(fa);
    const double nr = -r;
    return (q0 > r && q1 > r && q2 > r) || (q0 < nr && q1 < nr && q2 < nr);
}
__device__ __forceinline__ BoxTri box_tri(const Box &bx, const d3 p0, const d3 p1, const d3 p2)
{
    BoxTri t{false, false, 0u};
    if ((p0.x < bx.x1 && p1.x < bx.x1 && p2.x < bx.x1) || (p0.x > bx.x2 && p1.x > bx.x2 && p2.x > bx.x2)) { t.code = 1u; return t; }
    if ((p0.y < bx.y1 && p1.y < bx.y1 && p2.y < bx.y1) || (p0.y > bx.y2 && p1.y > bx.y2 && p2.y > bx.y2)) { t.code = 2u; return t; }
    if ((p0.z < bx.z1 && p1.z < bx.z1 && p2.z < bx.z1) || (p0.z > bx.z2 && p1.z > bx.z2 && p2.z > bx.z2)) { t.code = 3u; return t; }
    auto in = [&](const d3 p) { return bx.x1 <= p.x && p.x <= bx.x2 && bx.y1 <= p.y && p.y <= bx.y2 && bx.z1 <= p.z && p.z <= bx.z2; };
    const bool in0 = in(p0), in1 = in(p1), in2 = in(p2);
    if (in0 || in1 || in2) { t.hit = true; t.inside = in0 && in1 && in2; return t; }
    const d3 c{0.5 * bx.x1 + 0.5 * bx.x2, 0.5 * bx.y1 + 0.5 * bx.y2, 0.5 * bx.z1 + 0.5 * bx.z2};
    const d3 h{0.5 * bx.x2 - 0.5 * bx.x1, 0.5 * bx.y2 - 0.5 * bx.y1, 0.5 * bx.z2 - 0.5 * bx.z1};
    const d3 v0 = sub(p0, c), v1 = sub(p1, c), v2 = sub(p2, c);
    const d3 f0 = sub(p1, p0), f1 = sub(p2, p1), f2 = sub(p0, p2);
#define CD_BOX_TRI_EDGE(K, F)                                                                                                         \
    if (box_tri_axis(v0.y, v0.z, v1.y, v1.z, v2.y, v2.z, F.y, F.z, h.y, h.z)) { t.code = 4u + 3u * K; return t; }                     \
    if (box_tri_axis(v0.z, v0.x, v1.z, v1.x, v2.z, v2.x, F.z, F.x, h.z, h.x)) { t.code = 5u + 3u * K; return t; }                     \
    if (box_tri_axis(v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, F.x, F.y, h.x, h.y)) { t.code = 6u + 3u * K; return t; }
    CD_BOX_TRI_EDGE(0u, f0)
    CD_BOX_TRI_EDGE(1u, f1)
    CD_BOX_TRI_EDGE(2u, f2)
#undef CD_BOX_TRI_EDGE
    const d3 n = cross(f0, f1);
    const double d = (n.x * v0.x + n.y * v0.y) + n.z * v0.z;
    const double r = (h.x * dabs(n.x) + h.y * dabs(n.y)) + h.z * dabs(n.z);
    if (d > r || d < -r) { t.code = 13u; return t; }
    t.hit = true;
    return t;
}

// ---------------------------------------------------------------- plane against triangle (not reference behaviour)
// plane_tri(plane; p0, p1, p2): on which side of the plane {nx, ny, nz, d} -- the points with n . x = d; n need not be a unit vector --
// does the triangle lie, and if the plane cuts it, along which segment?  FP64 with this operation order, no contraction; every
// product, sum, difference and quotient is rounded on its own.
//   vertex : s_i = ((nx p_i.x + ny p_i.y) + nz p_i.z) - d  (plane_side).  Vertex i is BELOW iff s_i < 0; everything else -- s_i > 0, +-0,
//            a NaN -- is "not below".  The decision depends on the vertex and the plane alone.
//   class  : BELOW: all three vertices below.  ABOVE: none below (a face lying in the plane, or touching it from above, is ABOVE).
//            CUT: otherwise.
//   points : a CUT face has exactly two of its boundary edges e = 0 (p0 -> p1), 1 (p1 -> p2), 2 (p2 -> p0) whose ends differ in
//            "below".  For such an edge L is its below vertex and U the other one, whichever way the face runs through the edge.
//            s_U == 0: the point is U itself and t = 1.  Otherwise t = s_L / (s_L - s_U) and the point is L + t (U - L) per component
//            (difference, product, sum).  a is the point on the edge through which the boundary LEAVES "not below" (its first end is
//            not below, its second below), b the point on the edge through which it comes back; edge_a, edge_b, t_a, t_b go with them.
//   on     : bit i set iff s_i == 0.
// A face that is not CUT has a = b = (0, 0, 0), edges 0 and t = 0.
// What follows (DESIGN.md section 24 has the proofs):
//   - a point depends on (L, U, plane) alone, so the point of a shared edge is the same bits in both faces;
//   - on a closed, consistently oriented mesh every edge whose ends differ in "below" is an a-edge of one face and a b-edge of the
//     other: the multiset of a equals the multiset of b, the segments a -> b are closed loops, counter-clockwise seen from the tip of
//     n for an outward mesh, and  sum n . (a x b) / (2 |n|)  is the enclosed area;
//   - an edge lying in the plane is reported once, by the face below it (the face above it has no vertex below: ABOVE);
//   - a face below that touches the plane with one vertex is a row with a == b (both edges have that vertex as U, s_U == 0);
//   - every face has exactly one class: n_above + n_below + n_cut == n.
// Band: scaling plane (n kept, d scaled) and triangle by 2^k changes nothing -- classes, edges, t, on; a and b scale -- while no nonzero
// intermediate leaves the normal FP64 range.  The intermediates are products n_a p_a and their sums, so magnitudes around |n| m: as
// ray_tri's band, for |n| of order 1 and coordinates of order 1 .. 16, |k| <= 300.  Outside it the result follows this arithmetic.
constexpr uint32_t PLANE_ABOVE = 0u, PLANE_BELOW = 1u, PLANE_CUT = 2u;
struct Plane { double nx, ny, nz, d; };
struct PlaneTri { uint32_t cls, edge_a, edge_b, on; d3 a, b; double ta, tb; };
__device__ __forceinline__ double plane_side(const Plane &pl, const double x, const double y, const double z)
{
    return ((pl.nx * x + pl.ny * y) + pl.nz * z) - pl.d;
}
// the point of an edge whose ends differ in "below": L the below end (sl < 0), U the other one
__device__ __forceinline__ d3 plane_edge_point(const d3 L, const double sl, const d3 U, const double su, double &t)
{
    if (su == 0.0) { t = 1.0; return U; }
    t = sl / (sl - su);
    return d3{L.x + t * (U.x - L.x), L.y + t * (U.y - L.y), L.z + t * (U.z - L.z)};
}
__device__ __forceinline__ PlaneTri plane_tri(const Plane &pl, const d3 p0, const d3 p1, const d3 p2)
{
    PlaneTri r{PLANE_ABOVE, 0u, 0u, 0u, d3{0.0, 0.0, 0.0}, d3{0.0, 0.0, 0.0}, 0.0, 0.0};
    const double s0 = plane_side(pl, p0.x, p0.y, p0.z), s1 = plane_side(pl, p1.x, p1.y, p1.z), s2 = plane_side(pl, p2.x, p2.y, p2.z);
    const bool b0 = s0 < 0.0, b1 = s1 < 0.0, b2 = s2 < 0.0;
    r.on = (s0 == 0.0 ? 1u : 0u) | (s1 == 0.0 ? 2u : 0u) | (s2 == 0.0 ? 4u : 0u);
    if (b0 == b1 && b1 == b2) { r.cls = b0 ? PLANE_BELOW : PLANE_ABOVE; return r; }
    r.cls = PLANE_CUT;
    // the edge that leaves "not below" (first end not below, second below) and the edge that comes back
    if (!b0 && b1) { r.edge_a = 0u; r.a = plane_edge_point(p1, s1, p0, s0, r.ta); }
    else if (!b1 && b2) { r.edge_a = 1u; r.a = plane_edge_point(p2, s2, p1, s1, r.ta); }
    else { r.edge_a = 2u; r.a = plane_edge_point(p0, s0, p2, s2, r.ta); }
    if (b0 && !b1) { r.edge_b = 0u; r.b = plane_edge_point(p0, s0, p1, s1, r.tb); }
    else if (b1 && !b2) { r.edge_b = 1u; r.b = plane_edge_point(p1, s1, p2, s2, r.tb); }
    else { r.edge_b = 2u; r.b = plane_edge_point(p2, s2, p0, s0, r.tb); }
    return r;
}

// morton.h:7-29
__device__ __forceinline__ uint64_t expand64(uint64_t v)
{
    v &= 0x1fffffULL;
    v = (v | v << 32) & 0x1f00000000ffffULL;
    v = (v | v << 16) & 0x1f0000ff0000ffULL;
    v = (v | v << 8)  & 0x100f00f00f00f00fULL;
    v = (v | v << 4)  & 0x10c30c30c30c30c3ULL;
    v = (v | v << 2)  & 0x1249249249249249ULL;
    return v;
}
// double -> u64 of morton.h:80-82; negative / NaN -> 0, >= 2^63 -> 2^63-1 (undefined in the
// reference, defined here and identically in the oracle).
__device__ __forceinline__ uint64_t d2u64(double e)
{
    if (!(e > 0.0)) return 0;
    if (e >= 9223372036854775808.0) return 0x7fffffffffffffffULL;
    return (uint64_t)e;
}
// morton.h:70-89 with the frame as parameters
__device__ __forceinline__ uint64_t morton3d(double x, double y, double z, const double *off, const double *span)
{
    const double scale = 1048576.0;
    const double ex = ((x - off[0]) / span[0]) * scale;
    const double ey = ((y - off[1]) / span[1]) * scale;
    const double ez = ((z - off[2]) / span[2]) * scale;
    return (expand64(d2u64(ex)) << 2) | (expand64(d2u64(ey)) << 1) | expand64(d2u64(ez));
}

// ---------------------------------------------------------------- the ADAPTIVE frame (CD_FRAME_AUTO since round 6)
// Not reference behaviour: the reference has one frame, the constants of morton.h:43-58, and interleaves 20 bits an axis x, y, z
// (morton3d above: CD_FRAME_REFERENCE / CD_FRAME_CUSTOM, bit-identical to morton3D).  The pair set does not depend on the keys
// ("key freedom": a leaf is reached iff its own box overlaps the query's), the TREE does: per-axis normalisation of a
// 21 x 0.05 x 2.2 mesh (round 5's AUTO) gave cells of 400 : 1 and 44 node visits a query where this walks 29 (tools/sim/frame_study.py);
// an isotropic frame walks ~33 and leaves the thin axes' leading key bits constant -- the sort's 16 global bits (cd_sort.h) would hold 10
// that vary.  Here the 60 key bits are DEALT to the axes, all of them vary, and the cells of every level are as near to cubes as powers
// of two allow IN UNITS OF THE TRIANGLES' OWN EXTENT along each axis: a box query of size s meets a cell of length L with probability
// ~ (L + s); halving the cell along an axis costs (L + 2 s) / (L + s) -- least along the axis with the largest L / s, not the largest L.
// (A cloth is thin along one axis and so are its triangles: its sheets lie on top of each other there, and what separates them is worth a
// split early.  1 M cloth pair: 25.1 visits a query, the reference's hand-made frame 26.6, cubes by extent alone 30.9.)
//   statistic  per axis the mean of log2(box extent) over the triangles whose box is not flat on that axis, 8 fraction bits, piecewise
//              linear (flog2_fixed), summed as INTEGERS -- any order of summation gives the same sums, so this code and the oracle's
//              restatement (the CPU checker used by the tests) agree bit for bit;
//   E[a]       = flog2(extent of the centroids) + min(Lref - Lmean[a], LAYOUT_CAP): an axis whose triangles are thinner than those of the
//              axis where they are largest counts as longer by that ratio, at most 2^LAYOUT_CAP (every box flat on the axis: the cap);
//   layout     axes ordered by E, A >= B >= C (ties: the lower axis first); nA = round(E[A] - E[B]) leading bits split A alone,
//              nAB = round(E[B] - E[C]) pairs (A, B) follow, nABC triples (A, B, C) take the rest; one or two bits left over go to nA / nAB.
// layout word: bit 63 set | A | B << 2 | C << 4 | nA << 8 | nAB << 16 | nABC << 24;   0 = the reference's interleave.
constexpr unsigned long long LAYOUT_VALID = 1ull << 63;
constexpr int LAYOUT_CAP = 4;
constexpr double FLOG_MIN = 1e-300;                     // below this an extent counts as 0 (no subnormals in the statistic)
// 256 log2(x), piecewise linear between powers of two; x > 0 and normal
__device__ __forceinline__ long long flog2_fixed(double x)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (((long long)((u >> 52) & 0x7ffull) - 1023) << 8) + (long long)((u >> 44) & 0xffull);
}
// (written on scalars, no arrays: with E[ord[j]] indexed at run time this function alone took > 100 VGPRs and put k_morton at 127 with spills)
__device__ __forceinline__ long long layout_mean(long long sum, long long cnt, long long none)
{
    // floor of the mean, by ONE IEEE division of two exactly represented integers (|sum| < 2^53): the same on every machine, and a tenth of the instructions of a 64-bit integer division
    return cnt > 0 ? (long long)floor((double)sum / (double)cnt) : none;
}
__device__ inline unsigned long long frame_layout(const double lo[3], const double hi[3], const long long sum[3], const long long cnt[3])
{
    const long long NONE = -(1ll << 40), CAPF = (long long)LAYOUT_CAP << 8;
    const long long L0 = layout_mean(sum[0], cnt[0], NONE), L1 = layout_mean(sum[1], cnt[1], NONE), L2 = layout_mean(sum[2], cnt[2], NONE);
    long long Lref = L0 > L1 ? L0 : L1; Lref = L2 > Lref ? L2 : Lref;
    auto weight = [&](double e, long long Lm) -> long long {
        if (!(e > FLOG_MIN)) return NONE;
        long long d = CAPF;
        if (Lm != NONE) { d = Lref - Lm; if (d > CAPF) d = CAPF; }
        if (Lref == NONE) d = 0;                                              // every box flat on every axis: points
        return flog2_fixed(e) + d;
    };
    long long EA = weight(hi[0] - lo[0], L0), EB = weight(hi[1] - lo[1], L1), EC = weight(hi[2] - lo[2], L2);
    int A = 0, B = 1, C = 2;
    // stable, descending (an insertion sort of three: swap only on a strict '>', so ties keep the lower axis first)
    if (EB > EA) { const long long t = EA; EA = EB; EB = t; const int u = A; A = B; B = u; }
    if (EC > EB) { const long long t = EB; EB = EC; EC = t; const int u = B; B = C; C = u; }
    if (EB > EA) { const long long t = EA; EA = EB; EB = t; const int u = A; A = B; B = u; }
    long long nA = EA == NONE ? 0 : (EB == NONE ? 60 : (EA - EB + 128) >> 8);
    if (nA > 60) nA = 60;
    long long rem = 60 - nA;
    long long nAB = EB == NONE ? 0 : (EC == NONE ? 30 : (EB - EC + 128) >> 8);
    if (2 * nAB > rem) nAB = rem / 2;
    rem -= 2 * nAB;
    const long long nABC = rem / 3, left = rem % 3;
    if (left == 1) ++nA;
    if (left == 2) ++nAB;
    return LAYOUT_VALID | (unsigned long long)A | ((unsigned long long)B << 2) | ((unsigned long long)C << 4) |
           ((unsigned long long)nA << 8) | ((unsigned long long)nAB << 16) | ((unsigned long long)nABC << 24);
}
// is `w` a layout word morton3d_layout can take?  (0: the reference's interleave)
__host__ __device__ inline bool layout_ok(unsigned long long w)
{
    if (w == 0ull) return true;
    if (!(w >> 63) || ((w >> 32) & 0x7fffffffull) || ((w >> 6) & 3ull)) return false;
    const int A = (int)(w & 3), B = (int)((w >> 2) & 3), C = (int)((w >> 4) & 3), nA = (int)((w >> 8) & 255), p = (int)((w >> 16) & 255), t = (int)((w >> 24) & 255);
    return A < 3 && B < 3 && C < 3 && A != B && A != C && B != C && t <= 20 && p <= 30 && nA + 2 * p + 3 * t <= 60;
}
// spread the low 32 bits to the even positions
__device__ __forceinline__ uint64_t expand2(uint64_t v)
{
    v &= 0xffffffffULL;
    v = (v | v << 16) & 0x0000ffff0000ffffULL;
    v = (v | v << 8)  & 0x00ff00ff00ff00ffULL;
    v = (v | v << 4)  & 0x0f0f0f0f0f0f0f0fULL;
    v = (v | v << 2)  & 0x3333333333333333ULL;
    v = (v | v << 1)  & 0x5555555555555555ULL;
    return v;
}
// A layout word decoded once (wave-uniform: scalar registers) for a loop over keys.
// The cell of a triangle along axis a, in a frame WITH a layout, is   floor(((p1 + p2 + p3) - 3 off) * (2^bits / (3 span)))   clamped to [0, 2^bits - 1]:
// the vertex SUM against thrice the offset, times one factor per axis formed once per frame -- no division per key.  (morton.h's ((c - off) / span) * 2^20 on the
// centroid c = (p1 + p2 + p3) / 3 is six FP64 divisions a key, ~90 of the ~150 vector instructions k_morton<false> spends on one: they stay where the reference's
// bits are the contract, CD_FRAME_REFERENCE / CD_FRAME_CUSTOM.  Here the contract is this library's own -- the oracle restates it -- and the clamp makes it safe
// against the last cell's end whatever the rounding.)
struct KeyLayout {
    int A, B, C, t, p, nA;                              // t triples, p pairs, nA leading bits
    double off3A, off3B, off3C, kA, kB, kC;             // 3 off, 2^bits / (3 span)
    uint64_t topA, topB, topC;
};
// (a wave-uniform double into scalar registers: the compiler cannot see that a value read from LDS or through a pointer is uniform)
__device__ __forceinline__ double uniform_f64(double v)
{
    const long long b = __double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)b), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ KeyLayout key_layout(unsigned long long w, const double *off, const double *span)
{
    KeyLayout k;
    k.A = (int)(w & 3); k.B = (int)((w >> 2) & 3); k.C = (int)((w >> 4) & 3);
    k.nA = (int)((w >> 8) & 255); k.p = (int)((w >> 16) & 255); k.t = (int)((w >> 24) & 255);
    const int bA = k.nA + k.p + k.t, bB = k.p + k.t, bC = k.t;
    auto two_to = [](int b) { return __longlong_as_double((long long)(1023 + b) << 52); };                // 2^b, exact
    k.off3A = uniform_f64(3.0 * off[k.A]); k.off3B = uniform_f64(3.0 * off[k.B]); k.off3C = uniform_f64(3.0 * off[k.C]);
    k.kA = uniform_f64(two_to(bA) / (3.0 * span[k.A])); k.kB = uniform_f64(two_to(bB) / (3.0 * span[k.B])); k.kC = uniform_f64(two_to(bC) / (3.0 * span[k.C]));
    k.topA = (1ull << bA) - 1; k.topB = (1ull << bB) - 1; k.topC = (1ull << bC) - 1;
    return k;
}
// sx, sy, sz: the SUM of the triangle's three vertices per axis, p1 + p2 + p3 in that order (load_obj.h:90's numerator)
__device__ __forceinline__ uint64_t morton3d_layout(double sx, double sy, double sz, const KeyLayout &k)
{
    const double cA = k.A == 0 ? sx : (k.A == 1 ? sy : sz), cB = k.B == 0 ? sx : (k.B == 1 ? sy : sz), cC = k.C == 0 ? sx : (k.C == 1 ? sy : sz);
    uint64_t ia = d2u64((cA - k.off3A) * k.kA), ib = d2u64((cB - k.off3B) * k.kB), ic = d2u64((cC - k.off3C) * k.kC);
    ia = ia > k.topA ? k.topA : ia; ib = ib > k.topB ? k.topB : ib; ic = ic > k.topC ? k.topC : ic;   // a centroid beyond the frame takes the last cell: the key stays below 2^60
    const uint64_t mt = (1ull << k.t) - 1, mp = (1ull << k.p) - 1;
    const uint64_t triples = (expand64(ia & mt) << 2) | (expand64(ib & mt) << 1) | expand64(ic & mt);
    const uint64_t pairs = (expand2((ia >> k.t) & mp) << 1) | expand2((ib >> k.t) & mp);
    return ((ia >> (k.p + k.t)) << (2 * k.p + 3 * k.t)) | (pairs << (3 * k.t)) | triples;
}

}  // namespace cd
