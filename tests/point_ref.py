"""The closest-point queries restated on the CPU (no test in here): pt_tri in numpy, bit for bit as csrc/cd_math.h evaluates it; the
same in exact rational arithmetic; the closest triangle of points against ALL triangles of a mesh (no box filter of any kind); and the
operand sets the CPU and GPU tests share.

pt_tri (include/mi355cd.h): the point p against (p0, p1, p2):
    a = p0 - p, b = p1 - p, c = p2 - p; m = largest |component|; m == 0 -> dist 0, u = v = 0, feature 4, side 0, q = p0
    m = f 2^ex (frexp, |ex| clamped at 1000); a, b, c times 2^-ex; O = (0, 0, 0)
    best = face term pt_face2_vw(O, a, b, c) -> (u, v) = (fv, fw), feature 0
    then the edges (a, b), (b, c), (c, a) with pt_seg2_t(O, ., .) -> t, each replacing on strict '<' only:
        edge 01: u = t, v = 0 (feature 1; t == 0: 4; t == 1: 5)     edge 12: u = 1 - t, v = t (2; 5; 6)     edge 20: u = 0, v = 1 - t (3; 6; 4)
    dist = sqrt(best) 2^ex; side = (O - a) . ((b - a) x (c - a)) > 0; w = (1 - u) - v; q = (w p0 + u p1) + v p2 on the original vertices
Products are rounded one by one (numpy fuses nothing) and a dot product is (x x + y y) + z z.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

NONE = np.uint32(0xFFFFFFFF)
EXP_MAX = 1000          # cd_math.h TRI_DIST_EXP_MAX


# ---------------------------------------------------------------- FP64 restatement (tuples of broadcastable arrays, one per coordinate)
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _pt_seg2_t(p, a, b):
    ab, ap = _sub(b, a), _sub(p, a)
    den = _dot(ab, ab)
    pos = den > 0.0
    t = np.where(pos, _dot(ap, ab) / np.where(pos, den, 1.0), 0.0)
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    q = (a[0] + t * ab[0], a[1] + t * ab[1], a[2] + t * ab[2])
    d = _sub(p, q)
    return _dot(d, d), t


def _pt_face2_vw(p, a, b, c):
    ab, ac, ap = _sub(b, a), _sub(c, a), _sub(p, a)
    d00, d01, d11, d20, d21 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac), _dot(ap, ab), _dot(ap, ac)
    den = d00 * d11 - d01 * d01
    ok = den > 0.0
    dd = np.where(ok, den, 1.0)
    v = (d11 * d20 - d01 * d21) / dd
    w = (d00 * d21 - d01 * d20) / dd
    ok = ok & (v >= 0.0) & (w >= 0.0) & (v + w <= 1.0)
    q = ((a[0] + v * ab[0]) + w * ac[0], (a[1] + v * ab[1]) + w * ac[1], (a[2] + v * ab[2]) + w * ac[2])
    d = _sub(p, q)
    return np.where(ok, _dot(d, d), np.inf), np.where(ok, v, 0.0), np.where(ok, w, 0.0)


def _core(p, p0, p1, p2, full):
    """p, p0, p1, p2: tuples of three broadcastable arrays.  -> dist, or (dist, u, v, feature, side) with full."""
    a, b, c = _sub(p0, p), _sub(p1, p), _sub(p2, p)
    m = np.zeros(np.broadcast(a[0], a[1]).shape)
    for vec in (a, b, c):
        for k in range(3):
            x = np.abs(vec[k])
            m = np.where(x > m, x, m)
    ex = np.clip(np.frexp(m)[1], -EXP_MAX, EXP_MAX)
    sc = np.ldexp(1.0, -ex)
    a, b, c = (tuple(vec[k] * sc for k in range(3)) for vec in (a, b, c))
    zero = np.zeros_like(m)
    o = (zero, zero, zero)
    best, u, v = _pt_face2_vw(o, a, b, c)
    if full:
        f = np.zeros(m.shape, dtype=np.uint8)
    edges = ((a, b, (1, 5, 4)), (b, c, (2, 6, 5)), (c, a, (3, 4, 6)))
    for e, (x, y, (fe, f1, f0)) in enumerate(edges):
        d, t = _pt_seg2_t(o, x, y)
        rep = d < best
        best = np.where(rep, d, best)
        if full:
            eu, ev = ((t, zero), (1.0 - t, t), (zero, 1.0 - t))[e]
            u, v = np.where(rep, eu, u), np.where(rep, ev, v)
            f = np.where(rep, np.where(t > 0.0, np.where(t < 1.0, fe, f1), f0), f).astype(np.uint8)
    dist = np.where(m > 0.0, np.sqrt(best) * np.ldexp(1.0, ex), 0.0)
    if not full:
        return dist
    side = _dot(_sub(o, a), _cross(_sub(b, a), _sub(c, a))) > 0.0
    none = ~(m > 0.0)
    return dist, np.where(none, 0.0, u), np.where(none, 0.0, v), np.where(none, 4, f).astype(np.uint8), (side & ~none).astype(np.uint8)


def _cols(x):
    return tuple(x[..., k] for k in range(3))


def point_from_uv(u, v, tris):
    """q = (w p0 + u p1) + v p2 with w = (1 - u) - v, per coordinate: pt_tri's closest point from its barycentrics."""
    p = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    w = (1.0 - u) - v
    return (w[:, None] * p[:, 0] + u[:, None] * p[:, 1]) + v[:, None] * p[:, 2]


def pt_tri_np(points, tris):
    """points [n, 3], tris [n, 3, 3] -> (dist[n], q[n, 3], u[n], v[n], feature[n] uint8, side[n] uint8)."""
    pt = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    p = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        dist, u, v, f, side = _core(_cols(pt), _cols(p[:, 0]), _cols(p[:, 1]), _cols(p[:, 2]), True)
        q = point_from_uv(u, v, p)
    return dist, q, u, v, f, side


# ---------------------------------------------------------------- exact rationals
def exact_pt_tri(point, tri):
    """Exact: (d2, q, (u, v), feature, side, params).  d2: the squared distance; q: the closest point (for a degenerate triangle: a
    closest point); (u, v): its barycentrics, feature as pt_tri defines it (0 only in the OPEN face: all three barycentrics > 0);
    side: (p - p0) . n > 0; params: the unclamped quantities whose signs decide the feature -- the plane projection's three
    barycentrics (None for a degenerate triangle) and t, 1 - t of the three edges (None for a zero edge)."""
    pt = [Fraction(float(x)) for x in np.asarray(point, dtype=np.float64).reshape(3)]
    P = [[Fraction(float(x)) for x in row] for row in np.asarray(tri, dtype=np.float64).reshape(3, 3)]
    sub = lambda a, b: [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    at = lambda u, v: [(1 - u - v) * P[0][k] + u * P[1][k] + v * P[2][k] for k in range(3)]
    cands, params = [], []
    ab, ac, ap = sub(P[1], P[0]), sub(P[2], P[0]), sub(pt, P[0])
    d00, d01, d11, d20, d21 = dot(ab, ab), dot(ab, ac), dot(ac, ac), dot(ap, ab), dot(ap, ac)
    den = d00 * d11 - d01 * d01
    if den != 0:
        fv, fw = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        params += [fv, fw, 1 - fv - fw]
        if fv >= 0 and fw >= 0 and fv + fw <= 1:
            cands.append((fv, fw))
    else:
        params.append(None)
    for (i, j), uv in (((0, 1), lambda t: (t, Fraction(0))), ((1, 2), lambda t: (1 - t, t)), ((2, 0), lambda t: (Fraction(0), 1 - t))):
        e, w = sub(P[j], P[i]), sub(pt, P[i])
        ee = dot(e, e)
        if ee == 0:
            params.append(None)
            cands.append(uv(Fraction(0)))
            continue
        t = dot(w, e) / ee
        params += [t, 1 - t]
        cands.append(uv(min(max(t, Fraction(0)), Fraction(1))))
    best = None
    for (u, v) in cands:
        q = at(u, v)
        d = sub(pt, q)
        d2 = dot(d, d)
        if best is None or d2 < best[0]:
            best = (d2, q, (u, v))
    d2, q, (u, v) = best
    w = 1 - u - v
    zeros = (w == 0, u == 0, v == 0)
    feature = {(False, False, False): 0, (False, False, True): 1, (True, False, False): 2, (False, True, False): 3,
               (False, True, True): 4, (True, False, True): 5, (True, True, False): 6}[zeros]
    side = 1 if dot(ap, cross(ab, ac)) > 0 else 0
    return d2, q, (u, v), feature, side, params


# ---------------------------------------------------------------- the query
def closest_points_ref(verts, vidx, ids, points, rmax=np.inf, pairs_per_chunk=1 << 20, threads=8):
    """Every point against ALL triangles (chunks of points; no box filter of any kind), then per point, of the triangles with
    dist <= rmax, the smallest (dist, ID, face index).  -> (face[n] uint32 (NONE = 0xFFFFFFFF), ids[n], dist[n] (+inf when nothing
    is within rmax), closest[n, 3], uv[n, 2], feature[n] uint8, side[n] uint8), the outputs of cd_closest_points."""
    verts = np.asarray(verts, dtype=np.float64)
    vidx = np.asarray(vidx)
    nt = vidx.shape[0]
    ids = np.arange(nt, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    pt = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = pt.shape[0]
    rm = np.broadcast_to(np.asarray(rmax, dtype=np.float64), (n,))
    p = verts[vidx.astype(np.int64)]                                            # [T, 3, 3]
    T0, T1, T2 = (tuple(np.ascontiguousarray(p[:, j, k])[None, :] for k in range(3)) for j in range(3))
    key = (ids.astype(np.uint64) << np.uint64(32)) | np.arange(nt, dtype=np.uint64)     # (ID, face index)
    face = np.full(n, NONE, dtype=np.uint32)
    step = max(1, pairs_per_chunk // max(nt, 1))

    def work(a):
        b = min(n, a + step)
        with np.errstate(all="ignore"):
            d = _core(tuple(pt[a:b, k][:, None] for k in range(3)), T0, T1, T2, False)     # [b - a, T]
        d = np.where(d <= rm[a:b, None], d, np.inf)
        dmin = d.min(axis=1)
        k = np.where(d == dmin[:, None], key[None, :], np.uint64(0xFFFFFFFFFFFFFFFF)).argmin(axis=1)
        face[a:b] = np.where(np.isfinite(dmin), k.astype(np.uint32), NONE)

    starts = list(range(0, n, step))
    if threads > 1 and len(starts) > 1:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(work, starts))
    else:
        for a in starts:
            work(a)
    found = face != NONE
    f = np.where(found, face, 0).astype(np.int64)
    dist, q, u, v, feat, side = pt_tri_np(pt, p[f])                            # the winners again, with everything (the same bits)
    z = np.zeros(n)
    return (face, np.where(found, ids[f], 0).astype(np.uint32), np.where(found, dist, np.inf), np.where(found[:, None], q, 0.0),
            np.stack([np.where(found, u, z), np.where(found, v, z)], axis=1), np.where(found, feat, 0).astype(np.uint8),
            np.where(found, side, 0).astype(np.uint8))


# ---------------------------------------------------------------- operand sets
def _tri_frame(g, n):
    p = g.uniform(-1.0, 1.0, (n, 3, 3))
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    return p, e1, e2, np.cross(e1, e2)


def _bary_in(g, n):
    a, b = g.uniform(0.0, 1.0, n), g.uniform(0.0, 1.0, n)
    fl = a + b > 1.0
    return np.where(fl, 1 - a, a), np.where(fl, 1 - b, b)


WELL_CONDITIONED = ("random", "on_face", "on_edge", "on_vertex", "in_plane", "scaled")


def pair_classes(n, seed=0):
    """name -> (points [n, 3], tris [n, 3, 3]): the classes of (point, triangle) pairs the predicate is pinned on."""
    g = np.random.default_rng(seed)
    out = {}
    bary = lambda p, a, b: p[:, 0] + a[:, None] * (p[:, 1] - p[:, 0]) + b[:, None] * (p[:, 2] - p[:, 0])

    p, e1, e2, nrm = _tri_frame(g, n)
    out["random"] = (g.uniform(-2.0, 2.0, (n, 3)), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # on the face (up to the rounding of forming the point)
    out["on_face"] = (bary(p, *_bary_in(g, n)), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # on an edge: exact midpoints and rounded points
    k, s = g.integers(0, 3, n), np.where(g.random(n) < 0.5, 0.5, g.uniform(0.0, 1.0, n))
    x, y = p[np.arange(n), k], p[np.arange(n), (k + 1) % 3]
    out["on_edge"] = (x + s[:, None] * (y - x), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # exactly on a vertex, or beyond one (the vertex's region)
    k = g.integers(0, 3, n)
    x = p[np.arange(n), k]
    away = x - (p.sum(axis=1) - x) / 2.0                                        # from the opposite edge's midpoint through the vertex
    out["on_vertex"] = (x + away * (g.uniform(0.0, 1.0, n) * (g.random(n) < 0.5))[:, None], p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # in the plane, outside the triangle
    a, b = g.uniform(-2.0, 3.0, n), g.uniform(-2.0, 3.0, n)
    inside = (a >= 0) & (b >= 0) & (a + b <= 1)
    a = np.where(inside, a - 2.0, a)
    out["in_plane"] = (bary(p, a, b), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # slivers: the third vertex 2^-20 .. 2^-50 off an edge
    p[:, 2] = p[:, 0] + g.uniform(0, 1, n)[:, None] * e1 + nrm * (2.0 ** -g.uniform(20.0, 50.0, n))[:, None]
    near = g.random(n) < 0.5
    out["sliver"] = (np.where(near[:, None], bary(p, *_bary_in(g, n)) + nrm * g.uniform(-1e-3, 1e-3, n)[:, None], g.uniform(-2.0, 2.0, (n, 3))), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # segments and points
    k = g.integers(0, 4, n)
    p[k == 0, 2] = (p[:, 0] + g.uniform(-1, 2, n)[:, None] * e1)[k == 0]        # collinear (rounded)
    p[k == 1, 1] = p[k == 1, 0]                                                 # two vertices coincide
    p[k == 2, 1] = p[k == 2, 0]; p[k == 2, 2] = p[k == 2, 0]                    # a point
    p[k == 3, 2] = (0.5 * (p[:, 0] + p[:, 1]))[k == 3]                          # the midpoint
    pt = g.uniform(-2.0, 2.0, (n, 3))
    on = (k == 2) & (np.arange(n) % 4 == 0)
    pt[on] = p[on, 0]                                                           # three coincident vertices AT the point: dist = 0
    out["degenerate"] = (pt, p)

    pt0, p0 = out["random"]
    k = np.where(g.random(n) < 0.5, 100, -100)
    out["scaled"] = (np.ldexp(pt0, k[:, None]), np.ldexp(p0, k[:, None, None]))
    return out


def mesh_points(verts, vidx, n, seed=0, edge=None):
    """n points [n, 3] for a mesh, an eighth each: on the surface displaced along +- the normal by a small amount (up to a tenth of
    the triangle's edge) and by a large one (up to ten edges); exactly on vertices; exactly on edge midpoints and on faces (rounded
    centroids); midway between two random triangles' centroids (on the cloth pair: between the sheets, where ties live); inside the
    root box; and far outside it."""
    g = np.random.default_rng(seed)
    verts = np.asarray(verts, dtype=np.float64)
    p = verts[np.asarray(vidx).astype(np.int64)]
    nt = p.shape[0]
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3 * max(np.abs(verts).max(), 1e-300))
    m = n // 8
    pick = lambda k: p[g.integers(0, nt, k)]
    elen = lambda q: np.maximum(np.linalg.norm(q[:, 1] - q[:, 0], axis=1), np.linalg.norm(q[:, 2] - q[:, 0], axis=1))
    unit = lambda k: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(g.normal(size=(k, 3)))

    def normal(q):
        c = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
        l = np.linalg.norm(c, axis=1, keepdims=True)
        return np.where(l > 0, c / np.where(l > 0, l, 1.0), unit(q.shape[0]))

    def surface(q):
        a, b = _bary_in(g, q.shape[0])
        return q[:, 0] + a[:, None] * (q[:, 1] - q[:, 0]) + b[:, None] * (q[:, 2] - q[:, 0])

    sets = []
    q = pick(m); sets.append(surface(q) + normal(q) * (elen(q) * g.uniform(0.0, 0.1, m) * g.choice([-1.0, 1.0], m))[:, None])
    q = pick(m); sets.append(surface(q) + normal(q) * (elen(q) * g.uniform(0.1, 10.0, m) * g.choice([-1.0, 1.0], m))[:, None])
    q = pick(m); sets.append(q[np.arange(m), g.integers(0, 3, m)])
    q = pick(m); k = g.integers(0, 3, m)
    mid = 0.5 * (q[np.arange(m), k] + q[np.arange(m), (k + 1) % 3])
    sets.append(np.where((g.random(m) < 0.5)[:, None], mid, q.mean(axis=1)))
    sets.append(0.5 * (pick(m).mean(axis=1) + pick(m).mean(axis=1)))
    if edge is not None and nt > 1:                                             # half of them: midway between a triangle and one nearby in the list
        j = g.integers(0, nt, m)
        sets[-1] = np.where((g.random(m) < 0.5)[:, None], 0.5 * (p[j].mean(axis=1) + p[(j + nt // 2) % nt].mean(axis=1)), sets[-1])
    sets.append(lo + ext * g.random((m, 3)))
    sets.append(lo - 0.5 * ext + 2.0 * ext * g.random((m, 3)))
    k = n - 7 * m
    sets.append(0.5 * (lo + hi) + unit(k) * (np.linalg.norm(ext) * g.uniform(2.0, 100.0, k))[:, None])
    pts = np.concatenate(sets, axis=0)
    bad = ~np.isfinite(pts).all(axis=1)
    pts[bad] = lo
    return np.ascontiguousarray(pts)


def radii(dist_inf, edge, seed=0):
    """A finite radius per point such that a good share finds nothing, from the distances the rmax = +inf query gives: a quarter each
    0, U(0, edge), EXACTLY the nearest distance (the comparison is closed: found) and the nearest distance times U(0.5, 1.5)."""
    g = np.random.default_rng(seed)
    d = np.asarray(dist_inf, dtype=np.float64)
    n = d.shape[0]
    k = np.arange(n) % 4
    return np.select([k == 0, k == 1, k == 2], [np.zeros(n), g.uniform(0, edge, n), d], d * g.uniform(0.5, 1.5, n))
