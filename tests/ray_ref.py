"""The ray queries restated on the CPU (no test in here): ray_tri in numpy, bit for bit as csrc/cd_math.h evaluates it; the same in
exact rational arithmetic; the closest hit of rays against ALL triangles of a mesh (no box filter of any kind); and the operand sets
the CPU and GPU tests share.

ray_tri (include/mi355cd.h): the ray o + t d, t in [0, tmax], against (p0, p1, p2):
    e1 = p1 - p0, e2 = p2 - p0, pv = d x e2, det = e1 . pv            det == 0 -> miss
    inv = 1 / det, tv = o - p0, u = (tv . pv) inv                      u < 0 or u > 1 -> miss
    qv = tv x e1, v = (d . qv) inv                                     v < 0 or u + v > 1 -> miss
    t = (e2 . qv) inv                                                  t < 0 or t > tmax -> miss
    P = o + t d (two roundings an axis), G = 2^-30 max(|o|_inf, |p0|_inf, |p1|_inf, |p2|_inf)
    lo - G <= P <= hi + G on every axis (lo / hi: the triangle's box), else miss
    side = det > 0
Products are rounded one by one (numpy fuses nothing), a dot product is (x x + y y) + z z, and a NaN fails every comparison.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

MISS = np.uint32(0xFFFFFFFF)
GATE = 2.0 ** -30


def _cross(a, b):
    return (a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0])


def _dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _stage_u(o, d, p0, e1, e2):
    """Up to the u test, on broadcastable [..., 3] operands: (ok, det, inv, u, pv, tv)."""
    pvx, pvy, pvz = _cross(d, e2)
    det = _dot3(e1[..., 0], e1[..., 1], e1[..., 2], pvx, pvy, pvz)
    ok = (det > 0.0) | (det < 0.0)
    inv = 1.0 / det
    tv = o - p0
    u = _dot3(tv[..., 0], tv[..., 1], tv[..., 2], pvx, pvy, pvz) * inv
    ok &= (u >= 0.0) & (u <= 1.0)
    return ok, det, inv, u, tv


def _stage_rest(ok, det, inv, u, tv, o, d, tmax, e1, e2, lo, hi, mtri):
    """From qv on, elementwise on operands of one shape [n, 3] / [n]: (hit, t, v, side)."""
    qx, qy, qz = _cross(tv, e1)
    v = _dot3(d[..., 0], d[..., 1], d[..., 2], qx, qy, qz) * inv
    ok = ok & (v >= 0.0) & (u + v <= 1.0)
    t = _dot3(e2[..., 0], e2[..., 1], e2[..., 2], qx, qy, qz) * inv
    ok &= (t >= 0.0) & (t <= tmax)
    G = GATE * np.maximum(np.abs(o).max(axis=-1), mtri)
    P = o + t[..., None] * d
    ok &= ((lo - G[..., None] <= P) & (P <= hi + G[..., None])).all(axis=-1)
    return ok, t, v, det > 0.0


def ray_tri_np(rays, tris):
    """rays [n, 7] (o, d, tmax), tris [n, 3, 3] -> (hit[n] bool, t[n], u[n], v[n], side[n] uint8); t, u, v, side are 0 on a miss."""
    r = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    p = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    o, d, tmax = r[:, 0:3], r[:, 3:6], r[:, 6]
    p0 = p[:, 0]
    e1, e2 = p[:, 1] - p0, p[:, 2] - p0
    with np.errstate(all="ignore"):
        ok, det, inv, u, tv = _stage_u(o, d, p0, e1, e2)
        hit, t, v, side = _stage_rest(ok, det, inv, u, tv, o, d, tmax, e1, e2, p.min(axis=1), p.max(axis=1), np.abs(p).max(axis=(1, 2)))
    z = np.zeros_like(t)
    return hit, np.where(hit, t, z), np.where(hit, u, z), np.where(hit, v, z), (hit & side).astype(np.uint8)


def exact_ray_tri(ray, tri):
    """The same quantities in exact rational arithmetic, without the gate: (hit, t, u, v, det) as Fractions, or (False, None, None,
    None, det) when det == 0.  hit: det != 0, 0 <= u <= 1, v >= 0, u + v <= 1, 0 <= t <= tmax (tmax = +inf: no upper end)."""
    f = [Fraction(float(x)) for x in np.asarray(ray, dtype=np.float64).reshape(7)[:6]]
    tmax = float(np.asarray(ray, dtype=np.float64).reshape(7)[6])
    p = [[Fraction(float(x)) for x in row] for row in np.asarray(tri, dtype=np.float64).reshape(3, 3)]
    o, d = f[0:3], f[3:6]
    sub = lambda a, b: [a[0] - b[0], a[1] - b[1], a[2] - b[2]]
    cross = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    e1, e2 = sub(p[1], p[0]), sub(p[2], p[0])
    pv = cross(d, e2)
    det = dot(e1, pv)
    if det == 0:
        return False, None, None, None, det
    tv = sub(o, p[0])
    u = dot(tv, pv) / det
    qv = cross(tv, e1)
    v = dot(d, qv) / det
    t = dot(e2, qv) / det
    hit = 0 <= u <= 1 and v >= 0 and u + v <= 1 and t >= 0 and (tmax == np.inf or t <= Fraction(tmax))
    return hit, t, u, v, det


def cast_rays_ref(verts, vidx, ids, rays, pairs_per_chunk=1 << 22, threads=8):
    """Every ray against ALL triangles (chunks of rays; no box filter of any kind: only ray_tri's own early exits thin the pairs out),
    then the smallest (t, ID, face index) per ray.  -> (face[n] uint32 (MISS = 0xFFFFFFFF), ids[n], t[n] (+inf on a miss), uv[n, 2],
    side[n] uint8), the outputs of cd_cast_rays."""
    verts = np.asarray(verts, dtype=np.float64)
    vidx = np.asarray(vidx)
    nt = vidx.shape[0]
    ids = np.arange(nt, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    r = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = r.shape[0]
    p = verts[vidx.astype(np.int64)]                                            # [T, 3, 3]
    p0 = np.ascontiguousarray(p[:, 0])
    e1, e2 = p[:, 1] - p0, p[:, 2] - p0
    lo, hi, mtri = p.min(axis=1), p.max(axis=1), np.abs(p).max(axis=(1, 2))
    face = np.full(n, MISS, dtype=np.uint32)
    oid = np.zeros(n, dtype=np.uint32)
    ot = np.full(n, np.inf)
    ouv = np.zeros((n, 2))
    oside = np.zeros(n, dtype=np.uint8)
    step = max(1, pairs_per_chunk // max(nt, 1))

    def work(a):
        b = min(n, a + step)
        o, d, tmax = r[a:b, 0:3], r[a:b, 3:6], r[a:b, 6]
        with np.errstate(all="ignore"):
            ok, det, inv, u, tv = _stage_u(o[:, None, :], d[:, None, :], p0[None], e1[None], e2[None])
            ri, ti = np.nonzero(ok)
            if ri.size == 0:
                return
            hit, t, v, side = _stage_rest(ok[ri, ti], det[ri, ti], inv[ri, ti], u[ri, ti], tv[ri, ti], o[ri], d[ri], tmax[ri], e1[ti], e2[ti], lo[ti], hi[ti], mtri[ti])
        ri, ti, t, uu, v, side = ri[hit], ti[hit], t[hit], u[ri, ti][hit], v[hit], side[hit]
        if ri.size == 0:
            return
        order = np.lexsort((ti, ids[ti], t, ri))                                # by ray, then (t, ID, face index); -0.0 == 0.0
        first = order[np.unique(ri[order], return_index=True)[1]]
        k = a + ri[first]
        face[k] = ti[first].astype(np.uint32); oid[k] = ids[ti[first]]; ot[k] = t[first]
        ouv[k, 0] = uu[first]; ouv[k, 1] = v[first]; oside[k] = side[first].astype(np.uint8)

    starts = list(range(0, n, step))
    if threads > 1 and len(starts) > 1:
        with ThreadPoolExecutor(threads) as ex:
            list(ex.map(work, starts))
    else:
        for a in starts:
            work(a)
    return face, oid, ot, ouv, oside


# ---------------------------------------------------------------- operand sets
def _tri_frame(g, n):
    p = g.uniform(-1.0, 1.0, (n, 3, 3))
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nrm = np.cross(e1, e2)
    return p, e1, e2, nrm


def _tmax_mix(g, n, t_target=1.0):
    tm = np.full(n, np.inf)
    k = g.integers(0, 4, n)
    tt = np.broadcast_to(np.asarray(t_target, dtype=np.float64), (n,))
    tm[k == 1] = (tt * g.uniform(0.0, 2.0, n))[k == 1]
    tm[k == 2] = tt[k == 2]
    return tm


def _pack(o, d, tmax):
    r = np.empty((o.shape[0], 7))
    r[:, 0:3] = o; r[:, 3:6] = d; r[:, 6] = tmax
    return r


def pair_classes(n, seed=0):
    """name -> (rays [n, 7], tris [n, 3, 3]): the classes of (ray, triangle) pairs the predicate is pinned on."""
    g = np.random.default_rng(seed)
    out = {}
    bary = lambda p, a, b: p[:, 0] + a[:, None] * (p[:, 1] - p[:, 0]) + b[:, None] * (p[:, 2] - p[:, 0])

    p, e1, e2, nrm = _tri_frame(g, n)                                          # aimed at a point of the triangle's plane, half of them inside
    o = g.uniform(-2.0, 2.0, (n, 3))
    s = g.uniform(0.2, 3.0, n)
    d = (bary(p, g.uniform(-0.5, 1.5, n), g.uniform(-0.5, 1.5, n)) - o) * s[:, None]
    out["random"] = (_pack(o, d, _tmax_mix(g, n, 1.0 / s)), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # nearly parallel to the plane
    tgt = bary(p, g.uniform(0.0, 1.0, n), g.uniform(0.0, 1.0, n))
    w = e1 * g.uniform(-1, 1, n)[:, None] + e2 * g.uniform(-1, 1, n)[:, None]
    d = w + nrm * (2.0 ** -g.uniform(5.0, 40.0, n) * g.choice([-1.0, 1.0], n))[:, None]
    o = tgt - d * g.uniform(0.5, 2.0, n)[:, None]
    out["grazing"] = (_pack(o, d, np.inf), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # through a vertex or a point of an edge
    k = g.integers(0, 6, n)
    s = g.uniform(0.0, 1.0, n)
    a = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5], [0 * s, 1 + 0 * s, 0 * s, s, 0 * s, s])
    b = np.select([k == 0, k == 1, k == 2, k == 3, k == 4, k == 5], [0 * s, 0 * s, 1 + 0 * s, 0 * s, s, 1 - s])
    tgt = bary(p, a, b)
    o = g.uniform(-2.0, 2.0, (n, 3))
    out["vertex_edge"] = (_pack(o, tgt - o, _tmax_mix(g, n)), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # in the triangle's plane
    o = bary(p, g.uniform(-1.0, 2.0, n), g.uniform(-1.0, 2.0, n))
    d = e1 * g.uniform(-1, 1, n)[:, None] + e2 * g.uniform(-1, 1, n)[:, None]
    out["in_plane"] = (_pack(o, d, np.inf), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # segments, points, slivers
    k = g.integers(0, 4, n)
    p[k == 0, 2] = (p[:, 0] + g.uniform(-1, 2, n)[:, None] * e1)[k == 0]
    p[k == 1, 1] = p[k == 1, 0]
    p[k == 2, 1] = p[k == 2, 0]; p[k == 2, 2] = p[k == 2, 0]
    p[k == 3, 2] = (p[:, 0] + g.uniform(0, 1, n)[:, None] * e1 + nrm * (2.0 ** -g.uniform(20.0, 50.0, n))[:, None])[k == 3]
    o = g.uniform(-2.0, 2.0, (n, 3))
    tgt = p[:, 0] + g.uniform(0, 1, n)[:, None] * (p[:, 1] - p[:, 0])
    out["degenerate"] = (_pack(o, tgt - o, np.inf), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # exact zero direction components
    tgt = bary(p, g.uniform(-0.2, 1.2, n), g.uniform(-0.2, 1.2, n))
    d = g.uniform(-1.0, 1.0, (n, 3))
    z = g.integers(1, 7, n)                                                     # which components are zero (never all three)
    for ax in range(3):
        d[(z >> ax) & 1 == 1, ax] = 0.0
    d[z == 7] = [0.0, 0.0, 1.0]
    o = tgt - d * g.uniform(0.5, 2.0, n)[:, None]
    keep = g.random(n) < 0.5                                                    # half: o exactly on the axis line through the target
    o = np.where(keep[:, None], o, np.where(d == 0.0, tgt, o))
    out["axis"] = (_pack(o, d, _tmax_mix(g, n, 1.5)), p)

    p, e1, e2, nrm = _tri_frame(g, n)                                          # the origin ON the triangle: tmax = 0 and others
    k = g.integers(0, 3, n)
    a, b = g.uniform(0.0, 1.0, n), g.uniform(0.0, 1.0, n)
    fl = a + b > 1.0
    a, b = np.where(fl, 1 - a, a), np.where(fl, 1 - b, b)
    o = np.where((k == 0)[:, None], p[:, 0], bary(p, a, b))
    d = g.uniform(-1.0, 1.0, (n, 3))
    out["on_triangle"] = (_pack(o, d, np.where(g.random(n) < 0.5, 0.0, np.inf)), p)

    r0, p0 = out["random"]
    k = np.where(g.random(n) < 0.5, 100, -100)
    rs = r0.copy()
    rs[:, 0:6] = np.ldexp(r0[:, 0:6], k[:, None])
    out["scaled"] = (rs, np.ldexp(p0, k[:, None, None]))
    return out


def mesh_rays(verts, vidx, n, seed=0):
    """n rays [n, 7] for a mesh, an eighth each: random through the root box; axis-parallel with exact zero components; starting ON
    a triangle (a vertex: t = 0 exactly; or a point of its plane); starting inside leaf boxes; aimed along triangle edges (shared
    edges on a cloth); parallel to a triangle's plane (the cloth's, on a cloth); short segments that end just before / just behind a
    triangle's centre; long rays from outside aimed at triangle centres."""
    g = np.random.default_rng(seed)
    verts = np.asarray(verts, dtype=np.float64)
    p = verts[np.asarray(vidx).astype(np.int64)]
    nt = p.shape[0]
    lo, hi = verts.min(axis=0), verts.max(axis=0)
    ext = np.maximum(hi - lo, 1e-3 * max(np.abs(verts).max(), 1e-300))
    m = n // 8
    pick = lambda k: p[g.integers(0, nt, k)]
    unit = lambda k: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(g.normal(size=(k, 3)))
    edge = lambda q: np.maximum(np.linalg.norm(q[:, 1] - q[:, 0], axis=1), np.linalg.norm(q[:, 2] - q[:, 0], axis=1))
    normal = lambda q: (lambda c: c / np.maximum(np.linalg.norm(c, axis=1, keepdims=True), 1e-300))(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]))
    sets = []
    o = lo - 0.5 * ext + 2.0 * ext * g.random((m, 3))
    sets.append(_pack(o, lo + ext * g.random((m, 3)) - o, g.choice([np.inf, 1.0, 2.0, 0.5], m)))
    q = pick(m)                                                                 # axis-parallel, through or near a triangle's centre
    c = q.mean(axis=1) + (g.random((m, 3)) - 0.5) * edge(q)[:, None] * g.choice([0.0, 1.0], m)[:, None]
    ax = g.integers(0, 3, m)
    d = np.zeros((m, 3)); d[np.arange(m), ax] = g.choice([-1.0, 1.0], m) * ext[ax] * g.uniform(0.1, 2.0, m)
    sets.append(_pack(c - d * g.uniform(0.0, 1.5, m)[:, None], d, g.choice([np.inf, 1.0], m)))
    q = pick(m)                                                                 # ON a triangle
    a, b = g.uniform(0, 0.5, m), g.uniform(0, 0.5, m)
    o = np.where((g.random(m) < 0.5)[:, None], q[:, 0], q[:, 0] + a[:, None] * (q[:, 1] - q[:, 0]) + b[:, None] * (q[:, 2] - q[:, 0]))
    sets.append(_pack(o, unit(m) * edge(q)[:, None], g.choice([np.inf, 0.0, 1.0], m)))
    q = pick(m)                                                                 # inside leaf boxes
    o = q.min(axis=1) + (q.max(axis=1) - q.min(axis=1)) * g.random((m, 3))
    sets.append(_pack(o, unit(m) * ext.max(), np.inf))
    q = pick(m)                                                                 # along an edge
    e = q[:, 1] - q[:, 0]
    sets.append(_pack(q[:, 0] - 2.0 * e, e, g.choice([np.inf, 2.0, 3.0, 8.0], m)))
    q = pick(m)                                                                 # parallel to a triangle's plane, in it or just off it
    d = (q[:, 1] - q[:, 0]) * g.uniform(-1, 1, m)[:, None] + (q[:, 2] - q[:, 0]) * g.uniform(-1, 1, m)[:, None]
    off = normal(q) * (edge(q) * g.choice([0.0, 1e-9, -1e-9, 1e-3], m))[:, None]
    sets.append(_pack(q.mean(axis=1) + off - 4.0 * d, d, np.inf))
    q = pick(m)                                                                 # short segments ending just before / behind the centre
    h = normal(q) * (edge(q) * g.uniform(0.1, 1.0, m) * g.choice([-1.0, 1.0], m))[:, None]
    sets.append(_pack(q.mean(axis=1) + h, -h, g.choice([1.0 - 2.0 ** -20, 1.0 + 2.0 ** -20, 1.0], m)))
    k = n - 7 * m
    q = pick(k)
    o = lo - ext + 3.0 * ext * g.random((k, 3))
    sets.append(_pack(o, (q.mean(axis=1) - o) * g.uniform(0.5, 2.0, k)[:, None], np.inf))
    rays = np.concatenate(sets, axis=0)
    bad = ~np.isfinite(rays[:, 0:6]).all(axis=1) | (rays[:, 3:6] == 0.0).all(axis=1)       # (a degenerate triangle's edge: no direction)
    rays[bad, 0:3] = lo; rays[bad, 3:6] = ext; rays[bad, 6] = np.inf
    return np.ascontiguousarray(rays)


def pinhole(eye, target, up, fov_deg, res):
    """res x res rays of a pinhole camera, row by row (neighbouring pixels are neighbouring rays): [res * res, 7], tmax = +inf."""
    eye, target, up = (np.asarray(x, dtype=np.float64) for x in (eye, target, up))
    w = target - eye; w /= np.linalg.norm(w)
    uu = np.cross(w, up); uu /= np.linalg.norm(uu)
    vv = np.cross(uu, w)
    s = np.tan(np.radians(fov_deg) / 2.0)
    c = ((np.arange(res) + 0.5) / res * 2.0 - 1.0) * s
    d = w[None, None, :] + c[None, :, None] * uu[None, None, :] - c[:, None, None] * vv[None, None, :]
    return _pack(np.broadcast_to(eye, (res * res, 3)), d.reshape(-1, 3), np.inf)
