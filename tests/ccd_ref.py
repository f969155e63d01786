"""CPU restatement of the continuous collision query (include/mi355cd.h cd_find_ccd / cd_ccd_points; csrc/cd_ccd.h ccd_advance).

advance_np restates the device's conservative advancement operation for operation (numpy float64, no contraction, correctly rounded
divide and sqrt) on top of proximity_ref.tri_distance_np, so toi, the distance and the evaluation count agree bit for bit.
ccd_pairs enumerates candidates on its own, without the device's tree -- every pair of a mesh of up to proximity_ref.BRUTE_MAX
triangles, else a uniform grid over the swept boxes widened far beyond what the gate needs -- and applies the same definition:
neighbour filter, the FP64 swept-box gate, the advancement.
exact_dist2 is the exact rational squared distance of two triangles given as Fraction points (0 when they intersect): the yardstick
of the guarantee.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import proximity_ref as pr
from proximity_ref import tri_distance_np

MAX_EVALS = 1024                    # cd_ccd.h CCD_MAX_EVALS
L_SLACK = 1.0 + 2.0 ** -20          # cd_ccd.h CCD_L_SLACK


def rate_np(tri) -> np.ndarray:
    """L of every pair, tri f64[n, 12, 3] (A0 A1 A2 B0 B1 B2 at x0, then at x1)."""
    t = np.asarray(tri, dtype=np.float64).reshape(-1, 12, 3)
    D = t[:, 6:] - t[:, :6]
    g = np.zeros((t.shape[0], 3))
    for k in range(6):
        g = g + D[:, k]
    g = g / 6.0
    m = [np.zeros(t.shape[0]), np.zeros(t.shape[0])]
    with np.errstate(all="ignore"):
        for k in range(6):
            v = D[:, k] - g
            l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            m[k // 3] = np.where(l > m[k // 3], l, m[k // 3])
    return (m[0] + m[1]) * L_SLACK


def advance_np(tri, dist: float):
    """ccd_advance on every pair of tri f64[n, 12, 3]: (toi f64[n] (+inf: not reported), d f64[n], evals u32[n]).  A reported pair
    with d > dist is unresolved."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 12, 3)
    n = t.shape[0]
    dist = float(dist)
    h = dist * 0.5
    L = rate_np(t)
    tt = np.zeros(n)
    stage = np.zeros(n, dtype=np.int8)
    evals = np.zeros(n, dtype=np.uint32)
    d = np.zeros(n)
    toi = np.full(n, np.inf)
    active = np.ones(n, dtype=bool)
    while active.any():
        i = np.nonzero(active)[0]
        P0, P1, st, ti = t[i, :6], t[i, 6:], stage[i], tt[i]
        with np.errstate(all="ignore"):
            X = np.where((st == 0)[:, None, None], P0, np.where((st == 2)[:, None, None], P1, P0 + ti[:, None, None] * (P1 - P0)))
        dd = tri_distance_np(X)
        evals[i] += 1
        d[i] = dd
        rep = dd <= dist
        toi[i[rep]] = np.where(st[rep] == 2, 1.0, ti[rep])
        stop = ~rep & ((st == 2) | (L[i] == 0.0))
        unres = ~rep & ~stop & (evals[i] >= MAX_EVALS)
        toi[i[unres]] = ti[unres]
        go = ~(rep | stop | unres)
        ig = i[go]
        with np.errstate(all="ignore"):
            tn = ti[go] + (dd[go] - h) / L[ig]
        end = tn >= 1.0
        stage[ig] = np.where(end, 2, 1)
        tt[ig] = np.where(end, ti[go], tn)
        active[i[~go]] = False
    return toi, d, evals


def gate_np(six_a, six_b, dist: float) -> np.ndarray:
    """The FP64 swept-box gate: six_a, six_b f64[n, 6, 3] (a triangle's vertices at x0, then at x1)."""
    alo, ahi, blo, bhi = six_a.min(axis=1), six_a.max(axis=1), six_b.min(axis=1), six_b.max(axis=1)
    return np.all(((alo - dist) <= (bhi + dist)) & ((blo - dist) <= (ahi + dist)), axis=1)


def ccd_pairs(x0, x1, vidx, ids=None, dist=0.01, queries=None, chunk=1 << 18, brute=None, counts=False):
    """Every pair cd_find_ccd reports: (pairs u32[n, 2] (smaller ID, larger ID), toi f64[n], dists f64[n]), rows sorted by (ID, ID).
    queries: face indices -- only the pairs with a triangle among them.  brute: all pairs (default: up to BRUTE_MAX triangles).
    counts: also return (pairs through the gate, evaluations)."""
    x0 = np.asarray(x0, dtype=np.float64)
    x1 = np.asarray(x1, dtype=np.float64)
    vidx = np.asarray(vidx, dtype=np.int64).reshape(-1, 3)
    n = vidx.shape[0]
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    six = np.concatenate([x0[vidx], x1[vidx]], axis=1)                         # [n, 6, 3]
    lo, hi = six.min(axis=1), six.max(axis=1)
    m = float(np.max(np.abs(np.concatenate([lo, hi])))) if n else 0.0
    w = dist + dist / 1024.0 + m / 1024.0                                      # each box by >= dist: the gate's 2 dist gap and far more
    if brute is None:
        brute = n <= pr.BRUTE_MAX
    if brute:
        i, j = np.triu_indices(n, 1)
        cand = np.stack([i, j], axis=1).astype(np.int64)
        if queries is not None:
            cand = cand[np.isin(cand[:, 0], queries) | np.isin(cand[:, 1], queries)]
    else:
        cand = pr._candidates(lo - w, hi + w, queries)
    out_p, out_t, out_d = [np.zeros((0, 2), dtype=np.uint32)], [np.zeros(0)], [np.zeros(0)]
    tested = evals = 0
    for c0 in range(0, cand.shape[0], chunk):
        c = cand[c0:c0 + chunk]
        i, j = c[:, 0], c[:, 1]
        sh = (vidx[i][:, :, None] == vidx[j][:, None, :]).any(axis=(1, 2))
        i, j = i[~sh], j[~sh]
        swap = (ids[j] < ids[i]) | ((ids[j] == ids[i]) & (j < i))
        a, b = np.where(swap, j, i), np.where(swap, i, j)
        g = gate_np(six[a], six[b], dist)
        a, b = a[g], b[g]
        tested += a.shape[0]
        tri = np.concatenate([x0[vidx[a]], x0[vidx[b]], x1[vidx[a]], x1[vidx[b]]], axis=1)
        toi, d, ev = advance_np(tri, dist)
        evals += int(ev.sum())
        ok = np.isfinite(toi)
        out_p.append(np.stack([ids[a][ok], ids[b][ok]], axis=1).astype(np.uint32))
        out_t.append(toi[ok])
        out_d.append(d[ok])
    res = sort_pairs(np.concatenate(out_p), np.concatenate(out_t), np.concatenate(out_d))
    return (res, (tested, evals)) if counts else res


def sort_pairs(pairs, toi, dists):
    """Rows sorted by (first, second), with their times and distances."""
    p = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    o = np.lexsort((p[:, 1], p[:, 0]))
    return p[o], np.asarray(toi, dtype=np.float64)[o], np.asarray(dists, dtype=np.float64)[o]


# ---------------------------------------------------------------- exact rationals
def _orient(a, b, c, d):
    """Sign of det[b - a, c - a, d - a] (exact)."""
    u, v, w = pr._fsub(b, a), pr._fsub(c, a), pr._fsub(d, a)
    x = u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0])
    return (x > 0) - (x < 0)


def _seg_crosses_tri(p, q, a, b, c) -> bool:
    """The segment [p, q] meets the triangle (a, b, c) with p and q strictly on opposite sides of its plane (the other ways two
    triangles meet make one of the 15 feature terms 0)."""
    sp, sq = _orient(a, b, c, p), _orient(a, b, c, q)
    if sp * sq >= 0:
        return False
    s = [_orient(p, q, a, b), _orient(p, q, b, c), _orient(p, q, c, a)]
    return all(x >= 0 for x in s) or all(x <= 0 for x in s)


def exact_dist2(P, Q) -> Fraction:
    """Exact squared distance of the triangles P, Q (three Fraction points each): 0 when they intersect, else the minimum over the
    15 feature pairs."""
    for X, Y in ((P, Q), (Q, P)):
        for k in range(3):
            if _seg_crosses_tri(X[k], X[(k + 1) % 3], *Y):
                return Fraction(0)
    vals = []
    for X, Y in ((P, Q), (Q, P)):
        for p in X:
            vals.append(pr._e_pt_face(p, *Y))
            for k in range(3):
                vals.append(pr._e_pt_seg(p, Y[k], Y[(k + 1) % 3]))
    for i in range(3):
        for k in range(3):
            vals.append(pr._e_seg_seg(P[i], P[(i + 1) % 3], Q[k], Q[(k + 1) % 3]))
    return min(x for x in vals if x is not None)


def exact_at(pair, t: Fraction):
    """The pair f64[12, 3] at time t, exactly: p0 + t (p1 - p0) per coordinate as Fractions -> (P, Q)."""
    v = np.asarray(pair, dtype=np.float64).reshape(12, 3)
    pts = []
    for k in range(6):
        p0 = [Fraction(float(x)) for x in v[k]]
        p1 = [Fraction(float(x)) for x in v[6 + k]]
        pts.append(tuple(p0[a] + t * (p1[a] - p0[a]) for a in range(3)))
    return pts[:3], pts[3:]
