"""CPU restatement of the swept-point queries (include/mi355cd.h cd_sweep_points_all / cd_sweep_points / cd_pt_advance_points;
csrc/cd_sweep.h pt_advance).  No test in here.

pt_advance_np restates the device's conservative advancement of a moving point against a moving triangle operation for operation
(numpy float64, no contraction, correctly rounded divide and sqrt) on top of point_ref.pt_tri_np, so toi, every value of the reporting
evaluation and the evaluation count agree bit for bit.  sweep_rows_ref is the query as ALL pairs of items and triangles -- no tree and
no box filter beyond the gate the contract defines -- and first_of its per-item minimum in the form cd_sweep_points returns.
exact_dist2 is the exact rational squared distance of a Fraction point and a Fraction triangle: the yardstick of the guarantee.
pin_inputs are the (item, triangle) classes the CPU tests and the device pin share."""
from __future__ import annotations

import collections
from fractions import Fraction

import numpy as np

import point_ref as ptr
import proximity_ref as pr

MAX_EVALS = 1024                    # cd_ccd.h CCD_MAX_EVALS
L_SLACK = 1.0 + 2.0 ** -20          # cd_ccd.h CCD_L_SLACK
NONE = np.uint32(0xFFFFFFFF)

SweepRows = collections.namedtuple("SweepRows", "rows ids toi dist closest uv feature side")
Advance = collections.namedtuple("Advance", "toi dist closest uv feature side evals")


def _items(items):
    return np.ascontiguousarray(items, dtype=np.float64).reshape(-1, 7)


def _tris(tri):
    return np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 6, 3)


def rate_np(items, tri) -> np.ndarray:
    """L of every pair: items f64[n, 7] (p0, p1, dist), tri f64[n, 6, 3] (a0 a1 a2 at x0, then b0 b1 b2 at x1)."""
    it, t = _items(items), _tris(tri)
    dp = it[:, 3:6] - it[:, 0:3]
    m = np.zeros(it.shape[0])
    with np.errstate(all="ignore"):
        for k in range(3):
            v = (t[:, 3 + k] - t[:, k]) - dp
            l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
            m = np.where(l > m, l, m)
        return m * L_SLACK


def pt_advance_np(items, tri) -> Advance:
    """pt_advance on every pair: toi f64[n] (+inf: not reported) and pt_tri's values of the last evaluation made (the reporting one of a
    reported pair), with the evaluation count.  A reported pair with dist > the item's dist is unresolved."""
    it, t = _items(items), _tris(tri)
    n = it.shape[0]
    dist = it[:, 6]
    h = dist * 0.5
    L = rate_np(it, t)
    tt = np.zeros(n)
    stage = np.zeros(n, dtype=np.int8)
    evals = np.zeros(n, dtype=np.uint32)
    toi = np.full(n, np.inf)
    d = np.zeros(n); q = np.zeros((n, 3)); uv = np.zeros((n, 2)); feat = np.zeros(n, dtype=np.uint8); side = np.zeros(n, dtype=np.uint8)
    active = np.ones(n, dtype=bool)
    while active.any():
        i = np.nonzero(active)[0]
        st, ti = stage[i], tt[i]
        A = np.concatenate([it[i, None, 0:3], t[i, :3]], axis=1)               # the point, then the triangle, at the start ...
        B = np.concatenate([it[i, None, 3:6], t[i, 3:]], axis=1)               # ... and at the end
        with np.errstate(all="ignore"):
            X = np.where((st == 0)[:, None, None], A, np.where((st == 2)[:, None, None], B, A + ti[:, None, None] * (B - A)))
        dd, qq, u, v, f, s = ptr.pt_tri_np(X[:, 0], X[:, 1:])
        evals[i] += 1
        d[i] = dd; q[i] = qq; uv[i, 0] = u; uv[i, 1] = v; feat[i] = f; side[i] = s
        rep = dd <= dist[i]
        toi[i[rep]] = np.where(st[rep] == 2, 1.0, ti[rep])
        stop = ~rep & ((st == 2) | (L[i] == 0.0))
        unres = ~rep & ~stop & (evals[i] >= MAX_EVALS)
        toi[i[unres]] = ti[unres]
        go = ~(rep | stop | unres)
        ig = i[go]
        with np.errstate(all="ignore"):
            tn = ti[go] + (dd[go] - h[ig]) / L[ig]
        end = tn >= 1.0
        stage[ig] = np.where(end, 2, 1)
        tt[ig] = np.where(end, ti[go], tn)
        active[i[~go]] = False
    return Advance(toi, d, q, uv, feat, side, evals)


def gate_np(items, six) -> np.ndarray:
    """The FP64 gate: the box of {p0, p1} and the box of the triangle's six points, each widened by dist, overlap (closed)."""
    it, s = _items(items), _tris(six)
    plo, phi = np.minimum(it[:, 0:3], it[:, 3:6]), np.maximum(it[:, 0:3], it[:, 3:6])
    tlo, thi = s.min(axis=1), s.max(axis=1)
    dist = it[:, 6:7]
    return np.all(((plo - dist) <= (thi + dist)) & ((tlo - dist) <= (phi + dist)), axis=1)


def sweep_rows_ref(x0, x1, vidx, ids, items, skip=None, pairs_per_chunk=1 << 21, counts=False):
    """Every item against ALL triangles: the skip_vertex filter, the gate, pt_advance; a row for every reported pair, sorted by
    (item, face).  x1 None: the mesh does not move.  counts: also (pairs through the gate, evaluations, unresolved rows)."""
    x0 = np.asarray(x0, dtype=np.float64)
    x1 = x0 if x1 is None else np.asarray(x1, dtype=np.float64)
    vidx = np.asarray(vidx).astype(np.int64).reshape(-1, 3)
    nt = vidx.shape[0]
    ids = np.arange(nt, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    it = _items(items)
    n = it.shape[0]
    six = np.concatenate([x0[vidx], x1[vidx]], axis=1)                          # [T, 6, 3]
    tlo, thi = six.min(axis=1), six.max(axis=1)
    plo, phi = np.minimum(it[:, 0:3], it[:, 3:6]), np.maximum(it[:, 0:3], it[:, 3:6])
    sk = None if skip is None else np.asarray(skip, dtype=np.int64)
    step = max(1, pairs_per_chunk // max(nt, 1))
    ks, fs = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for a in range(0, n, step):
        b = min(n, a + step)
        dist = it[a:b, 6][:, None, None]
        ok = np.all(((plo[a:b, None] - dist) <= (thi[None] + dist)) & ((tlo[None] - dist) <= (phi[a:b, None] + dist)), axis=2)   # [b - a, T]
        if sk is not None:
            ok &= ~(vidx[None, :, :] == sk[a:b, None, None]).any(axis=2)
        ri, ti = np.nonzero(ok)
        ks.append(a + ri); fs.append(ti)
    k, f = np.concatenate(ks), np.concatenate(fs)                               # (sorted by (item, face): chunks in order, nonzero row-major)
    adv = pt_advance_np(it[k], six[f])
    assert gate_np(it[k], six[f]).all()
    hit = np.isfinite(adv.toi)
    w = SweepRows(np.stack([k[hit], f[hit]], axis=1).astype(np.uint32), ids[f[hit]], adv.toi[hit], adv.dist[hit], adv.closest[hit], adv.uv[hit],
                  adv.feature[hit], adv.side[hit])
    if counts:
        return w, (int(k.shape[0]), int(adv.evals.sum()), int((hit & ~(adv.dist <= it[k, 6])).sum()))
    return w


def first_of(w: SweepRows, n):
    """The per-item minimum of a row set by (toi, ID, face) as cd_sweep_points returns it: (face, ids, toi, dist, closest, uv, feature,
    side); an item without a row: face NONE, toi +inf, zeros."""
    o = np.lexsort((w.rows[:, 1], w.ids, w.toi, w.rows[:, 0]))
    k, first = np.unique(w.rows[o, 0], return_index=True)
    at, k = o[first], k.astype(np.int64)
    face = np.full(n, NONE, dtype=np.uint32); oid = np.zeros(n, dtype=np.uint32); toi = np.full(n, np.inf); dist = np.zeros(n)
    q = np.zeros((n, 3)); uv = np.zeros((n, 2)); feat = np.zeros(n, dtype=np.uint8); side = np.zeros(n, dtype=np.uint8)
    face[k] = w.rows[at, 1]; oid[k] = w.ids[at]; toi[k] = w.toi[at]; dist[k] = w.dist[at]; q[k] = w.closest[at]; uv[k] = w.uv[at]
    feat[k] = w.feature[at]; side[k] = w.side[at]
    return face, oid, toi, dist, q, uv, feat, side


# ---------------------------------------------------------------- exact rationals
def exact_at(item, tri, t: Fraction):
    """The point and the triangle at time t, exactly: a + t (b - a) per coordinate as Fractions -> (p, (a, b, c))."""
    it = np.asarray(item, dtype=np.float64).reshape(7)
    s = np.asarray(tri, dtype=np.float64).reshape(6, 3)
    mix = lambda a, b: tuple(Fraction(float(a[k])) + t * (Fraction(float(b[k])) - Fraction(float(a[k]))) for k in range(3))
    return mix(it[0:3], it[3:6]), tuple(mix(s[k], s[3 + k]) for k in range(3))


def exact_dist2(p, tri) -> Fraction:
    """Exact squared distance of the Fraction point p from the Fraction triangle: the face term where the projection falls inside, and
    the three edges (a degenerate triangle has the distance of the segment or point it is)."""
    a, b, c = tri
    vals = [pr._e_pt_face(p, a, b, c), pr._e_pt_seg(p, a, b), pr._e_pt_seg(p, b, c), pr._e_pt_seg(p, c, a)]
    return min(x for x in vals if x is not None)


# ---------------------------------------------------------------- the pin's inputs
def _frame(g, n):
    p = g.uniform(-1.0, 1.0, (n, 3, 3))
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    nrm = np.cross(e1, e2)
    return p, nrm / np.linalg.norm(nrm, axis=1, keepdims=True)


def _inside(g, p):
    """A point well inside each triangle (every barycentric >= 0.1)."""
    a, b = ptr._bary_in(g, p.shape[0])
    a, b = 0.1 + 0.7 * a, 0.1 + 0.7 * b
    return p[:, 0] + a[:, None] * (p[:, 1] - p[:, 0]) + b[:, None] * (p[:, 2] - p[:, 0])


def _pack(p0, p1, dist, a, b):
    n = p0.shape[0]
    it = np.empty((n, 7)); it[:, 0:3] = p0; it[:, 3:6] = p1; it[:, 6] = dist
    return it, np.concatenate([a, b], axis=1)


CLASSES = ("random", "start_within", "translate", "end_touch", "approach", "long", "unresolved", "near_parallel", "degenerate", "rotating",
           "scaled_up", "scaled_down")


def pin_class(kind, n, g):
    """(items f64[n, 7], tris f64[n, 6, 3]) of one kind."""
    if kind == "random":                                                        # anything: short of, past and through a triangle that deforms
        a = g.uniform(-1, 1, (n, 3, 3))
        b = a + g.normal(size=(n, 3, 3)) * 0.3
        p0 = g.uniform(-2, 2, (n, 3))
        aim = _inside(g, b) + g.normal(size=(n, 3)) * 0.2                        # (a point near the triangle's end position)
        return _pack(p0, p0 + (aim - p0) * g.uniform(0.3, 2.0, (n, 1)), g.uniform(0.01, 0.3, n), a, b)
    if kind == "start_within":                                                  # within dist at t = 0: toi 0 after one evaluation
        a, nh = _frame(g, n)
        dist = g.uniform(0.01, 0.1, n)
        p0 = _inside(g, a) + nh * (dist * g.uniform(-0.9, 0.9, n))[:, None]
        return _pack(p0, p0 + g.normal(size=(n, 3)), dist, a, a + g.normal(size=(n, 3, 3)) * 0.2)
    if kind == "translate":                                                     # a common translation on dyadic positions: L == 0 exactly
        a = np.round(g.uniform(-1, 1, (n, 3, 3)) * 1024) / 1024
        p0 = np.round(g.uniform(-1, 1, (n, 3)) * 1024) / 1024 + np.array([0.0, 0.0, 2.5])
        near = np.arange(n) % 4 == 0
        p0[near] = a[near, 0] + np.array([0.0, 0.0, 1.0 / 64])                   # a quarter of them within dist of a vertex
        move = np.round(g.uniform(-4, 4, (n, 3)) * 64) / 64
        return _pack(p0, p0 + move, np.full(n, 0.0625), a, a + move[:, None])
    if kind == "end_touch":                                                     # the first step overshoots the end, where the point is within dist: toi 1, two evaluations
        a, nh = _frame(g, n)
        dist = g.uniform(0.01, 0.1, n)
        s = _inside(g, a)
        return _pack(s + nh * g.uniform(0.5, 1.0, n)[:, None], s + nh * (0.75 * dist)[:, None], dist, a, a)
    if kind == "approach":                                                      # through the moving triangle: toi strictly inside
        a, nh = _frame(g, n)
        s = _inside(g, a)
        b = a + g.normal(size=(n, 1, 3)) * 0.1
        return _pack(s + nh * g.uniform(0.5, 2.0, n)[:, None], _inside(g, b) - nh * g.uniform(0.2, 1.0, n)[:, None], g.uniform(0.005, 0.05, n), a, b)
    if kind in ("long", "unresolved"):                                          # along the face at 1.5 dist, K dist far: about K evaluations
        a, nh = _frame(g, n)
        s0, s1 = _inside(g, a), _inside(g, a)
        K = g.uniform(150, 400, n) if kind == "long" else g.uniform(1500, 3000, n)
        dist = np.linalg.norm(s1 - s0, axis=1) / K
        end = np.where(np.arange(n) % 2 == 0, 1.5, 0.8) if kind == "long" else np.full(n, 1.5)   # (long: half of them dip within dist at the end)
        return _pack(s0 + nh * (1.5 * dist)[:, None], s1 + nh * (end * dist)[:, None], dist, a, a)
    if kind == "near_parallel":                                                 # nearly the same motion: L tiny, not zero
        a, nh = _frame(g, n)
        V = g.normal(size=(n, 3))
        p0 = _inside(g, a) + nh * g.uniform(0.02, 0.5, n)[:, None]
        return _pack(p0, p0 + V - nh * g.uniform(0.0, 1e-6, n)[:, None], g.uniform(0.01, 0.1, n), a, a + V[:, None] + g.normal(size=(n, 3, 3)) * 1e-9)
    if kind == "degenerate":                                                    # segments and points, at both ends
        it, t = pin_class("approach", n, g)
        k = np.arange(n) % 3
        t[k == 0, 1] = t[k == 0, 0]; t[k == 0, 4] = t[k == 0, 3]                 # a repeated vertex
        c = k == 1
        t[c, 2] = t[c, 0] + 0.37 * (t[c, 1] - t[c, 0])                           # collinear at x0
        c = k == 2
        t[c, 1] = t[c, 0]; t[c, 2] = t[c, 0]; t[c, 4] = t[c, 3]; t[c, 5] = t[c, 3]   # a point
        return it, t
    if kind == "rotating":                                                      # the triangle turns about its centroid and moves toward the point
        a, nh = _frame(g, n)
        th = g.uniform(0.3, 1.5, n)
        c, s = np.cos(th), np.sin(th)
        R = np.zeros((n, 3, 3)); R[:, 0, 0] = c; R[:, 0, 1] = -s; R[:, 1, 0] = s; R[:, 1, 1] = c; R[:, 2, 2] = 1.0
        ctr = a.mean(axis=1, keepdims=True)
        p0 = ctr[:, 0] + nh * g.uniform(0.3, 1.0, n)[:, None]
        b = np.einsum("nij,nkj->nki", R, a - ctr) + ctr + (nh * g.uniform(0.2, 1.2, n)[:, None])[:, None]
        return _pack(p0, p0 + g.normal(size=(n, 3)) * 0.1, g.uniform(0.01, 0.1, n), a, b)
    if kind in ("scaled_up", "scaled_down"):                                    # 1e+-100
        it, t = pin_class("random", n, g)
        s = 1e100 if kind == "scaled_up" else 1e-100
        return it * s, t * s
    raise ValueError(kind)


def pin_inputs(n, seed=0):
    """name -> (items, tris) with n pairs a class (the two long-running classes: n / 8)."""
    g = np.random.default_rng(seed)
    return {k: pin_class(k, max(1, n // 8) if k in ("long", "unresolved") else n, g) for k in CLASSES}


def pin_conditions(items, tris, adv: Advance):
    """What a pin of pt_advance needs of its inputs, asserted from the restatement's own results, so that no branch can go unvisited:
    evaluation counts of 1, of 2, of at least 100 and of exactly MAX_EVALS with an unresolved result; toi of 0, of 1 and strictly between;
    pairs not reported after one evaluation (L == 0), after two, and after many."""
    it = _items(items)
    rep = np.isfinite(adv.toi)
    unres = rep & (adv.dist > it[:, 6])
    L = rate_np(it, tris)
    figures = {
        "evals 1": int((adv.evals == 1).sum()), "evals 2": int((adv.evals == 2).sum()), "evals >= 100": int((adv.evals >= 100).sum()),
        "unresolved": int(unres.sum()), "toi 0": int((adv.toi == 0.0).sum()), "toi 1": int((adv.toi == 1.0).sum()),
        "toi between": int(((adv.toi > 0.0) & (adv.toi < 1.0) & ~unres).sum()), "L == 0 apart": int(((L == 0.0) & ~rep).sum()),
        "not reported": int((~rep).sum()), "not reported after many": int((~rep & (adv.evals >= 100)).sum()),
    }
    print(figures)
    assert all(v > 0 for v in figures.values()), figures
    assert np.all(adv.evals[unres] == MAX_EVALS) and np.all((adv.evals >= 1) & (adv.evals <= MAX_EVALS))
    assert np.all(adv.evals[(L == 0.0)] == 1)
    return figures
