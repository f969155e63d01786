"""CPU restatement of the swept-segment queries (include/mi355cd.h cd_sweep_segments_all / cd_sweep_segments / cd_seg_advance_points;
csrc/cd_sweep_segments.h seg_advance).  No test in here.

seg_advance_np restates the device's conservative advancement of a moving segment against a moving triangle operation for operation
(numpy float64, no contraction, correctly rounded divide and sqrt) on top of segment_ref.seg_tri_np, in sweep_ref.pt_advance_np's loop,
so toi, every value of the reporting evaluation and the evaluation count agree bit for bit.  sweep_segment_rows_ref is the query as ALL
pairs of items and triangles -- no tree and no box filter beyond the gate the contract defines -- and first_of its per-item minimum in
the form cd_sweep_segments returns.  exact_seg_tri_d2 is the exact rational squared distance of a Fraction segment and a Fraction
triangle: the yardstick of the guarantee.  pin_inputs are the (item, triangle) classes the CPU tests and the device pin share.

An item is 13 doubles (a0, b0, a1, b1, dist); a triangle 6 x 3 (its vertices at x0, then at x1)."""
from __future__ import annotations

import collections
import functools
from fractions import Fraction

import numpy as np

import proximity_ref as pr
import segment_ref as sref
import sweep_ref as swr
import within_ref as wr

MAX_EVALS = swr.MAX_EVALS
L_SLACK = swr.L_SLACK
NONE = np.uint32(0xFFFFFFFF)

VALUES = "dist s on_seg on_tri uv feature end cross side"
SweepSegRows = collections.namedtuple("SweepSegRows", "rows ids toi " + VALUES)
SegAdvance = collections.namedtuple("SegAdvance", "toi " + VALUES + " evals term stage")


def _items(items):
    return np.ascontiguousarray(items, dtype=np.float64).reshape(-1, 13)


def _tris(tri):
    return np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 6, 3)


def pack(a0, b0, a1, b1, dist):
    pts = [np.asarray(x, dtype=np.float64).reshape(-1, 3) for x in (a0, b0, a1, b1)]
    it = np.empty((pts[0].shape[0], 13))
    for k, x in enumerate(pts):
        it[:, 3 * k:3 * k + 3] = x
    it[:, 12] = dist
    return it


def point_items(items7):
    """The swept-point items [n, 7] (p0, p1, dist) as zero-length segments."""
    it = np.asarray(items7, dtype=np.float64).reshape(-1, 7)
    return pack(it[:, 0:3], it[:, 0:3], it[:, 3:6], it[:, 3:6], it[:, 6])


def rate_np(items, tri) -> np.ndarray:
    """L of every pair: the largest of the six norms |(x1_i - x0_i) - (j1 - j0)|, j in {a, b}, times 1 + 2^-20."""
    it, t = _items(items), _tris(tri)
    da, db = it[:, 6:9] - it[:, 0:3], it[:, 9:12] - it[:, 3:6]
    m = np.zeros(it.shape[0])
    with np.errstate(all="ignore"):
        for k in range(3):
            dv = t[:, 3 + k] - t[:, k]
            for dj in (da, db):
                v = dv - dj
                l = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
                m = np.where(l > m, l, m)
        return m * L_SLACK


def positions(items, tri, stage, t):
    """The five points (a, b, the triangle's three) where the advancement evaluates them: sweep_at per point -> [n, 5, 3]."""
    it, tr = _items(items), _tris(tri)
    A = np.concatenate([it[:, None, 0:3], it[:, None, 3:6], tr[:, :3]], axis=1)
    B = np.concatenate([it[:, None, 6:9], it[:, None, 9:12], tr[:, 3:]], axis=1)
    st, ti = np.asarray(stage), np.asarray(t, dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.where((st == 0)[:, None, None], A, np.where((st == 2)[:, None, None], B, A + ti[:, None, None] * (B - A)))


def seg_advance_np(items, tri) -> SegAdvance:
    """seg_advance on every pair: toi f64[n] (+inf: not reported) and seg_tri's values of the last evaluation made (the reporting one of
    a reported pair), with the evaluation count, seg_tri's winning term (-1: a crossing) and the stage of that evaluation.  A reported
    pair with dist > the item's dist is unresolved."""
    it, t = _items(items), _tris(tri)
    n = it.shape[0]
    dist = it[:, 12]
    h = dist * 0.5
    L = rate_np(it, t)
    tt = np.zeros(n)
    stage = np.zeros(n, dtype=np.int8)
    evals = np.zeros(n, dtype=np.uint32)
    toi = np.full(n, np.inf)
    out = dict(dist=np.zeros(n), s=np.zeros(n), on_seg=np.zeros((n, 3)), on_tri=np.zeros((n, 3)), uv=np.zeros((n, 2)), feature=np.zeros(n, dtype=np.uint8),
               end=np.zeros(n, dtype=np.uint8), cross=np.zeros(n, dtype=np.uint8), side=np.zeros(n, dtype=np.uint8), term=np.zeros(n, dtype=np.int64))
    last = np.zeros(n, dtype=np.int8)
    active = np.ones(n, dtype=bool)
    while active.any():
        i = np.nonzero(active)[0]
        st, ti = stage[i], tt[i]
        X = positions(it[i], t[i], st, ti)
        r = sref.seg_tri_np(np.concatenate([X[:, 0], X[:, 1]], axis=1), X[:, 2:])
        evals[i] += 1
        for name in out:
            out[name][i] = getattr(r, name)
        last[i] = st
        dd = r.dist
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
    return SegAdvance(toi, *(out[k] for k in VALUES.split()), evals, out["term"], last)


def item_box(items):
    it = _items(items)
    p = it[:, 0:12].reshape(-1, 4, 3)
    return p.min(axis=1), p.max(axis=1)


def gate_np(items, six) -> np.ndarray:
    """The FP64 gate: the box of {a0, b0, a1, b1} and the box of the triangle's six points, each widened by dist, overlap (closed)."""
    it, s = _items(items), _tris(six)
    plo, phi = item_box(it)
    tlo, thi = s.min(axis=1), s.max(axis=1)
    dist = it[:, 12:13]
    return np.all(((plo - dist) <= (thi + dist)) & ((tlo - dist) <= (phi + dist)), axis=1)


def sweep_segment_rows_ref(x0, x1, vidx, ids, items, skip=None, pairs_per_chunk=1 << 21, counts=False):
    """Every item against ALL triangles: the skip_vertices filter (n x 2), the gate, seg_advance; a row for every reported pair, sorted
    by (item, face).  x1 None: the mesh does not move.  counts: also (pairs through the gate, evaluations, unresolved rows)."""
    x0 = np.asarray(x0, dtype=np.float64)
    x1 = x0 if x1 is None else np.asarray(x1, dtype=np.float64)
    vidx = np.asarray(vidx).astype(np.int64).reshape(-1, 3)
    nt = vidx.shape[0]
    ids = np.arange(nt, dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    it = _items(items)
    n = it.shape[0]
    six = np.concatenate([x0[vidx], x1[vidx]], axis=1)                          # [T, 6, 3]
    tlo, thi = six.min(axis=1), six.max(axis=1)
    plo, phi = item_box(it)
    sk = None if skip is None else np.asarray(skip, dtype=np.int64).reshape(-1, 2)
    step = max(1, pairs_per_chunk // max(nt, 1))
    ks, fs = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for a in range(0, n, step):
        b = min(n, a + step)
        dist = it[a:b, 12][:, None, None]
        ok = np.all(((plo[a:b, None] - dist) <= (thi[None] + dist)) & ((tlo[None] - dist) <= (phi[a:b, None] + dist)), axis=2)   # [b - a, T]
        if sk is not None:
            for c in range(2):                                                  # (0xFFFFFFFF is no vertex's index: it removes nothing)
                ok &= ~(vidx[None, :, :] == sk[a:b, c, None, None]).any(axis=2)
        ri, ti = np.nonzero(ok)
        ks.append(a + ri); fs.append(ti)
    k, f = np.concatenate(ks), np.concatenate(fs)                               # (sorted by (item, face): chunks in order, nonzero row-major)
    adv = seg_advance_np(it[k], six[f])
    assert gate_np(it[k], six[f]).all()
    hit = np.isfinite(adv.toi)
    w = SweepSegRows(np.stack([k[hit], f[hit]], axis=1).astype(np.uint32), ids[f[hit]], adv.toi[hit], *(x[hit] for x in adv[1:10]))
    if counts:
        return w, (int(k.shape[0]), int(adv.evals.sum()), int((hit & ~(adv.dist <= it[k, 12])).sum()))
    return w


def first_of(w: SweepSegRows, n):
    """The per-item minimum of a row set by (toi, ID, face) as cd_sweep_segments returns it: (face, ids, toi, dist, s, on_seg, on_tri,
    uv, feature, end, cross, side); an item without a row: face NONE, toi +inf, zeros."""
    o = np.lexsort((w.rows[:, 1], w.ids, w.toi, w.rows[:, 0]))
    k, first = np.unique(w.rows[o, 0], return_index=True)
    at, k = o[first], k.astype(np.int64)
    face = np.full(n, NONE, dtype=np.uint32)
    face[k] = w.rows[at, 1]
    out = [face]
    for name, x in zip(w._fields[1:], w[1:]):
        v = np.full((n,) + x.shape[1:], np.inf if name == "toi" else 0, dtype=x.dtype)
        v[k] = x[at]
        out.append(v)
    return tuple(out)


# ---------------------------------------------------------------- exact rationals
def _fr(x):
    return tuple(Fraction(float(v)) for v in x)


def exact_at(item, tri, t: Fraction):
    """The segment and the triangle at time t, exactly: x + t (y - x) per coordinate as Fractions -> ((a, b), (p0, p1, p2))."""
    it = np.asarray(item, dtype=np.float64).reshape(13)
    s = np.asarray(tri, dtype=np.float64).reshape(6, 3)
    mix = lambda a, b: tuple(Fraction(float(a[k])) + t * (Fraction(float(b[k])) - Fraction(float(a[k]))) for k in range(3))
    return (mix(it[0:3], it[6:9]), mix(it[3:6], it[9:12])), tuple(mix(s[k], s[3 + k]) for k in range(3))


def exact_meets(seg, tri) -> bool:
    """Does the Fraction segment meet the closed Fraction triangle?  Decided in rationals."""
    return exact_seg_tri_d2(seg, tri) == 0


def exact_seg_tri_d2(seg, tri) -> Fraction:
    """Exact squared distance of the Fraction segment (a, b) from the Fraction triangle: 0 when the segment crosses the face (decided
    in rationals: the point where it meets the plane lies in the closed triangle); otherwise the minimum of the point-face, point-edge
    and edge-edge blocks of proximity_ref's exact section (a degenerate triangle has the distance of the segment or point it is; a
    segment in the face's plane that meets the triangle has an end in it or meets an edge: one of those blocks is 0)."""
    a, b = seg
    p = tri
    e1, e2 = pr._fsub(p[1], p[0]), pr._fsub(p[2], p[0])
    nrm = (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])
    if any(c != 0 for c in nrm):
        da, db = pr._fdot(nrm, pr._fsub(a, p[0])), pr._fdot(nrm, pr._fsub(b, p[0]))
        if da != db and da * db <= 0:
            t = da / (da - db)
            x = tuple(a[k] + t * (b[k] - a[k]) for k in range(3))
            if pr._e_pt_face(x, *p) is not None:
                return Fraction(0)
    vals = [pr._e_pt_face(a, *p), pr._e_pt_face(b, *p)]
    for k in range(3):
        u, v = p[k], p[(k + 1) % 3]
        vals += [pr._e_pt_seg(a, u, v), pr._e_pt_seg(b, u, v), pr._e_pt_seg(u, a, b), pr._e_seg_seg(a, b, u, v)]
    return min(x for x in vals if x is not None)


def exact_pair_d2(segs6, tri9) -> Fraction:
    """exact_seg_tri_d2 of one float pair: segs6 (a, b), tri9 (p0, p1, p2)."""
    s = np.asarray(segs6, dtype=np.float64).reshape(2, 3)
    p = np.asarray(tri9, dtype=np.float64).reshape(3, 3)
    return exact_seg_tri_d2((_fr(s[0]), _fr(s[1])), tuple(_fr(x) for x in p))


# ---------------------------------------------------------------- the pin's inputs
def _unit(g, n):
    u = g.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _from_points(it7, tris, off0, off1):
    """Swept-point items as segments: a is the point, b = a + off0 at the start and a + off1 at the end."""
    return pack(it7[:, 0:3], it7[:, 0:3] + off0, it7[:, 3:6], it7[:, 3:6] + off1, it7[:, 6]), tris


# sweep_ref's classes with a segment grown from the point, then the edge-edge classes
CLASSES = tuple("pt_" + k for k in swr.CLASSES) + ("zero_length", "shrink", "edge_on", "rim", "vertex", "rotating_segment", "cross_start")
# classes whose crossing reports may be ray_tri's noise (a segment within rounding of the face's plane, or a sliver / degenerate face):
# half 2 of the guarantee is not asserted on their cross = 1 reports
EXEMPT = ("pt_degenerate",)


def pin_class(kind, n, g):
    """(items f64[n, 13], tris f64[n, 6, 3]) of one kind."""
    if kind.startswith("pt_"):
        base = kind[3:]
        it7, t = swr.pin_class(base, n, g)
        a = t[:, :3]
        nrm = np.cross(a[:, 1] - a[:, 0], a[:, 2] - a[:, 0])
        ln = np.linalg.norm(nrm, axis=1, keepdims=True)
        nh = np.where(ln > 0, nrm / np.where(ln > 0, ln, 1.0), _unit(g, n))
        if base == "translate":                                                 # a common translation on dyadic positions: L == 0 exactly
            off = np.round(g.uniform(-1, 1, (n, 3)) * 64) / 64 + np.array([0.0, 0.0, 0.25])
            return _from_points(it7, t, off, off)
        if base in ("long", "unresolved", "end_touch", "near_parallel"):        # the segment stands off the face: end a stays the closest point
            sgn = np.sign(np.einsum("nk,nk->n", it7[:, 0:3] - a[:, 0], nh))[:, None]
            off = nh * sgn * g.uniform(0.2, 0.6, (n, 1))
            return _from_points(it7, t, off, off)
        if base in ("scaled_up", "scaled_down"):
            s = 1e100 if base == "scaled_up" else 1e-100
            return _from_points(it7, t, _unit(g, n) * g.uniform(0.1, 1.0, (n, 1)) * s, _unit(g, n) * g.uniform(0.1, 1.0, (n, 1)) * s)
        return _from_points(it7, t, _unit(g, n) * g.uniform(0.05, 0.8, (n, 1)), _unit(g, n) * g.uniform(0.05, 0.8, (n, 1)))
    if kind == "zero_length":                                                   # moving points: a == b at both ends
        it7 = np.concatenate([swr.pin_class(k, max(1, n // 4), g)[0] for k in ("random", "approach", "start_within", "rotating")])
        g2 = np.random.default_rng(int(g.integers(1 << 30)))
        t = np.concatenate([swr.pin_class(k, max(1, n // 4), g2)[1] for k in ("random", "approach", "start_within", "rotating")])
        return point_items(it7), t
    if kind == "shrink":                                                        # a segment that shrinks to a point during the step
        it7, t = swr.pin_class("approach", n, g)
        return _from_points(it7, t, _unit(g, n) * g.uniform(0.1, 0.6, (n, 1)), np.zeros((n, 3)))
    a, nh = swr._frame(g, n)
    ctr = a.mean(axis=1)
    e = a[:, 1] - a[:, 0]
    e /= np.linalg.norm(e, axis=1, keepdims=True)
    if kind == "edge_on":                                                       # parallel to the face, longer than it, both ends far outside dist: passes through the sheet
        dist = g.uniform(0.005, 0.02, n)
        w = np.cross(nh, e)
        d = e * np.cos(0.3) + w * np.sin(0.3)
        c0, c1 = swr._inside(g, a), swr._inside(g, a)
        h0, h1 = g.uniform(0.3, 0.8, (n, 1)), g.uniform(0.3, 0.8, (n, 1))
        return pack(c0 - 4.0 * d + nh * h0, c0 + 4.0 * d + nh * h0, c1 - 4.0 * d - nh * h1, c1 + 4.0 * d - nh * h1, dist), np.concatenate([a, a], axis=1)
    if kind == "rim":                                                           # across the face's plane, outside the triangle, sliding in over edge 0-1
        dist = g.uniform(0.005, 0.03, n)
        out = np.cross(e, nh)                                                   # in the plane, normal to edge 0-1
        out *= np.sign(np.einsum("nk,nk->n", out, a[:, 0] - ctr))[:, None]      # pointing away from the triangle
        m = a[:, 0] + (a[:, 1] - a[:, 0]) * g.uniform(0.2, 0.8, (n, 1))
        lean = e * g.uniform(-0.3, 0.3, (n, 1))
        s0, s1 = m + out * g.uniform(0.3, 0.9, (n, 1)), m - out * g.uniform(0.05, 0.15, (n, 1))
        up, dn = nh * g.uniform(0.5, 1.0, (n, 1)) + lean, -nh * g.uniform(0.5, 1.0, (n, 1)) - lean
        return pack(s0 + up, s0 + dn, s1 + up, s1 + dn, dist), np.concatenate([a, a + g.normal(size=(n, 1, 3)) * 0.02], axis=1)
    if kind == "vertex":                                                        # across the plane beyond vertex 0, moving in on it: the vertex against the segment's inside
        dist = g.uniform(0.005, 0.03, n)
        out = a[:, 0] - ctr
        out /= np.linalg.norm(out, axis=1, keepdims=True)
        s0, s1 = a[:, 0] + out * g.uniform(0.3, 0.9, (n, 1)), a[:, 0] - out * g.uniform(0.0, 0.05, (n, 1))
        up, dn = nh * g.uniform(0.5, 1.0, (n, 1)), -nh * g.uniform(0.5, 1.0, (n, 1))
        return pack(s0 + up, s0 + dn, s1 + up, s1 + dn, dist), np.concatenate([a, a], axis=1)
    if kind == "rotating_segment":                                              # the segment turns about its midpoint over the face and sinks toward it
        dist = g.uniform(0.01, 0.05, n)
        w = np.cross(nh, e)
        th = g.uniform(0.5, 1.5, (n, 1))
        d0, d1 = e, e * np.cos(th) + w * np.sin(th)
        half = g.uniform(0.2, 1.5, (n, 1))
        c = swr._inside(g, a)
        h0, h1 = g.uniform(0.2, 0.6, (n, 1)), g.uniform(-0.1, 0.1, (n, 1))
        tilt = nh * g.uniform(-0.1, 0.1, (n, 1))
        return pack(c + nh * h0 - half * d0 - tilt, c + nh * h0 + half * d0 + tilt, c + nh * h1 - half * d1 - tilt, c + nh * h1 + half * d1 + tilt, dist), \
            np.concatenate([a, a + g.normal(size=(n, 3, 3)) * 0.05], axis=1)
    if kind == "cross_start":                                                   # through the face at t = 0: toi 0, cross = 1, one evaluation
        dist = g.uniform(0.01, 0.1, n)
        c = swr._inside(g, a)
        u = nh + _unit(g, n) * 0.3
        a0, b0 = c + u * g.uniform(0.2, 1.0, (n, 1)), c - u * g.uniform(0.2, 1.0, (n, 1))
        return pack(a0, b0, a0 + g.normal(size=(n, 3)), b0 + g.normal(size=(n, 3)), dist), np.concatenate([a, a + g.normal(size=(n, 3, 3)) * 0.2], axis=1)
    raise ValueError(kind)


def pin_inputs(n, seed=0):
    """name -> (items, tris) with n pairs a class (the two long-running classes: n / 8)."""
    g = np.random.default_rng(seed)
    return {k: pin_class(k, max(1, n // 8) if k in ("pt_long", "pt_unresolved") else n, g) for k in CLASSES}


def pin_all(n, seed=0):
    """Every class concatenated: (items, tris)."""
    c = pin_inputs(n, seed)
    return np.concatenate([v[0] for v in c.values()]), np.concatenate([v[1] for v in c.values()])


def pin_conditions(items, tris, adv: SegAdvance):
    """What a pin of seg_advance needs of its inputs, asserted from the restatement's own results, so that no branch can go unvisited:
    evaluation counts of 1, of 2, of at least 100 and of exactly MAX_EVALS with an unresolved result; toi of 0, of 1 and strictly between;
    reports with cross = 1 and with cross = 0; every one of seg_tri's term groups (0-7 an end of the segment, 8-10 a vertex of the
    triangle, 11-13 edge against edge) as the reporting term; pairs not reported after one evaluation (L == 0), after two, and after many."""
    it = _items(items)
    rep = np.isfinite(adv.toi)
    unres = rep & (adv.dist > it[:, 12])
    res = rep & ~unres
    L = rate_np(it, tris)
    figures = {
        "evals 1": int((adv.evals == 1).sum()), "evals 2": int((adv.evals == 2).sum()), "evals >= 100": int((adv.evals >= 100).sum()),
        "unresolved": int(unres.sum()), "toi 0": int((adv.toi == 0.0).sum()), "toi 1": int((adv.toi == 1.0).sum()),
        "toi between": int(((adv.toi > 0.0) & (adv.toi < 1.0) & ~unres).sum()), "cross 1": int((res & (adv.cross == 1)).sum()),
        "cross 0": int((res & (adv.cross == 0)).sum()), "terms 0-7": int((res & (adv.term >= 0) & (adv.term < 8)).sum()),
        "terms 8-10": int((res & (adv.term >= 8) & (adv.term < 11)).sum()), "terms 11-13": int((res & (adv.term >= 11)).sum()),
        "L == 0 apart": int(((L == 0.0) & ~rep).sum()), "not reported after 2": int((~rep & (adv.evals == 2)).sum()),
        "not reported after many": int((~rep & (adv.evals >= 100)).sum()),
    }
    print(figures)
    assert all(v > 0 for v in figures.values()), figures
    assert np.all(adv.evals[unres] == MAX_EVALS) and np.all((adv.evals >= 1) & (adv.evals <= MAX_EVALS))
    assert np.all(adv.evals[(L == 0.0)] == 1)
    return figures


M_OF = lambda items, tris: np.maximum(np.abs(_items(items)[:, :12]).max(axis=1), np.abs(_tris(tris).reshape(-1, 18)).max(axis=1))

# | seg_tri.dist - exact distance | <= SEG_TRI_BOUND M on the operands the advancement of the pin classes evaluates (the start, the
# reporting or last position and one between), M the largest |coordinate| of the five points there: the worst case measured against
# exact rationals, 2^-51.00 M (pt_approach; 19 classes x 150 pairs x 3 positions, seeds 3 and 4 of
# tests/test_swept_segment_ref.py measured_seg_tri_error), rounded up to the next power of two.  DESIGN.md section 26 records it.
# DELTA is the guarantee's delta, section 11's, in units of M.
SEG_TRI_BOUND = 2.0 ** -50
DELTA = 2.0 ** -38


# ---------------------------------------------------------------- the items of the mesh tests
MESHES = wr.MESHES
SMALL = wr.SMALL
COUNTS = (1, 63, 64, 65, 1000)


@functools.lru_cache(maxsize=None)
def mesh_end(name):
    """x1 of mesh `name`: every vertex moved by N(0, 0.3 edge) per coordinate."""
    v, i, ids, edge = MESHES[name]
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64) + np.random.default_rng(21).normal(0.0, 0.3 * edge, np.shape(v)))


@functools.lru_cache(maxsize=None)
def items(name, n=None, factor=0.5):
    """[n, 13]: segment_ref's segments of the mesh at the start; each end moves by its own N(0, edge) vector plus a common one; every
    16th has zero length at both ends (a moving point) and every 16th + 1 does not move.  dist = factor * edge."""
    v, i, ids, edge = MESHES[name]
    n = n or sref.n_items(name)
    s = sref.segments(name, n)
    g = np.random.default_rng(31)
    common = g.normal(0.0, edge, (n, 3))
    a1 = s[:, 0:3] + common + g.normal(0.0, 0.5 * edge, (n, 3))
    b1 = s[:, 3:6] + common + g.normal(0.0, 0.5 * edge, (n, 3))
    b1[::16] = a1[::16]
    a1[1::16] = s[1::16, 0:3]; b1[1::16] = s[1::16, 3:6]
    return np.ascontiguousarray(pack(s[:, 0:3], s[:, 3:6], a1, b1, factor * edge))


@functools.lru_cache(maxsize=None)
def want(name, n=None, moving=True):
    """(rows, (gate, evals, unresolved)) of items(name, n) against mesh `name` moving to mesh_end (moving) or standing still."""
    v, i, ids, edge = MESHES[name]
    return sweep_segment_rows_ref(v, mesh_end(name) if moving else None, i, ids, items(name, n), counts=True)
