"""CPU restatement of the self-proximity query (include/mi355cd.h cd_find_proximity; csrc/cd_math.h tri_distance).

tri_distance_np restates the device's FP64 tri_distance operation for operation (numpy float64: IEEE round-to-nearest,
no contraction, correctly rounded divide and sqrt), so the two agree bit for bit; the contact predicate comes from the
oracle's tri_contact (oracle.tri_contact_points).  proximity_pairs enumerates candidates on its own, without the device's
tree -- every pair of a mesh of up to BRUTE_MAX triangles, else a uniform grid over boxes widened by a slack ~1000 x the
device's -- and applies the same definition.
exact_d2 is the exact rational minimum of the 15 feature-pair squared distances: the yardstick of the restatement.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import oracle

EXP_MAX = 1000          # cd_math.h TRI_DIST_EXP_MAX


# ---------------------------------------------------------------- FP64 restatement (arrays of shape [n] per coordinate)
def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _pt_seg2(p, a, b):
    ab, ap = _sub(b, a), _sub(p, a)
    den = _dot(ab, ab)
    pos = den > 0.0
    t = np.where(pos, _dot(ap, ab) / np.where(pos, den, 1.0), 0.0)
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    q = (a[0] + t * ab[0], a[1] + t * ab[1], a[2] + t * ab[2])
    d = _sub(p, q)
    return _dot(d, d)


def _pt_face2(p, a, b, c):
    ab, ac, ap = _sub(b, a), _sub(c, a), _sub(p, a)
    d00, d01, d11, d20, d21 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac), _dot(ap, ab), _dot(ap, ac)
    den = d00 * d11 - d01 * d01
    ok = den > 0.0
    dd = np.where(ok, den, 1.0)
    v = (d11 * d20 - d01 * d21) / dd
    w = (d00 * d21 - d01 * d20) / dd
    ok &= (v >= 0.0) & (w >= 0.0) & (v + w <= 1.0)
    q = ((a[0] + v * ab[0]) + w * ac[0], (a[1] + v * ab[1]) + w * ac[1], (a[2] + v * ab[2]) + w * ac[2])
    d = _sub(p, q)
    return np.where(ok, _dot(d, d), np.inf)


def _seg_seg2(p1, q1, p2, q2):
    d1, d2, r = _sub(q1, p1), _sub(q2, p2), _sub(p1, p2)
    a, e, b, c, f = _dot(d1, d1), _dot(d2, d2), _dot(d1, d2), _dot(d1, r), _dot(d2, r)
    den = a * e - b * b
    ok = den > 0.0
    dd = np.where(ok, den, 1.0)
    s = (b * f - c * e) / dd
    t = (a * f - b * c) / dd
    ok &= (s >= 0.0) & (s <= 1.0) & (t >= 0.0) & (t <= 1.0)
    P = (p1[0] + s * d1[0], p1[1] + s * d1[1], p1[2] + s * d1[2])
    Q = (p2[0] + t * d2[0], p2[1] + t * d2[1], p2[2] + t * d2[2])
    d = _sub(P, Q)
    return np.where(ok, _dot(d, d), np.inf)


def in_contact(tri, contact=None) -> np.ndarray:
    """The pairs tri_distance puts at 0: strict overlap of the FP64 boxes in box.cuh's product form AND tri_contact (the oracle's,
    or the verdicts passed in) -- what the collision path calls in contact."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 6, 3)
    if contact is None:
        contact = oracle.tri_contact_points(t.reshape(-1, 18)) if t.shape[0] else np.zeros(0, dtype=np.int32)
    a_lo, a_hi, b_lo, b_hi = t[:, :3].min(axis=1), t[:, :3].max(axis=1), t[:, 3:].min(axis=1), t[:, 3:].max(axis=1)
    with np.errstate(all="ignore"):
        ov = np.all((a_lo - b_hi) * (b_lo - a_hi) > 0, axis=1)
    return ov & (np.asarray(contact) != 0)


def tri_distance_np(tri, contact=None) -> np.ndarray:
    """tri: f64[n, 6, 3] (A's vertices, then B's).  contact: the tri_contact verdicts (computed with the oracle if None)."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 6, 3)
    zero = in_contact(t, contact)
    with np.errstate(all="ignore"):
        V = [tuple(t[:, k, a] for a in range(3)) for k in range(6)]
        P1 = V[0]
        p2, p3, q1, q2, q3 = (_sub(V[k], P1) for k in (1, 2, 3, 4, 5))
        m = np.zeros(t.shape[0])
        for v in (p2, p3, q1, q2, q3):
            for a in range(3):
                x = np.abs(v[a])
                m = np.where(x > m, x, m)
        ex = np.clip(np.frexp(m)[1], -EXP_MAX, EXP_MAX)
        sc = np.ldexp(1.0, -ex)
        p1 = (np.zeros_like(m),) * 3
        p2, p3, q1, q2, q3 = (tuple(v[a] * sc for a in range(3)) for v in (p2, p3, q1, q2, q3))
        P, Q = (p1, p2, p3), (q1, q2, q3)
        best = np.full(t.shape[0], np.inf)
        for i in range(3):
            pi, pn, qi = P[i], P[(i + 1) % 3], Q[i]
            terms = [_pt_face2(pi, q1, q2, q3), _pt_face2(qi, p1, p2, p3),
                     _pt_seg2(pi, q1, q2), _pt_seg2(pi, q2, q3), _pt_seg2(pi, q3, q1),
                     _pt_seg2(qi, p1, p2), _pt_seg2(qi, p2, p3), _pt_seg2(qi, p3, p1),
                     _seg_seg2(pi, pn, q1, q2), _seg_seg2(pi, pn, q2, q3), _seg_seg2(pi, pn, q3, q1)]
            for x in terms:
                best = np.where(x < best, x, best)
        d = np.sqrt(best) * np.ldexp(1.0, ex)
    d = np.where(m > 0.0, d, 0.0)
    return np.where(zero, 0.0, d)


# ---------------------------------------------------------------- exact rationals
def _fsub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _fdot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _e_pt_seg(p, a, b):
    ab, ap = _fsub(b, a), _fsub(p, a)
    den = _fdot(ab, ab)
    t = Fraction(0)
    if den > 0:
        t = min(max(_fdot(ap, ab) / den, Fraction(0)), Fraction(1))
    d = _fsub(p, (a[0] + t * ab[0], a[1] + t * ab[1], a[2] + t * ab[2]))
    return _fdot(d, d)


def _e_pt_face(p, a, b, c):
    ab, ac, ap = _fsub(b, a), _fsub(c, a), _fsub(p, a)
    d00, d01, d11, d20, d21 = _fdot(ab, ab), _fdot(ab, ac), _fdot(ac, ac), _fdot(ap, ab), _fdot(ap, ac)
    den = d00 * d11 - d01 * d01
    if den == 0:
        return None
    v = (d11 * d20 - d01 * d21) / den
    w = (d00 * d21 - d01 * d20) / den
    if v < 0 or w < 0 or v + w > 1:
        return None
    d = _fsub(p, tuple(a[k] + v * ab[k] + w * ac[k] for k in range(3)))
    return _fdot(d, d)


def _e_seg_seg(p1, q1, p2, q2):
    d1, d2, r = _fsub(q1, p1), _fsub(q2, p2), _fsub(p1, p2)
    a, e, b, c, f = _fdot(d1, d1), _fdot(d2, d2), _fdot(d1, d2), _fdot(d1, r), _fdot(d2, r)
    den = a * e - b * b
    if den == 0:
        return None
    s = (b * f - c * e) / den
    t = (a * f - b * c) / den
    if not (0 <= s <= 1 and 0 <= t <= 1):
        return None
    d = _fsub(tuple(p1[k] + s * d1[k] for k in range(3)), tuple(p2[k] + t * d2[k] for k in range(3)))
    return _fdot(d, d)


def exact_d2(pair) -> Fraction:
    """Exact minimum over the 15 feature pairs of the squared distance (6 vertex-triangle, 9 edge-edge) of one pair
    f64[6, 3]: the squared distance of the two triangles whenever they do not intersect."""
    v = [tuple(Fraction(float(x)) for x in row) for row in np.asarray(pair, dtype=np.float64).reshape(6, 3)]
    P, Q = v[:3], v[3:]
    vals = []
    for X, Y in ((P, Q), (Q, P)):
        for p in X:
            vals.append(_e_pt_face(p, *Y))
            for k in range(3):
                vals.append(_e_pt_seg(p, Y[k], Y[(k + 1) % 3]))
    for i in range(3):
        for k in range(3):
            vals.append(_e_seg_seg(P[i], P[(i + 1) % 3], Q[k], Q[(k + 1) % 3]))
    return min(x for x in vals if x is not None)


# ---------------------------------------------------------------- the query
def _candidates(lo, hi, qsel=None, chunk=1 << 16):
    """Index pairs (i, j), i < j, whose boxes [lo, hi] overlap (closed), via a uniform grid of cells at least as large as
    every box; qsel: only pairs with i or j in it."""
    n = lo.shape[0]
    if n < 2:
        return np.zeros((0, 2), dtype=np.int64)
    h = np.max(hi - lo, axis=0)
    h = np.where(h > 0, h, 1.0) * (1.0 + 1e-9)
    g0 = lo.min(axis=0)
    cell = np.floor((lo - g0) / h).astype(np.int64)
    dims = cell.max(axis=0) + 3
    key = ((cell[:, 0] + 1) * dims[1] + (cell[:, 1] + 1)) * dims[2] + (cell[:, 2] + 1)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    qs = np.arange(n) if qsel is None else np.unique(np.asarray(qsel, dtype=np.int64))
    out = []
    for c0 in range(0, qs.shape[0], chunk):
        q = qs[c0:c0 + chunk]
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    k = ((cell[q, 0] + 1 + dx) * dims[1] + (cell[q, 1] + 1 + dy)) * dims[2] + (cell[q, 2] + 1 + dz)
                    a = np.searchsorted(skey, k, "left")
                    b = np.searchsorted(skey, k, "right")
                    cnt = b - a
                    if cnt.sum() == 0:
                        continue
                    qi = np.repeat(q, cnt)
                    pos = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(a, cnt)
                    oj = order[pos]
                    keep = (qi != oj) & np.all(lo[qi] <= hi[oj], axis=1) & np.all(lo[oj] <= hi[qi], axis=1)
                    i, j = qi[keep], oj[keep]
                    out.append(np.stack([np.minimum(i, j), np.maximum(i, j)], axis=1))
    if not out:
        return np.zeros((0, 2), dtype=np.int64)
    c = np.concatenate(out)
    return np.unique(c, axis=0)


BRUTE_MAX = 2000        # up to this many triangles proximity_pairs evaluates EVERY pair: no box filter at all decides anything there


def proximity_pairs(verts, vidx, ids=None, dist=0.0, queries=None, chunk=1 << 20, brute=None):
    """Every unordered pair with no shared vertex index and tri_distance <= dist: (pairs u32[n, 2] (smaller ID, larger ID),
    dists f64[n]), rows sorted by (ID, ID).  queries: face indices -- only the pairs with a triangle among them.  brute: all
    n (n - 1) / 2 pairs instead of the grid's candidates (default: meshes of up to BRUTE_MAX triangles)."""
    verts = np.asarray(verts, dtype=np.float64)
    vidx = np.asarray(vidx, dtype=np.int64).reshape(-1, 3)
    n = vidx.shape[0]
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    tv = verts[vidx]                                                            # [n, 3, 3]
    lo, hi = tv.min(axis=1), tv.max(axis=1)
    m = float(np.max(np.abs(np.concatenate([lo, hi])))) if n else 0.0
    w = dist + dist / 1024.0 + m / 1024.0                                       # the device's slack is 2^-20
    if brute is None:
        brute = n <= BRUTE_MAX
    if brute:
        i, j = np.triu_indices(n, 1)
        cand = np.stack([i, j], axis=1).astype(np.int64)
        if queries is not None:
            cand = cand[np.isin(cand[:, 0], queries) | np.isin(cand[:, 1], queries)]
    else:
        cand = _candidates(lo - w, hi + w, queries)
    pairs, dists = [np.zeros((0, 2), dtype=np.uint32)], [np.zeros(0)]
    for c0 in range(0, cand.shape[0], chunk):
        c = cand[c0:c0 + chunk]
        i, j = c[:, 0], c[:, 1]
        sh = (vidx[i][:, :, None] == vidx[j][:, None, :]).any(axis=(1, 2))
        i, j = i[~sh], j[~sh]
        swap = (ids[j] < ids[i]) | ((ids[j] == ids[i]) & (j < i))
        a, b = np.where(swap, j, i), np.where(swap, i, j)
        d = tri_distance_np(np.concatenate([tv[a], tv[b]], axis=1))
        ok = d <= dist
        pairs.append(np.stack([ids[a][ok], ids[b][ok]], axis=1).astype(np.uint32))
        dists.append(d[ok])
    return sort_pairs(np.concatenate(pairs), np.concatenate(dists))


def sort_pairs(pairs, dists):
    """Rows sorted by (first, second): the canonical order in which pair lists and their distances are compared."""
    p = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    o = np.lexsort((p[:, 1], p[:, 0]))
    return p[o], np.asarray(dists, dtype=np.float64)[o]
