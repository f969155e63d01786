"""CPU restatement of the witness of the pair queries (include/mi355cd.h cd_find_*_witness / cd_tri_witness_points; csrc/cd_math.h
tri_witness).

tri_witness_np restates the device's tri_witness operation for operation (numpy float64, no contraction, correctly rounded divide and
sqrt): proximity_ref's three blocks, here returning their parameters too, taken in tri_distance's order with the strict-less tie rule,
so dist, the two points, the barycentrics and the features agree with the device bit for bit -- and dist with
proximity_ref.tri_distance_np.  witness_pairs / witness_pairs_between enumerate the rows the four queries report the way
proximity_ref.proximity_pairs, ccd_ref.ccd_pairs and between_ref's do (the same candidates, filters and A / B rule), keeping the FACE
indices of every row, and evaluate the witness where the query evaluated the row's distance.  Rows are sorted by (face_a, face_b).
"""
from __future__ import annotations

import collections

import numpy as np

import between_ref as br
import ccd_ref as cr
import proximity_ref as pr
from proximity_ref import _dot, _sub

FEATURE_NONE = 7

TriWitness = collections.namedtuple("TriWitness", "dist points bary feature win")
Rows = collections.namedtuple("Rows", "faces pairs toi dists points bary feature")


# ---------------------------------------------------------------- proximity_ref's blocks, with their parameters
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
    ok &= (v >= 0.0) & (w >= 0.0) & (v + w <= 1.0)
    q = ((a[0] + v * ab[0]) + w * ac[0], (a[1] + v * ab[1]) + w * ac[1], (a[2] + v * ab[2]) + w * ac[2])
    d = _sub(p, q)
    return np.where(ok, _dot(d, d), np.inf), np.where(ok, v, 0.0), np.where(ok, w, 0.0)


def _seg_seg2_st(p1, q1, p2, q2):
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
    return np.where(ok, _dot(d, d), np.inf), np.where(ok, s, 0.0), np.where(ok, t, 0.0)


def _vertex(i, like):
    """(u, v, feature) of vertex i."""
    return np.full_like(like, 1.0 if i == 1 else 0.0), np.full_like(like, 1.0 if i == 2 else 0.0), 4 + i


def _edge(e, t):
    """(u, v, feature) of the point at parameter t from vertex e on edge e (pt_tri's table)."""
    f = np.where(t > 0.0, np.where(t < 1.0, 1 + e, 4 + (e + 1) % 3), 4 + e)
    z = np.zeros_like(t)
    if e == 0:
        return t, z, f
    if e == 1:
        return 1.0 - t, t, f
    return z, 1.0 - t, f


def _face(v, w):
    return v, w, 0


def tri_witness_np(tri, contact=None) -> TriWitness:
    """tri: f64[n, 6, 3] (A's vertices, then B's) -> (dist[n], points[n, 2, 3], bary[n, 2, 2], feature u8[n, 2], win i8[n]).
    win: the index 11 i + k of the winning term, -1 where there is no witness (feature 7).  contact: the tri_contact verdicts
    (computed with the oracle if None)."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 6, 3)
    n = t.shape[0]
    none = pr.in_contact(t, contact)
    with np.errstate(all="ignore"):
        V = [tuple(t[:, k, a] for a in range(3)) for k in range(6)]
        P1 = V[0]
        p2, p3, q1, q2, q3 = (_sub(V[k], P1) for k in (1, 2, 3, 4, 5))
        m = np.zeros(n)
        for v in (p2, p3, q1, q2, q3):
            for a in range(3):
                x = np.abs(v[a])
                m = np.where(x > m, x, m)
        ex = np.clip(np.frexp(m)[1], -pr.EXP_MAX, pr.EXP_MAX)
        sc = np.ldexp(1.0, -ex)
        p1 = (np.zeros(n),) * 3
        p2, p3, q1, q2, q3 = (tuple(v[a] * sc for a in range(3)) for v in (p2, p3, q1, q2, q3))
        P, Q = (p1, p2, p3), (q1, q2, q3)
        best = np.full(n, np.inf)
        win = np.zeros(n, dtype=np.int8)
        par = [np.zeros(n) for _ in range(4)]                                  # ua va ub vb
        fea = [np.zeros(n, dtype=np.uint8) for _ in range(2)]
        like = np.zeros(n)

        def take(d, idx, A, B):
            nonlocal best, win
            upd = d < best                                                      # strictly smaller: an earlier term keeps a tie
            best = np.where(upd, d, best)
            win = np.where(upd, idx, win).astype(np.int8)
            for k, x in enumerate((A[0], A[1], B[0], B[1])):
                par[k] = np.where(upd, x, par[k])
            fea[0] = np.where(upd, A[2], fea[0]).astype(np.uint8)
            fea[1] = np.where(upd, B[2], fea[1]).astype(np.uint8)

        for i in range(3):
            pi, pn, qi = P[i], P[(i + 1) % 3], Q[i]
            b = 11 * i
            d, v, w = _pt_face2_vw(pi, q1, q2, q3)
            take(d, b, _vertex(i, like), _face(v, w))
            d, v, w = _pt_face2_vw(qi, p1, p2, p3)
            take(d, b + 1, _face(v, w), _vertex(i, like))
            for e in range(3):
                d, s = _pt_seg2_t(pi, Q[e], Q[(e + 1) % 3])
                take(d, b + 2 + e, _vertex(i, like), _edge(e, s))
            for e in range(3):
                d, s = _pt_seg2_t(qi, P[e], P[(e + 1) % 3])
                take(d, b + 5 + e, _edge(e, s), _vertex(i, like))
            for e in range(3):
                d, s, u = _seg_seg2_st(pi, pn, Q[e], Q[(e + 1) % 3])
                take(d, b + 8 + e, _edge(i, s), _edge(e, u))
        dist = np.sqrt(best) * np.ldexp(1.0, ex)
        none = none | ~(m > 0.0)
        dist = np.where(none, 0.0, dist)
        ua, va, ub, vb = (np.where(none, 0.0, x) for x in par)
        feature = np.stack([np.where(none, FEATURE_NONE, fea[0]), np.where(none, FEATURE_NONE, fea[1])], axis=1).astype(np.uint8)
        win = np.where(none, -1, win).astype(np.int8)

        def point(u, v, X):
            w = (1.0 - u) - v
            return np.stack([(w * X[0][a] + u * X[1][a]) + v * X[2][a] for a in range(3)], axis=1)

        qa = np.where(none[:, None], 0.0, point(ua, va, V[:3]))
        qb = np.where(none[:, None], 0.0, point(ub, vb, V[3:]))
    points = np.stack([qa, qb], axis=1)
    bary = np.stack([np.stack([ua, va], axis=1), np.stack([ub, vb], axis=1)], axis=1)
    return TriWitness(dist, points, bary, feature, win)


# ---------------------------------------------------------------- the rows of the four queries
def sort_rows(faces, *arrays):
    """Rows sorted by (face_a, face_b): the order in which witness rows are compared."""
    f = np.asarray(faces, dtype=np.uint32).reshape(-1, 2)
    o = np.lexsort((f[:, 1], f[:, 0]))
    return (f[o],) + tuple(None if a is None else np.asarray(a)[o] for a in arrays)


def positions_at(x0, x1, toi):
    """Where the advancement evaluated a reported row: x1 itself at toi == 1, else a + toi (b - a) per coordinate (ccd_at).
    x0, x1: f64[n, 3, 3], toi: f64[n]."""
    with np.errstate(all="ignore"):
        return np.where((toi == 1.0)[:, None, None], x1, x0 + toi[:, None, None] * (x1 - x0))


def witness_pairs(verts, vidx, ids=None, dist=0.0, verts_end=None, chunk=1 << 18, brute=None) -> Rows:
    """The rows of cd_find_proximity_witness (verts_end None) or cd_find_ccd_witness on one mesh: candidates, neighbour filter and A / B
    rule as proximity_ref.proximity_pairs / ccd_ref.ccd_pairs, with every row's face indices kept.  toi is None for proximity."""
    x0 = np.asarray(verts, dtype=np.float64)
    vidx = np.asarray(vidx, dtype=np.int64).reshape(-1, 3)
    n = vidx.shape[0]
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    ccd = verts_end is not None
    x1 = np.asarray(verts_end, dtype=np.float64) if ccd else x0
    six = np.concatenate([x0[vidx], x1[vidx]], axis=1)
    lo, hi = six.min(axis=1), six.max(axis=1)
    m = float(np.max(np.abs(np.concatenate([lo, hi])))) if n else 0.0
    w = dist + dist / 1024.0 + m / 1024.0
    if brute is None:
        brute = n <= pr.BRUTE_MAX
    if brute:
        i, j = np.triu_indices(n, 1)
        cand = np.stack([i, j], axis=1).astype(np.int64)
    else:
        cand = pr._candidates(lo - w, hi + w)
    out = []
    for c0 in range(0, cand.shape[0], chunk):
        c = cand[c0:c0 + chunk]
        i, j = c[:, 0], c[:, 1]
        sh = (vidx[i][:, :, None] == vidx[j][:, None, :]).any(axis=(1, 2))
        i, j = i[~sh], j[~sh]
        swap = (ids[j] < ids[i]) | ((ids[j] == ids[i]) & (j < i))
        a, b = np.where(swap, j, i), np.where(swap, i, j)
        if ccd:
            g = cr.gate_np(six[a], six[b], dist)
            a, b = a[g], b[g]
            toi, d, _ = cr.advance_np(np.concatenate([x0[vidx[a]], x0[vidx[b]], x1[vidx[a]], x1[vidx[b]]], axis=1), dist)
            ok = np.isfinite(toi)
            a, b, toi, d = a[ok], b[ok], toi[ok], d[ok]
            tri = np.concatenate([positions_at(x0[vidx[a]], x1[vidx[a]], toi), positions_at(x0[vidx[b]], x1[vidx[b]], toi)], axis=1)
        else:
            d = pr.tri_distance_np(np.concatenate([x0[vidx[a]], x0[vidx[b]]], axis=1))
            ok = d <= dist
            a, b, d, toi = a[ok], b[ok], d[ok], None
            tri = np.concatenate([x0[vidx[a]], x0[vidx[b]]], axis=1)
        out.append((a, b, toi, d, tri))
    return _gather(out, ids, ids, ccd)


def witness_pairs_between(va, ia, vb, ib, dist, ids_a=None, ids_b=None, ccd=False, va1=None, vb1=None, chunk=1 << 18, brute=None) -> Rows:
    """The rows of cd_find_proximity_between_witness, or with ccd of cd_find_ccd_between_witness (va1 / vb1 None: that mesh does not
    move): between_ref's candidates and predicates, a's triangle as A, faces indexing each mesh's own list."""
    va0, vb0 = np.asarray(va, dtype=np.float64), np.asarray(vb, dtype=np.float64)
    va1 = va0 if va1 is None else np.asarray(va1, dtype=np.float64)
    vb1 = vb0 if vb1 is None else np.asarray(vb1, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.int64).reshape(-1, 3), np.asarray(ib, dtype=np.int64).reshape(-1, 3)
    ida, idb = br._ids(ids_a, ia.shape[0]), br._ids(ids_b, ib.shape[0])
    sa = np.concatenate([va0[ia], va1[ia] if ccd else va0[ia]], axis=1)
    sb = np.concatenate([vb0[ib], vb1[ib] if ccd else vb0[ib]], axis=1)
    w = br._pad((sa, sb), dist)
    ci, cj = br._cross_candidates(sa.min(axis=1) - w, sa.max(axis=1) + w, sb.min(axis=1) - w, sb.max(axis=1) + w, brute)
    out = []
    for c0 in range(0, ci.shape[0], chunk):
        i, j = ci[c0:c0 + chunk], cj[c0:c0 + chunk]
        if ccd:
            g = cr.gate_np(sa[i], sb[j], dist)
            i, j = i[g], j[g]
            toi, d, _ = cr.advance_np(np.concatenate([sa[i][:, :3], sb[j][:, :3], sa[i][:, 3:], sb[j][:, 3:]], axis=1), dist)
            ok = np.isfinite(toi)
            i, j, toi, d = i[ok], j[ok], toi[ok], d[ok]
            tri = np.concatenate([positions_at(sa[i][:, :3], sa[i][:, 3:], toi), positions_at(sb[j][:, :3], sb[j][:, 3:], toi)], axis=1)
        else:
            d = pr.tri_distance_np(np.concatenate([sa[i][:, :3], sb[j][:, :3]], axis=1))
            ok = d <= dist
            i, j, d, toi = i[ok], j[ok], d[ok], None
            tri = np.concatenate([sa[i][:, :3], sb[j][:, :3]], axis=1)
        out.append((i, j, toi, d, tri))
    return _gather(out, ida, idb, ccd)


def _gather(out, ida, idb, ccd) -> Rows:
    """The chunks' rows (face_a, face_b, toi, d, positions) as one sorted Rows, with the witness of every row."""
    a = np.concatenate([np.zeros(0, np.int64)] + [o[0] for o in out]); b = np.concatenate([np.zeros(0, np.int64)] + [o[1] for o in out])
    toi = np.concatenate([np.zeros(0)] + [o[2] for o in out]) if ccd else None
    d = np.concatenate([np.zeros(0)] + [o[3] for o in out]); tri = np.concatenate([np.zeros((0, 6, 3))] + [o[4] for o in out])
    w = tri_witness_np(tri)
    # one evaluation rule: the row's distance IS the witness's (tests/test_witness_ref.py pins tri_witness_np's dist to tri_distance_np)
    assert np.array_equal(d.view(np.uint64), w.dist.view(np.uint64))
    faces = np.stack([a, b], axis=1).astype(np.uint32)
    pairs = np.stack([ida[a], idb[b]], axis=1).astype(np.uint32)
    return Rows(*sort_rows(faces, pairs, toi, d, w.points, w.bary, w.feature))


# ---------------------------------------------------------------- inputs shared by the CPU and GPU tests
def pin_sets(n, seed=5):
    """name -> f64[n, 6, 3]: the vector sets of the pin (random unit pairs, near pairs, pairs offset by 2^20 + 0.37, integer-grid pairs
    full of ties, slivers, degenerate triangles, pairs in contact)."""
    g = np.random.default_rng(seed)
    out = {}
    a = g.uniform(-1, 1, (n, 6, 3)); a[:, 3:] += g.uniform(-2.5, 2.5, (n, 1, 3))
    out["unit"] = a
    c = g.uniform(-1, 1, (n, 6, 3)); c[:, 3:] = c[:, 3:] * 0.3 + c[:, :3].mean(axis=1, keepdims=True)
    nrm = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]); nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    c[:, 3:] += (nrm * 10.0 ** g.uniform(-6, -0.5, (n, 1)))[:, None, :] + 0.3 * nrm[:, None, :] * np.abs(g.normal(size=(n, 3, 1)))
    out["near"] = c
    out["offset"] = a + (2.0 ** 20 + 0.37)
    k = g.integers(-2, 3, (n, 6, 3)).astype(np.float64); k[:, 3:, 2] = g.integers(3, 5, (n, 3))
    out["grid"] = k
    s = g.uniform(-1, 1, (n, 6, 3)); s[:, 3:] += g.uniform(-1.5, 1.5, (n, 1, 3))
    s[:, 2] = s[:, 0] + g.uniform(-0.5, 1.5, (n, 1)) * (s[:, 1] - s[:, 0]) + g.normal(size=(n, 3)) * 1e-9
    s[: n // 2, 5] = s[: n // 2, 3] + g.uniform(0, 1, (n // 2, 1)) * (s[: n // 2, 4] - s[: n // 2, 3]) + g.normal(size=(n // 2, 3)) * 1e-12
    out["sliver"] = s
    dv, _ = br.with_degenerate(a.reshape(-1, 3), np.zeros((0, 3), np.uint32), seed + 1)
    out["degenerate"] = dv.reshape(n, 6, 3)
    t = g.uniform(-1, 1, (n, 6, 3)); t[:, 3:] = t[:, 3:] * 1.5 + t[:, :3].mean(axis=1, keepdims=True) * 0.8
    t[: max(1, n // 16), 3:] = t[: max(1, n // 16), :3]                        # coincident triangles
    t[:1] = t[0, 0]                                                             # six coincident points
    out["contact"] = t
    return out


def pin_inputs(n, seed=5):
    """The seven sets of pin_sets as one array f64[7 * ceil(n / 7), 6, 3] cut to n rows, the sets interleaved (so every n has them all)."""
    per = (n + 6) // 7
    s = pin_sets(per, seed)
    return np.ascontiguousarray(np.stack(list(s.values()), axis=1).reshape(-1, 6, 3)[:n])


def self_meshes():
    """name -> (verts, vidx, ids, edge): query_meshes' meshes without the three large ones."""
    from query_meshes import _meshes
    return {m[0]: m[1:] for m in _meshes() if m[0] not in ("soup100k", "cloth300", "cloth300d")}


def self_dists(edge):
    """The two distances of the self-proximity cases: 0 (only pairs in contact: rows without a witness) and a quarter of an edge."""
    return (0.0, edge / 4)


def ccd_case(name):
    """(x1, dist) of the self-CCD case on self_meshes()[name]."""
    import scale_inputs
    verts, _, _, edge = self_meshes()[name]
    x1 = scale_inputs.motion(verts, edge) if name == "soup10k" else br.motion(verts, 0.3 * edge, 11)
    return x1, edge / 8


def between_cases():
    """name -> (va, ia, vb, ib, dist): two soups of 63 and 65 triangles, and cloth100 split in two."""
    import mi355_synth as synth
    va, ia = br.soup(63, 0.3, 31)
    vb, ib = br.soup(65, 0.3, 32)
    v, i = synth.cloth_pair(100)
    ca, cia, cb, cib = br.split(v, i, i.shape[0] // 2)                         # sheet A, sheet B (no vertex is shared across the cut)
    return {"soups": (va, ia, vb, ib, 0.15), "cloth100": (ca, cia, cb, cib, 2.88 / 100 / 8)}


_cache = {}


def cached(key, fn):
    """fn() computed once per process and key: the references the tests share (never modified by them)."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def sort_by_ids(pairs, *vals):
    """Rows sorted by (ID, ID, then the values' bits): the order in which a witness call's (pairs, toi, dists) are compared with the
    plain call's (repeated IDs make (ID, ID) alone ambiguous).  Values come back as their bit patterns."""
    p = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
    bits = [np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) for v in vals]
    o = np.lexsort(bits[::-1] + [p[:, 1], p[:, 0]])
    return (p[o],) + tuple(b[o] for b in bits)
