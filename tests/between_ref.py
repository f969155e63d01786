"""CPU restatement of the queries between two meshes (include/mi355cd.h cd_find_collisions_between, cd_find_proximity_between,
cd_find_ccd_between; csrc/cd_between.h).

Built only from what is pinned elsewhere: the oracle's tri_contact (oracle.tri_contact_points) and box.cuh's strict product-form box
test (as proximity_ref.in_contact states it), proximity_ref.tri_distance_np, ccd_ref.gate_np and ccd_ref.advance_np.  A pair is (a's
triangle, b's triangle) with a's triangle first in every predicate; there is no neighbour filter (the vertex arrays are separate).
Candidates are enumerated without the device's trees: every a x b pair when there are at most BRUTE_MAX of them, else the cross pairs
of a uniform grid over both meshes' boxes widened ~1000 x the device's slack.  Results: pairs (ID in a, ID in b) sorted by (a ID, b ID)
with their distances or times.
"""
from __future__ import annotations

import numpy as np

import ccd_ref as cr
import oracle
import proximity_ref as pr

BRUTE_MAX = 1 << 20     # up to this many a x b pairs every pair is evaluated


def _ids(ids, n):
    return np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)


def _cross_candidates(lo_a, hi_a, lo_b, hi_b, brute=None):
    """(i in a, j in b) index pairs: all of them, or those whose boxes (already widened) overlap, closed."""
    na, nb = lo_a.shape[0], lo_b.shape[0]
    if brute is None:
        brute = na * nb <= BRUTE_MAX
    if brute:
        i, j = np.meshgrid(np.arange(na, dtype=np.int64), np.arange(nb, dtype=np.int64), indexing="ij")
        return i.ravel(), j.ravel()
    c = pr._candidates(np.concatenate([lo_a, lo_b]), np.concatenate([hi_a, hi_b]))
    c = c[(c[:, 0] < na) & (c[:, 1] >= na)]
    return c[:, 0], c[:, 1] - na


def _pad(boxes, dist):
    m = max(float(np.max(np.abs(b))) if b.size else 0.0 for b in boxes)
    return dist + dist / 1024.0 + m / 1024.0


def strict_overlap(tri_a, tri_b) -> np.ndarray:
    """box.cuh:40-43 on the FP64 boxes of tri_a[n, 3, 3] and tri_b[n, 3, 3]: (a.lo - b.hi) (b.lo - a.hi) > 0 on every axis."""
    a_lo, a_hi, b_lo, b_hi = tri_a.min(axis=1), tri_a.max(axis=1), tri_b.min(axis=1), tri_b.max(axis=1)
    with np.errstate(all="ignore"):
        return np.all((a_lo - b_hi) * (b_lo - a_hi) > 0, axis=1)


def contact_pairs(va, ia, vb, ib, ids_a=None, ids_b=None, chunk=1 << 18, brute=None):
    """cd_find_collisions_between: (pairs u32[n, 2] (ID in a, ID in b) sorted, n_tested = pairs whose FP64 boxes overlap strictly)."""
    va, vb = np.asarray(va, dtype=np.float64), np.asarray(vb, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.int64).reshape(-1, 3), np.asarray(ib, dtype=np.int64).reshape(-1, 3)
    ida, idb = _ids(ids_a, ia.shape[0]), _ids(ids_b, ib.shape[0])
    ta, tb = va[ia], vb[ib]
    w = _pad((ta, tb), 0.0)
    ci, cj = _cross_candidates(ta.min(axis=1) - w, ta.max(axis=1) + w, tb.min(axis=1) - w, tb.max(axis=1) + w, brute)
    out, tested = [np.zeros((0, 2), dtype=np.uint32)], 0
    for c0 in range(0, ci.shape[0], chunk):
        i, j = ci[c0:c0 + chunk], cj[c0:c0 + chunk]
        ov = strict_overlap(ta[i], tb[j])
        i, j = i[ov], j[ov]
        tested += int(i.shape[0])
        if not i.shape[0]:
            continue
        hit = oracle.tri_contact_points(np.concatenate([ta[i], tb[j]], axis=1).reshape(-1, 18)) != 0
        out.append(np.stack([ida[i][hit], idb[j][hit]], axis=1).astype(np.uint32))
    p, _ = pr.sort_pairs(np.concatenate(out), np.zeros(sum(x.shape[0] for x in out)))
    return p, tested


def proximity_pairs(va, ia, vb, ib, dist, ids_a=None, ids_b=None, chunk=1 << 18, brute=None):
    """cd_find_proximity_between: (pairs u32[n, 2] (ID in a, ID in b), dists f64[n]) sorted, tri_distance(a, b) <= dist."""
    va, vb = np.asarray(va, dtype=np.float64), np.asarray(vb, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.int64).reshape(-1, 3), np.asarray(ib, dtype=np.int64).reshape(-1, 3)
    ida, idb = _ids(ids_a, ia.shape[0]), _ids(ids_b, ib.shape[0])
    ta, tb = va[ia], vb[ib]
    w = _pad((ta, tb), dist)
    ci, cj = _cross_candidates(ta.min(axis=1) - w, ta.max(axis=1) + w, tb.min(axis=1) - w, tb.max(axis=1) + w, brute)
    out_p, out_d = [np.zeros((0, 2), dtype=np.uint32)], [np.zeros(0)]
    for c0 in range(0, ci.shape[0], chunk):
        i, j = ci[c0:c0 + chunk], cj[c0:c0 + chunk]
        if not i.shape[0]:
            continue
        d = pr.tri_distance_np(np.concatenate([ta[i], tb[j]], axis=1))
        ok = d <= dist
        out_p.append(np.stack([ida[i][ok], idb[j][ok]], axis=1).astype(np.uint32))
        out_d.append(d[ok])
    return pr.sort_pairs(np.concatenate(out_p), np.concatenate(out_d))


def ccd_pairs(va0, ia, vb0, ib, dist, va1=None, vb1=None, ids_a=None, ids_b=None, chunk=1 << 16, brute=None, counts=False):
    """cd_find_ccd_between: (pairs u32[n, 2] (ID in a, ID in b), toi f64[n], dists f64[n]) sorted.  va1 / vb1 None: that mesh does not
    move.  counts: also (pairs through the gate, evaluations)."""
    va0, vb0 = np.asarray(va0, dtype=np.float64), np.asarray(vb0, dtype=np.float64)
    va1 = va0 if va1 is None else np.asarray(va1, dtype=np.float64)
    vb1 = vb0 if vb1 is None else np.asarray(vb1, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.int64).reshape(-1, 3), np.asarray(ib, dtype=np.int64).reshape(-1, 3)
    ida, idb = _ids(ids_a, ia.shape[0]), _ids(ids_b, ib.shape[0])
    sa = np.concatenate([va0[ia], va1[ia]], axis=1)                            # [na, 6, 3]: x0 then x1
    sb = np.concatenate([vb0[ib], vb1[ib]], axis=1)
    w = _pad((sa, sb), dist)
    ci, cj = _cross_candidates(sa.min(axis=1) - w, sa.max(axis=1) + w, sb.min(axis=1) - w, sb.max(axis=1) + w, brute)
    out_p, out_t, out_d = [np.zeros((0, 2), dtype=np.uint32)], [np.zeros(0)], [np.zeros(0)]
    tested = evals = 0
    for c0 in range(0, ci.shape[0], chunk):
        i, j = ci[c0:c0 + chunk], cj[c0:c0 + chunk]
        g = cr.gate_np(sa[i], sb[j], dist)
        i, j = i[g], j[g]
        tested += int(i.shape[0])
        if not i.shape[0]:
            continue
        tri = np.concatenate([sa[i][:, :3], sb[j][:, :3], sa[i][:, 3:], sb[j][:, 3:]], axis=1)
        toi, d, ev = cr.advance_np(tri, dist)
        evals += int(ev.sum())
        ok = np.isfinite(toi)
        out_p.append(np.stack([ida[i][ok], idb[j][ok]], axis=1).astype(np.uint32))
        out_t.append(toi[ok])
        out_d.append(d[ok])
    res = cr.sort_pairs(np.concatenate(out_p), np.concatenate(out_t), np.concatenate(out_d))
    return (res, (tested, evals)) if counts else res


def split(verts, vidx, k):
    """A mesh of private-vertex triangles (a soup) cut into a = its first k triangles and b = the rest, each with its own 0-based vertex
    array: (va, ia, vb, ib).  Vertices that no triangle of a side uses are dropped from that side."""
    verts = np.asarray(verts, dtype=np.float64)
    vidx = np.asarray(vidx, dtype=np.int64).reshape(-1, 3)
    out = []
    for part in (vidx[:k], vidx[k:]):
        used, inv = np.unique(part.ravel(), return_inverse=True)
        out += [np.ascontiguousarray(verts[used]), inv.reshape(-1, 3).astype(np.uint32)]
    return tuple(out)


def merge(va, ia, vb, ib):
    """The merged mesh of the equivalence: a's vertices and triangles first, b's vertices offset by a's nv."""
    va, vb = np.asarray(va, dtype=np.float64), np.asarray(vb, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.int64).reshape(-1, 3), np.asarray(ib, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([va, vb]), np.concatenate([ia, ib + va.shape[0]]).astype(np.uint32)


def cross(pairs, na, *vals):
    """The rows of a merged-mesh self result (smaller ID first, face index = ID) with one triangle in a and one in b, as
    (ID in a, ID in b), plus the same rows of `vals`."""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    keep = (p[:, 0] < na) & (p[:, 1] >= na)
    q = np.stack([p[keep, 0], p[keep, 1] - na], axis=1).astype(np.uint32)
    return (q,) + tuple(np.asarray(v)[keep] for v in vals)


# ---------------------------------------------------------------- inputs shared by the CPU and GPU tests
def soup(n, e, seed, lo=0.0, hi=1.0):
    """n triangles of private vertices, centroid uniform in [lo, hi]^3, vertices centroid + U(-e/2, e/2)^3, rounded to fp32."""
    g = np.random.default_rng(seed)
    c = lo + (hi - lo) * g.random((n, 3))
    v = (c[:, None, :] + (g.random((n, 3, 3)) - 0.5) * e).reshape(-1, 3)
    return np.ascontiguousarray(v.astype(np.float32).astype(np.float64)), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def shared_positions(n, seed):
    """Two meshes that share vertex POSITIONS but no indices: b reuses a's corner positions in new triangles (fans through a's
    vertices, coincident copies of some of a's triangles, triangles with one vertex on a's); a is a small grid sheet with shared
    vertices inside it.  (va, ia, vb, ib)."""
    g = np.random.default_rng(seed)
    q = max(2, int(np.sqrt(n / 2)))
    xs = np.linspace(0.0, 1.0, q + 1)
    X, Z = np.meshgrid(xs, xs, indexing="ij")
    va = np.stack([X.ravel(), 0.05 * np.sin(5 * X.ravel()) * np.cos(4 * Z.ravel()), Z.ravel()], axis=1)
    va = va.astype(np.float32).astype(np.float64)
    k = np.arange(q + 1) [:, None] * (q + 1) + np.arange(q + 1)[None, :]
    a0, a1, a2, a3 = k[:-1, :-1].ravel(), k[1:, :-1].ravel(), k[1:, 1:].ravel(), k[:-1, 1:].ravel()
    ia = np.concatenate([np.stack([a0, a1, a2], 1), np.stack([a0, a2, a3], 1)]).astype(np.uint32)
    m = ia.shape[0]
    pick = g.choice(m, size=m // 3, replace=False)
    copies = va[ia[pick]]                                                       # coincident copies
    fans = va[ia[g.choice(m, size=m // 3)]].copy()
    fans[:, 2] = fans[:, 2] + g.normal(0.0, 0.02, (fans.shape[0], 3))             # one vertex off the sheet, two on a's vertices
    fans = fans.astype(np.float32).astype(np.float64)
    pts = va[g.choice(va.shape[0], size=m // 3)]
    touch = np.stack([pts, pts + g.normal(0.0, 0.03, pts.shape), pts + g.normal(0.0, 0.03, pts.shape)], axis=1)
    touch = touch.astype(np.float32).astype(np.float64)                         # one vertex on a's vertex
    tb = np.concatenate([copies, fans, touch])
    return va, ia, np.ascontiguousarray(tb.reshape(-1, 3)), np.arange(3 * tb.shape[0], dtype=np.uint32).reshape(-1, 3)


def with_degenerate(verts, vidx, seed):
    """A copy of a private-vertex mesh in which a third of the triangles are degenerate: a repeated vertex, collinear vertices, a point."""
    v = np.array(verts, dtype=np.float64).reshape(-1, 3, 3)
    g = np.random.default_rng(seed)
    n = v.shape[0]
    sel = g.permutation(n)[: max(3, n // 3)]
    k = sel.shape[0] // 3
    v[sel[:k], 1] = v[sel[:k], 0]
    s = sel[k:2 * k]
    v[s, 2] = (v[s, 0] + 0.375 * (v[s, 1] - v[s, 0])).astype(np.float32).astype(np.float64)
    s = sel[2 * k:]
    v[s, 1] = v[s, 0]; v[s, 2] = v[s, 0]
    return np.ascontiguousarray(v.reshape(-1, 3)), np.asarray(vidx, dtype=np.uint32)


def motion(verts, scale, seed):
    """x1 = x0 + N(0, scale) per coordinate."""
    return np.asarray(verts, dtype=np.float64) + np.random.default_rng(seed).normal(0.0, scale, np.shape(verts))
