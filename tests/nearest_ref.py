"""CPU restatement of the nearest-triangle and separation-distance queries between two meshes (include/mi355cd.h cd_nearest_between;
csrc/cd_nearest.h).

Built only from what is pinned elsewhere.  The definition is rows_of_all_pairs: witness_ref.witness_pairs_between, which evaluates
tri_distance and tri_witness (a's triangle first) on EVERY a x b pair up to between_ref.BRUTE_MAX pairs and keeps the rows with
dist <= rmax, with their face indices, IDs, distance bits and witness, reduced per face of a by (dist, ID of b, face of b).
nearest_rows gives the same rows with the witness of the winners only (tests/test_nearest_ref.py compares the two); within derives the
rows of a smaller radius; nearest_min reduces rows to the one with the smallest (dist, ID a, face a, ID b, face b).  No tree, no box
filter, no bound.
"""
from __future__ import annotations

import collections

import numpy as np

import between_ref as br
import proximity_ref as pr
import witness_ref as wr

NONE = 0xFFFFFFFF

# faces u32[n, 2], ids u32[n, 2], dist f64[n], points f64[n, 2, 3], bary f64[n, 2, 2], feature u8[n, 2]
NearestRows = collections.namedtuple("NearestRows", "faces ids dist points bary feature")


def nothing(n) -> NearestRows:
    """n rows that found nothing: faces NONE, dist +inf, every other output 0."""
    return NearestRows(np.full((n, 2), NONE, dtype=np.uint32), np.zeros((n, 2), dtype=np.uint32), np.full(n, np.inf),
                       np.zeros((n, 2, 3)), np.zeros((n, 2, 2)), np.zeros((n, 2), dtype=np.uint8))


def joint_diameter(va, vb) -> float:
    """The diagonal of the box around both vertex sets: no two points of the meshes are farther apart."""
    v = np.concatenate([np.asarray(va, dtype=np.float64).reshape(-1, 3), np.asarray(vb, dtype=np.float64).reshape(-1, 3)])
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


def rows_of_all_pairs(va, ia, vb, ib, rmax, ids_a=None, ids_b=None, brute=None) -> NearestRows:
    """The definition, as it is written: the rows of witness_ref.witness_pairs_between(..., dist = rmax) -- the witness of EVERY pair
    within rmax -- reduced per face of a by (dist, ID of b, face of b)."""
    na = np.asarray(ia).reshape(-1, 3).shape[0]
    rows = wr.witness_pairs_between(va, ia, vb, ib, _radius(va, vb, rmax), ids_a, ids_b, brute=brute)
    out = nothing(na)
    first = _first_per_face(rows.faces[:, 0], rows.dists, rows.pairs[:, 1], rows.faces[:, 1])
    i = rows.faces[first, 0].astype(np.int64)
    for dst, src in zip(out, (rows.faces, rows.pairs, rows.dists, rows.points, rows.bary, rows.feature)):
        dst[i] = src[first]
    return out


def _radius(va, vb, rmax):
    """rmax = +inf is restated with a finite radius above the joint diameter (tri_distance exceeds the true distance by rounding at
    most, so twice the diameter holds every pair)."""
    return 2.0 * joint_diameter(va, vb) + 1e-300 if np.isinf(rmax) else float(rmax)


def _first_per_face(fa, d, idb, fb):
    """Of rows (face a, dist, ID b, face b): the index of the smallest (dist, ID b, face b) of every face of a that has a row."""
    if fa.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    fa = fa.astype(np.int64)
    o = np.lexsort((fb.astype(np.int64), idb.astype(np.int64), d, fa))
    return o[np.concatenate([[True], fa[o][1:] != fa[o][:-1]])]


def nearest_rows(va, ia, vb, ib, rmax, ids_a=None, ids_b=None, chunk=1 << 18) -> NearestRows:
    """cd_nearest_between, flags = 0: row i for face i of a.  The same rows as rows_of_all_pairs (tests/test_nearest_ref.py compares the
    two), computed with the witness of the WINNERS only: proximity_ref.tri_distance_np on every a x b pair (no filter of any kind), the
    reduction, then witness_ref.tri_witness_np on the na winning pairs, whose dist must be the reduced distance bit for bit
    (tri_witness's contract)."""
    va, vb = np.asarray(va, dtype=np.float64), np.asarray(vb, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.int64).reshape(-1, 3), np.asarray(ib, dtype=np.int64).reshape(-1, 3)
    na, nb = ia.shape[0], ib.shape[0]
    ida, idb = br._ids(ids_a, na), br._ids(ids_b, nb)
    ta, tb = va[ia], vb[ib]
    r = _radius(va, vb, rmax)
    out = nothing(na)
    per = max(1, chunk // nb)
    for a0 in range(0, na, per):                                               # whole faces of a per chunk: the reduction is per chunk
        i = np.repeat(np.arange(a0, min(a0 + per, na), dtype=np.int64), nb)
        j = np.tile(np.arange(nb, dtype=np.int64), i.shape[0] // nb)
        d = pr.tri_distance_np(np.concatenate([ta[i], tb[j]], axis=1))
        ok = d <= r
        i, j, d = i[ok], j[ok], d[ok]
        first = _first_per_face(i, d, idb[j], j)
        fa, fb = i[first], j[first]
        w = wr.tri_witness_np(np.concatenate([ta[fa], tb[fb]], axis=1))
        assert np.array_equal(w.dist.view(np.uint64), d[first].view(np.uint64))
        out.faces[fa] = np.stack([fa, fb], axis=1)
        out.ids[fa] = np.stack([ida[fa], idb[fb]], axis=1)
        out.dist[fa] = d[first]
        out.points[fa] = w.points
        out.bary[fa] = w.bary
        out.feature[fa] = w.feature
    return out


def within(rows: NearestRows, rmax) -> NearestRows:
    """The rows of a smaller radius from those of a larger one: a face's nearest triangle is within rmax or nothing is (the triangles
    within rmax are a subset containing every smaller (dist, ID, face))."""
    n = rows.dist.shape[0]
    keep = (rows.faces[:, 0] != NONE) & (rows.dist <= rmax)
    out = nothing(n)
    for dst, src in zip(out, rows):
        dst[keep] = src[keep]
    return out


def nearest_min(rows: NearestRows) -> NearestRows:
    """cd_nearest_between, CD_NEAREST_MIN: the one row with the smallest (dist, ID a, face a, ID b, face b), or the "nothing" row."""
    found = np.nonzero(rows.faces[:, 0] != NONE)[0]
    if found.size == 0:
        return nothing(1)
    k = rows
    o = np.lexsort((k.faces[found, 1], k.ids[found, 1], k.faces[found, 0], k.ids[found, 0], k.dist[found]))
    w = found[o[:1]]
    return NearestRows(*(x[w].copy() for x in rows))


# ---------------------------------------------------------------- inputs shared by the CPU and GPU tests
def between_cases():
    """name -> (va, ia, vb, ib): the small cases of the between-mesh tests (tests/test_between_gpu.py builds the same), the smallest
    shapes at which the no-records, two-leaf and partial-wave paths differ."""
    out = {}
    for na, nb, e, seed in ((1, 1, 0.5, 1), (1, 400, 0.15, 2), (400, 1, 0.15, 3), (2, 600, 0.12, 4), (700, 900, 0.06, 5), (1500, 500, 0.05, 6)):
        v, i = br.soup(na + nb, e, seed)
        out[f"soup_{na}_{nb}_s{seed}"] = br.split(v, i, na)
    va, ia = br.soup(300, 0.05, 7, 0.0, 1.0)
    vb, ib = br.soup(300, 0.05, 8, 3.0, 4.0)
    out["disjoint"] = (va, ia, vb, ib)
    out["shared_positions"] = br.shared_positions(200, 9)
    v, i = br.with_degenerate(*br.soup(900, 0.1, 10), seed=10)
    out["degenerate"] = br.split(v, i, 400)
    return out


def doubled(vb, ib):
    """b with every triangle twice: (vb2, ib2), face j and face j + nb coincide."""
    vb = np.asarray(vb, dtype=np.float64)
    ib = np.asarray(ib, dtype=np.uint32).reshape(-1, 3)
    return np.concatenate([vb, vb]), np.concatenate([ib, ib + vb.shape[0]]).astype(np.uint32)
