"""CPU restatement of the self-nearest queries (include/mi355cd.h cd_nearest_self; csrc/cd_nearest.h k_nearest_self): for every triangle
of a mesh the nearest triangle of the same mesh that shares no vertex index with it, and the mesh's clearance.

The definition as it is written, built only from what is pinned elsewhere: EVERY unordered pair of faces, the shared-index filter of
proximity_ref.proximity_pairs, its (ID, face) swap into (A, B), proximity_ref.tri_distance_np on every admissible pair -- no tree, no
box filter of any kind, no bound -- the per-face reduction by (dist, partner ID, partner face), and witness_ref.tri_witness_np on the
winners in the order that was played, whose dist must be the reduced distance bit for bit.  Every function returns
(nearest_ref.NearestRows, played): played u32[n, 2] are the faces that played A and B (NONE twice in a "nothing" row).
"""
from __future__ import annotations

import numpy as np

import nearest_ref as nr
import proximity_ref as pr
import witness_ref as wr

NONE = nr.NONE


def nothing(n):
    return nr.nothing(n), np.full((n, 2), NONE, dtype=np.uint32)


def diameter(verts) -> float:
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0))) if v.shape[0] else 0.0


def admissible_pairs(vidx):
    """(i, j), i < j: every unordered pair of distinct faces with no shared vertex index."""
    vidx = np.asarray(vidx, dtype=np.int64).reshape(-1, 3)
    i, j = np.triu_indices(vidx.shape[0], 1)
    sh = (vidx[i][:, :, None] == vidx[j][:, None, :]).any(axis=(1, 2))
    return i[~sh].astype(np.int64), j[~sh].astype(np.int64)


def played_order(i, j, ids):
    """(a, b) of the pairs (i, j): A is the face with the smaller (ID, face index)."""
    swap = (ids[j] < ids[i]) | ((ids[j] == ids[i]) & (j < i))
    return np.where(swap, j, i), np.where(swap, i, j)


def nearest_rows(verts, vidx, rmax=np.inf, ids=None, chunk=1 << 18):
    """cd_nearest_self, flags = 0: row i for face i."""
    v = np.asarray(verts, dtype=np.float64)
    vidx = np.asarray(vidx, dtype=np.int64).reshape(-1, 3)
    n = vidx.shape[0]
    ids = np.arange(n, dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    tv = v[vidx]
    i, j = admissible_pairs(vidx)
    a, b = played_order(i, j, ids)
    d = np.concatenate([np.zeros(0)] + [pr.tri_distance_np(np.concatenate([tv[a[c:c + chunk]], tv[b[c:c + chunk]]], axis=1))
                                        for c in range(0, a.shape[0], chunk)])
    r = 2.0 * diameter(v) + 1e-300 if np.isinf(rmax) else float(rmax)          # (+inf restated as nearest_ref does)
    ok = d <= r
    a, b, d = a[ok], b[ok], d[ok]
    # every pair is a candidate of both of its faces
    own, partner, dd = np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([d, d])
    pa, pb = np.concatenate([a, a]), np.concatenate([b, b])
    rows, played = nothing(n)
    first = nr._first_per_face(own, dd, ids[partner], partner)
    fo, fp, fa, fb = own[first], partner[first], pa[first], pb[first]
    w = wr.tri_witness_np(np.concatenate([tv[fa], tv[fb]], axis=1).reshape(-1, 6, 3))
    assert np.array_equal(w.dist.view(np.uint64), dd[first].view(np.uint64))
    rows.faces[fo] = np.stack([fo, fp], axis=1)
    rows.ids[fo] = np.stack([ids[fo], ids[fp]], axis=1)
    rows.dist[fo] = dd[first]
    rows.points[fo] = w.points
    rows.bary[fo] = w.bary
    rows.feature[fo] = w.feature
    played[fo] = np.stack([fa, fb], axis=1)
    return rows, played


def within(res, rmax):
    """The rows of a smaller radius from those of a larger one (nearest_ref.within's argument)."""
    rows, played = res
    keep = (rows.faces[:, 0] != NONE) & (rows.dist <= rmax)
    out, op = nothing(rows.dist.shape[0])
    for dst, src in zip(out, rows):
        dst[keep] = src[keep]
    op[keep] = played[keep]
    return out, op


def nearest_min(res):
    """CD_NEAREST_MIN: the one row with the smallest (dist, own ID, own face, partner ID, partner face), or the "nothing" row."""
    rows, played = res
    found = np.nonzero(rows.faces[:, 0] != NONE)[0]
    if found.size == 0:
        return nothing(1)
    o = np.lexsort((rows.faces[found, 1], rows.ids[found, 1], rows.faces[found, 0], rows.ids[found, 0], rows.dist[found]))
    w = found[o[:1]]
    return nr.NearestRows(*(x[w].copy() for x in rows)), played[w].copy()


def reduce_pairs(n, faces, pairs, dists, points, bary, feature):
    """Rows of a proximity witness call -- faces u32[m, 2] (played A, B), pairs (their IDs), dists, the witness -- reduced per face by
    (dist, partner ID, partner face): every row is a candidate of both of its faces."""
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 2)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    m = faces.shape[0]
    own, partner = np.concatenate([faces[:, 0], faces[:, 1]]), np.concatenate([faces[:, 1], faces[:, 0]])
    oid, pid = np.concatenate([pairs[:, 0], pairs[:, 1]]), np.concatenate([pairs[:, 1], pairs[:, 0]])
    src = np.concatenate([np.arange(m), np.arange(m)])
    first = nr._first_per_face(own, np.concatenate([dists, dists]), pid, partner)
    rows, played = nothing(n)
    fo, k = own[first], src[first]
    rows.faces[fo] = np.stack([fo, partner[first]], axis=1)
    rows.ids[fo] = np.stack([oid[first], pid[first]], axis=1)
    rows.dist[fo] = np.asarray(dists)[k]
    rows.points[fo] = np.asarray(points)[k]
    rows.bary[fo] = np.asarray(bary)[k]
    rows.feature[fo] = np.asarray(feature)[k]
    played[fo] = faces[k]
    return rows, played


def fan(k=40):
    """k triangles around one vertex: every pair shares vertex 0, so there is no admissible pair."""
    t = np.linspace(0.0, 2.0 * np.pi, k + 1)[:-1]
    rim = np.stack([np.cos(t), np.sin(t), 0.1 * np.cos(3 * t)], axis=1)
    verts = np.concatenate([np.zeros((1, 3)), rim])
    vidx = np.stack([np.zeros(k, dtype=np.int64), 1 + np.arange(k), 1 + (np.arange(k) + 1) % k], axis=1).astype(np.uint32)
    return verts, vidx


def fan_and_far(k=40):
    """The fan plus one private triangle far away: the only admissible partner of every fan triangle, and no near seed for it."""
    verts, vidx = fan(k)
    far = np.array([[50.0, 50.0, 50.0], [51.0, 50.0, 50.0], [50.0, 51.0, 50.5]])
    n = verts.shape[0]
    return np.concatenate([verts, far]), np.concatenate([vidx, np.array([[n, n + 1, n + 2]], dtype=np.uint32)])
