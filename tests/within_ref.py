"""The all-results item queries restated on the CPU (no test in here): cd_points_within and cd_cast_rays_all as ALL pairs of items and
triangles -- no box filter of any kind -- from the predicates of tests/point_ref.py and tests/ray_ref.py, which are pt_tri and ray_tri
bit for bit; the per-item minimum of a row set in the form the single-answer references return; and the items the CPU and GPU tests
share.

A row set is sorted by (item, face), the order the comparisons use (the device's order is free)."""
from __future__ import annotations

import collections
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import point_ref as ptr
import query_meshes as qm
import ray_ref as rr

NONE = np.uint32(0xFFFFFFFF)

PointRows = collections.namedtuple("PointRows", "rows ids dist closest uv feature side")
RayRows = collections.namedtuple("RayRows", "rows ids t uv side")


def _chunks(work, n, step, threads):
    starts = list(range(0, n, step))
    if threads > 1 and len(starts) > 1:
        with ThreadPoolExecutor(threads) as ex:
            return list(ex.map(work, starts))
    return [work(a) for a in starts]


def _mesh(verts, vidx, ids):
    verts = np.asarray(verts, dtype=np.float64)
    vidx = np.asarray(vidx)
    ids = np.arange(vidx.shape[0], dtype=np.uint32) if ids is None else np.asarray(ids, dtype=np.uint32)
    return verts[vidx.astype(np.int64)], ids                                    # [T, 3, 3]


def _pairs(parts):
    k = np.concatenate([p[0] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
    f = np.concatenate([p[1] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
    return k.astype(np.int64), f.astype(np.int64)                               # (chunks in order, np.nonzero row-major: sorted by (item, face))


def points_within_ref(verts, vidx, ids, points, rmax, pairs_per_chunk=1 << 20, threads=8) -> PointRows:
    """Every point against ALL triangles (chunks of points): a row wherever pt_tri's dist <= rmax, with pt_tri's values."""
    p, ids = _mesh(verts, vidx, ids)
    nt = p.shape[0]
    pt = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = pt.shape[0]
    rm = np.broadcast_to(np.asarray(rmax, dtype=np.float64), (n,))
    T0, T1, T2 = (tuple(np.ascontiguousarray(p[:, j, k])[None, :] for k in range(3)) for j in range(3))
    step = max(1, pairs_per_chunk // max(nt, 1))

    def work(a):
        b = min(n, a + step)
        with np.errstate(all="ignore"):
            d = ptr._core(tuple(pt[a:b, k][:, None] for k in range(3)), T0, T1, T2, False)     # [b - a, T]
        ri, ti = np.nonzero(d <= rm[a:b, None])
        return a + ri, ti

    k, f = _pairs(_chunks(work, n, step, threads))
    dist, q, u, v, feat, side = ptr.pt_tri_np(pt[k], p[f])                      # the rows again, with everything (the same bits)
    assert (dist <= rm[k]).all()
    return PointRows(np.stack([k, f], axis=1).astype(np.uint32), ids[f], dist, q, np.stack([u, v], axis=1), feat, side)


def cast_rays_all_ref(verts, vidx, ids, rays, pairs_per_chunk=1 << 22, threads=8) -> RayRows:
    """Every ray against ALL triangles (chunks of rays; only ray_tri's own first exit, the u test, thins the pairs out before ray_tri_np
    evaluates them): a row wherever ray_tri hits, with ray_tri's values."""
    p, ids = _mesh(verts, vidx, ids)
    nt = p.shape[0]
    r = np.asarray(rays, dtype=np.float64).reshape(-1, 7)
    n = r.shape[0]
    p0 = np.ascontiguousarray(p[:, 0])
    e1, e2 = p[:, 1] - p0, p[:, 2] - p0
    step = max(1, pairs_per_chunk // max(nt, 1))

    def work(a):
        b = min(n, a + step)
        with np.errstate(all="ignore"):
            ok = rr._stage_u(r[a:b, None, 0:3], r[a:b, None, 3:6], p0[None], e1[None], e2[None])[0]
        ri, ti = np.nonzero(ok)
        hit = rr.ray_tri_np(r[a + ri], p[ti])[0]
        return a + ri[hit], ti[hit]

    k, f = _pairs(_chunks(work, n, step, threads))
    hit, t, u, v, side = rr.ray_tri_np(r[k], p[f])
    assert hit.all()
    return RayRows(np.stack([k, f], axis=1).astype(np.uint32), ids[f], t, np.stack([u, v], axis=1), side)


def sort_rows(rows, *vals):
    """A call's rows and their value arrays sorted by (item, face): the order of the restatement."""
    rows = np.asarray(rows).reshape(-1, 2)
    o = np.lexsort((rows[:, 1], rows[:, 0]))
    return (rows[o],) + tuple(np.asarray(v)[o] for v in vals)


def per_item(w):
    """Rows per item as the key of the smallest: the indices, into w's arrays, of each item's first row by (dist or t, ID, face), and
    those items.  (-0.0 == 0.0, as the device's comparisons have it.)"""
    o = np.lexsort((w.rows[:, 1], w.ids, w[2], w.rows[:, 0]))
    items, first = np.unique(w.rows[o, 0], return_index=True)
    return o[first], items.astype(np.int64)


def closest_of(w: PointRows, n):
    """The per-point minimum of a row set as closest_points_ref returns it: (face, ids, dist, closest, uv, feature, side)."""
    at, k = per_item(w)
    face = np.full(n, NONE, dtype=np.uint32); oid = np.zeros(n, dtype=np.uint32); dist = np.full(n, np.inf)
    q = np.zeros((n, 3)); uv = np.zeros((n, 2)); feat = np.zeros(n, dtype=np.uint8); side = np.zeros(n, dtype=np.uint8)
    face[k] = w.rows[at, 1]; oid[k] = w.ids[at]; dist[k] = w.dist[at]; q[k] = w.closest[at]; uv[k] = w.uv[at]; feat[k] = w.feature[at]; side[k] = w.side[at]
    return face, oid, dist, q, uv, feat, side


def first_hit_of(w: RayRows, n):
    """The per-ray minimum of a row set as cast_rays_ref returns it: (face, ids, t, uv, side)."""
    at, k = per_item(w)
    face = np.full(n, NONE, dtype=np.uint32); oid = np.zeros(n, dtype=np.uint32); t = np.full(n, np.inf)
    uv = np.zeros((n, 2)); side = np.zeros(n, dtype=np.uint8)
    face[k] = w.rows[at, 1]; oid[k] = w.ids[at]; t[k] = w.t[at]; uv[k] = w.uv[at]; side[k] = w.side[at]
    return face, oid, t, uv, side


def rows_per_item(w, n):
    return np.bincount(w.rows[:, 0].astype(np.int64), minlength=n)


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def same_rows(got, want, what=""):
    """got: a call's (rows, values ...) in any order; want: a PointRows / RayRows.  The same set of (item, face), and after sorting both
    by (item, face) every value bit for bit."""
    g = sort_rows(*got[:len(want)])
    assert g[0].shape == want.rows.shape and np.array_equal(g[0], want.rows), (what, g[0].shape, want.rows.shape)
    for name, a, b in zip(want._fields[1:], g[1:], want[1:]):
        if b.dtype == np.float64:
            a, b = _bits(a), _bits(b)
        bad = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
        assert bad.size == 0, (what, name, bad.size, g[0][bad[:4]])


# ---------------------------------------------------------------- the items of the tests
MESHES = {m[0]: m[1:] for m in qm._meshes()}
SMALL = [name for name, m in MESHES.items() if m[1].shape[0] <= 10_000]
SEED = 5


def n_items(name):
    return 256 if name == "cloth100" else 1000                                 # (1000: not a multiple of 64)


@functools.lru_cache(maxsize=None)
def points(name, n=None):
    v, i, ids, edge = MESHES[name]
    return ptr.mesh_points(v, i, n or n_items(name), seed=SEED, edge=edge)


@functools.lru_cache(maxsize=None)
def rays(name, n=None):
    v, i, ids, edge = MESHES[name]
    return rr.mesh_rays(v, i, n or n_items(name), seed=SEED)


@functools.lru_cache(maxsize=None)
def want_points(name, factor, n=None):
    """The rows of points(name, n) with rmax = factor * the mesh's edge."""
    v, i, ids, edge = MESHES[name]
    return points_within_ref(v, i, ids, points(name, n), factor * edge)


@functools.lru_cache(maxsize=None)
def want_rays(name, n=None):
    v, i, ids, edge = MESHES[name]
    return cast_rays_all_ref(v, i, ids, rays(name, n))


def input_conditions(name):
    """What the test of the row sets needs of its items, per mesh: items with no row and items with several rows, in numbers.
    On every mesh of at least 2 triangles: at least n / 8 items of EVERY item set (points at radius edge, at 3 edge, rays) have no row;
    at least n / 64 points at radius 3 edge have two or more rows; and of the mesh's 3 n items taken together at least 3 n / 8 have none
    and 3 n / 64 two or more.  The several-rows count cannot hold for every set on its own: n3 is three scattered triangles, where no
    point is within one edge of two of them (0 of 1000) and no ray of mesh_rays crosses two (0 of 1000; n2: 4 of 1000).  Figures with
    seed 5, n = 1000 (cloth100: 256), the smallest over the meshes: no row 279 (edge), 191 (3 edge), 385 (rays), cloth100 94, 84, 40;
    two or more rows at 3 edge 415, cloth100 172.  n1 has at most one row an item, and items with none and with one."""
    n, nt = n_items(name), MESHES[name][1].shape[0]
    counts = [rows_per_item(w, n) for w in (want_points(name, 1.0), want_points(name, 3.0), want_rays(name))]
    print(name, [(int((c == 0).sum()), int((c >= 2).sum()), int(c.max())) for c in counts])
    if nt == 1:
        assert all(c.max() <= 1 and (c == 0).any() and (c == 1).any() for c in counts)
        return
    assert all((c == 0).sum() >= n // 8 for c in counts)
    assert (counts[1] >= 2).sum() >= n // 64
    assert sum((c == 0).sum() for c in counts) >= 3 * n // 8 and sum((c >= 2).sum() for c in counts) >= 3 * n // 64
