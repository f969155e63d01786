"""The box queries restated on the CPU (no test in here): box_tri (csrc/cd_math.h) in numpy with the same operation order, bit for
bit in hit, inside and code; cd_boxes_overlap_all and cd_boxes_count as ALL pairs of boxes and triangles -- no box filter of any kind:
only box_tri's own first step, the gate, thins the pairs out before the rest of it is evaluated -- and the items the CPU and GPU
tests share.

A box is six doubles {x1, x2, y1, y2, z1, z2}, closed.  A row set is sorted by (item, face), the order the comparisons use (the
device's order is free)."""
from __future__ import annotations

import collections
import functools

import numpy as np

import within_ref as wr

BoxRows = collections.namedtuple("BoxRows", "rows ids inside")


# ---------------------------------------------------------------- the predicate
def _core(b, P):
    """box_tri on broadcastable operands.  b: (x1, x2, y1, y2, z1, z2); P: three vertices, each (x, y, z).  -> hit, inside, code.
    Every test is evaluated and the first that separates, in box_tri's order, gives the code; rules 2 and 2b (a vertex in the box) end the
    evaluation."""
    lo, hi = (b[0], b[2], b[4]), (b[1], b[3], b[5])
    p0, p1, p2 = P
    with np.errstate(all="ignore"):
        shape = np.broadcast(b[0], p0[0]).shape
        code = np.zeros(shape, dtype=np.uint8)

        def first(sep, c):
            np.copyto(code, np.uint8(c), where=sep & (code == 0))

        for a in range(3):                                                   # 1: the gate
            below = (p0[a] < lo[a]) & (p1[a] < lo[a]) & (p2[a] < lo[a])
            above = (p0[a] > hi[a]) & (p1[a] > hi[a]) & (p2[a] > hi[a])
            first(below | above, 1 + a)
        inside = np.ones(shape, dtype=bool)                                  # 2: all three vertices in the closed box
        for p in P:
            for a in range(3):
                inside = inside & (lo[a] <= p[a]) & (p[a] <= hi[a])
        inside &= code == 0
        some = np.zeros(shape, dtype=bool)                                   # 2b: any vertex in the closed box: a hit, nothing further
        for p in P:
            some = some | ((lo[0] <= p[0]) & (p[0] <= hi[0]) & (lo[1] <= p[1]) & (p[1] <= hi[1]) & (lo[2] <= p[2]) & (p[2] <= hi[2]))
        c = tuple(0.5 * lo[a] + 0.5 * hi[a] for a in range(3))               # 3: the nine edge axes
        h = tuple(0.5 * hi[a] - 0.5 * lo[a] for a in range(3))
        v = tuple(tuple(p[a] - c[a] for a in range(3)) for p in P)
        f = (tuple(p1[a] - p0[a] for a in range(3)), tuple(p2[a] - p1[a] for a in range(3)), tuple(p0[a] - p2[a] for a in range(3)))
        for k in range(3):
            for j in range(3):
                a, bb = (j + 1) % 3, (j + 2) % 3
                q = [v[i][bb] * f[k][a] - v[i][a] * f[k][bb] for i in range(3)]
                r = h[a] * np.abs(f[k][bb]) + h[bb] * np.abs(f[k][a])
                sep = ((q[0] > r) & (q[1] > r) & (q[2] > r)) | ((q[0] < -r) & (q[1] < -r) & (q[2] < -r))
                first(sep & ~some, 4 + 3 * k + j)
        n = (f[0][1] * f[1][2] - f[0][2] * f[1][1], f[0][2] * f[1][0] - f[0][0] * f[1][2], f[0][0] * f[1][1] - f[0][1] * f[1][0])   # 4: the plane
        d = (n[0] * v[0][0] + n[1] * v[0][1]) + n[2] * v[0][2]
        r = (h[0] * np.abs(n[0]) + h[1] * np.abs(n[1])) + h[2] * np.abs(n[2])
        first(((d > r) | (d < -r)) & ~some, 13)
    return code == 0, inside, code


def box_tri_np(boxes, tris):
    """boxes [n, 6], tris [n, 3, 3] -> hit[n] (bool), inside[n] (bool), code[n] (uint8)."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    return _core(tuple(b[:, k] for k in range(6)), tuple(tuple(t[:, i, a] for a in range(3)) for i in range(3)))


# ---------------------------------------------------------------- the families of single pairs (tests/test_box_ref.py checks them against exact arithmetic)
N = 20_000


@functools.lru_cache(maxsize=None)
def integer_family(n=N, seed=1):
    """Vertices in {-5 .. 5}^3, integer box bounds with widths 0 .. 3: every operation of box_tri is exact (halves of integers
    included).  Touching vertices, edges through box edges and triangles in a box face all occur."""
    g = np.random.default_rng(seed)
    tris = g.integers(-5, 6, (n, 3, 3)).astype(np.float64)
    lo = g.integers(-5, 4, (n, 3))
    hi = lo + g.integers(0, 4, (n, 3))
    boxes = np.stack([lo, hi], axis=2).reshape(n, 6).astype(np.float64)
    return boxes, tris


@functools.lru_cache(maxsize=None)
def random_family(offset=0.0, n=N, seed=2):
    """Boxes (two corners, sorted per axis) and triangles (a vertex and two more within 0.6 of it) uniform in the unit cube, moved by
    `offset`: 0, or 2^20 + 0.37, where the arithmetic works on the low bits of every coordinate."""
    g = np.random.default_rng(seed)
    c = np.sort(g.random((n, 3, 2)), axis=2)
    p0 = g.random((n, 1, 3))
    tris = np.concatenate([p0, np.clip(p0 + 0.6 * (g.random((n, 2, 3)) - 0.5), 0.0, 1.0)], axis=1)
    return np.ascontiguousarray(c.reshape(n, 6) + offset), np.ascontiguousarray(tris + offset)


OFFSET = 2.0 ** 20 + 0.37


def near_touching_family(n=100_000, seed=3):
    """Triangles with a vertex, an edge point or an interior point ON a face, an edge or a corner of the box or within a few ulps of
    it: the unit-cube family's boxes, and triangles whose first vertex is such a point with the other two anywhere."""
    g = np.random.default_rng(seed)
    c = np.sort(g.random((n, 3, 2)), axis=2)
    on = g.random((n, 3))
    pick = g.integers(0, 3, (n, 3))                                              # per axis: lo, hi, or anywhere in between
    q = np.where(pick == 0, c[:, :, 0], np.where(pick == 1, c[:, :, 1], c[:, :, 0] + on * (c[:, :, 1] - c[:, :, 0])))
    ulps = g.integers(-2, 3, (n, 3))
    q = np.where(ulps < 0, np.nextafter(q, -np.inf), np.where(ulps > 0, np.nextafter(q, np.inf), q))
    rest = g.random((n, 2, 3))
    w = g.random((n, 1, 1))
    kind = g.integers(0, 3, n)[:, None, None]
    # kind 0: q is the first vertex; 1: q lies on the first edge (up to rounding); 2: as 0 with both others outside on one side
    p0 = np.where(kind == 1, q[:, None, :] + w * (q[:, None, :] - rest[:, :1]), q[:, None, :])
    tris = np.concatenate([p0, rest], axis=1)
    return np.ascontiguousarray(c.reshape(n, 6)), np.ascontiguousarray(tris)


# ---------------------------------------------------------------- the two calls, all pairs
def boxes_overlap_all_ref(verts, vidx, ids, boxes, pairs_per_chunk=1 << 21, threads=8) -> BoxRows:
    """Every box against ALL triangles (chunks of boxes): a row wherever box_tri hits, with its inside."""
    p, ids = wr._mesh(verts, vidx, ids)
    nt = p.shape[0]
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    n = b.shape[0]
    tmin, tmax = p.min(axis=1), p.max(axis=1)                                # (max < lo: all three below; exact comparisons either way)
    step = max(1, pairs_per_chunk // max(nt, 1))

    def work(a):
        e = min(n, a + step)
        gate = np.ones((e - a, nt), dtype=bool)
        for ax in range(3):
            gate &= ~((tmax[None, :, ax] < b[a:e, None, 2 * ax]) | (tmin[None, :, ax] > b[a:e, None, 2 * ax + 1]))
        ri, ti = np.nonzero(gate)
        hit = box_tri_np(b[a + ri], p[ti])[0]
        return a + ri[hit], ti[hit]

    k, f = wr._pairs(wr._chunks(work, n, step, threads))
    hit, inside, code = box_tri_np(b[k], p[f])                               # the rows again (the same bits)
    assert hit.all()
    return BoxRows(np.stack([k, f], axis=1).astype(np.uint32).reshape(-1, 2), ids[f], inside)


def boxes_count_ref(verts, vidx, boxes, pairs_per_chunk=1 << 19):
    """Every box against ALL triangles with the whole predicate on every pair (not even the gate thins them out): count, n_inside."""
    p, _ = wr._mesh(verts, vidx, None)
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    n, nt = b.shape[0], p.shape[0]
    count, n_inside = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    P = tuple(tuple(np.ascontiguousarray(p[:, i, a])[None, :] for a in range(3)) for i in range(3))
    step = max(1, pairs_per_chunk // max(nt, 1))
    for a in range(0, n, step):
        e = min(n, a + step)
        hit, inside, _ = _core(tuple(b[a:e, k][:, None] for k in range(6)), P)
        count[a:e] = hit.sum(axis=1)
        n_inside[a:e] = inside.sum(axis=1)
    return count, n_inside


def counts_of(w: BoxRows, n):
    """count, n_inside per item of a row set."""
    k = w.rows[:, 0].astype(np.int64)
    return np.bincount(k, minlength=n).astype(np.uint32), np.bincount(k[np.asarray(w.inside, dtype=bool)], minlength=n).astype(np.uint32)


def take_items(w: BoxRows, m):
    """The rows of the first m items."""
    keep = w.rows[:, 0] < m
    return BoxRows(w.rows[keep], w.ids[keep], w.inside[keep])


def same_rows(got, want: BoxRows, what=""):
    wr.same_rows((got[0], got[1], np.asarray(got[2], dtype=bool)), want, what)


# ---------------------------------------------------------------- the items of the tests
MESHES = wr.MESHES
NAMES = ["n1", "n2", "n3", "n63", "n64", "n65", "duplicates", "custom_ids", "comb", "soup10k", "cloth100"]
COUNTS = (1, 63, 64, 65, 1000)
SEED = 23
KINDS = ("half", "one", "three", "point", "slab", "miss", "off", "half")     # item i is of kind KINDS[i % 8]; item ROOT_AT is the root box
ROOT_AT = 7


def root_box(verts, vidx):
    """The FP64 box of every triangle of the mesh: what cd_root_box returns."""
    p = np.asarray(verts, dtype=np.float64)[np.asarray(vidx).astype(np.int64)].reshape(-1, 3)
    return np.stack([p.min(axis=0), p.max(axis=0)], axis=1).reshape(6)


def make_boxes(verts, vidx, edge, n, seed=SEED):
    """n boxes [n, 6] for a mesh: by index modulo 8 a box centred on a mesh vertex with half-width 0.5, 1 or 3 edges; a POINT box on
    a vertex; a SLAB (lo == hi in y, one edge either way in x and z: in the plane of a cloth sheet, which spans x and z) through a
    vertex; a box that MISSES the mesh (beyond its root box); a box of half-width 1 edge centred half an edge off a vertex; and at
    index ROOT_AT the mesh's root box.  (The first item is of kind `half`, so one item alone is an ordinary box.)"""
    v = np.asarray(verts, dtype=np.float64)
    used = v[np.asarray(vidx).astype(np.int64)].reshape(-1, 3)
    g = np.random.default_rng(seed)
    c = used[g.integers(0, used.shape[0], n)]
    root = root_box(verts, vidx)
    extent = root[1::2] - root[0::2]
    out = np.empty((n, 6))
    for i in range(n):
        kind = KINDS[i % 8]
        if kind == "point":
            lo = hi = c[i]
        elif kind == "slab":
            hw = np.array([edge, 0.0, edge])
            lo, hi = c[i] - hw, c[i] + hw
        elif kind == "miss":
            far = c[i] + extent + 10.0 * edge
            lo, hi = far - edge, far + edge
        elif kind == "off":
            m = c[i] + 0.5 * edge * g.uniform(-1.0, 1.0, 3)
            lo, hi = m - edge, m + edge
        else:
            hw = {"half": 0.5, "one": 1.0, "three": 3.0}[kind] * edge
            lo, hi = c[i] - hw, c[i] + hw
        out[i, 0::2], out[i, 1::2] = lo, hi
    if n > ROOT_AT:
        out[ROOT_AT] = root
    return np.ascontiguousarray(out)


@functools.lru_cache(maxsize=None)
def boxes(name, n=1000):
    v, i, ids, edge = MESHES[name]
    return make_boxes(v, i, edge, n)


@functools.lru_cache(maxsize=None)
def want_rows(name, n=1000):
    v, i, ids, edge = MESHES[name]
    return boxes_overlap_all_ref(v, i, ids, boxes(name, n))


def input_conditions(name):
    """What the GPU test needs of its items, per mesh: items with no row (the miss boxes at least: n / 8), items with several rows,
    rows with inside = 0 and rows with inside = 1 (the root box's at least).  On the meshes of one to three triangles an item set
    holds what it can: n1 has at most one row an item, so no item with several; n2 and n3 are scattered triangles an edge long, where
    only the root box and the boxes of three edges can meet two.  Every mesh has rows of both inside values: a point box on a
    vertex of a non-degenerate triangle gives inside = 0, the root box inside = 1."""
    n, nt = 1000, MESHES[name][1].shape[0]
    w = want_rows(name)
    c, ci = counts_of(w, n)
    print(name, "items without a row", int((c == 0).sum()), "with several", int((c >= 2).sum()), "rows", w.rows.shape[0], "inside", int(w.inside.sum()))
    assert (c == 0).sum() >= n // 8 and c[ROOT_AT] == nt == ci[ROOT_AT]
    assert w.inside.any() and not w.inside.all()
    if nt == 1:
        assert c.max() == 1
    elif nt <= 3:
        assert (c >= 2).sum() >= 1
    else:
        assert (c >= 2).sum() >= n // 8
