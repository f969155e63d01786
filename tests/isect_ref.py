"""The contour of the contact queries restated on the CPU (no test in here): tri_isect in numpy, built on ray_ref.ray_tri_np and so bit
for bit what csrc/cd_math.h evaluates; the rows of cd_find_collisions_contour and cd_find_collisions_between_contour enumerated by
face pair without any tree; and the operand sets the CPU and GPU tests share.

tri_isect(A, B) (include/mi355cd.h): six terms, k = 0, 1, 2 A's edge (A_k, A_(k+1 mod 3)) against B's face,
k = 3, 4, 5 B's edge (B_(k-3), B_(k-2 mod 3)) against A's face, each ray_tri(o = start, d = end - start, tmax = 1; face) with
x_k = o + t d (product rounded, then the sum).  mask = the terms that hit.  No hit: n = 0.  One: endpoint 0.  Two or more: the pair
(i, j), i < j, of hit terms with the largest D = (dx dx + dy dy) + dz dz of x_i - x_j, pairs taken in lexicographic order, a later
pair replacing the kept one only when its D is strictly larger.
"""
from __future__ import annotations

import collections

import numpy as np

import between_ref as br
import oracle
import point_ref
import proximity_ref as pr
import ray_ref

TERM_NONE = 7

Isect = collections.namedtuple("Isect", "n code param points hit t u v side x")
Isect.__doc__ = """tri_isect of m pairs: n u8[m] (0, 1, 2 endpoints), code u8[m, 3] (endpoint 0 and 1 as term | side << 3, 7 = missing; the
mask), param f64[m, 2, 3] (t, u, v of the two endpoints), points f64[m, 2, 3]; and the six terms themselves: hit bool[m, 6], t, u, v
f64[m, 6], side u8[m, 6], x f64[m, 6, 3] (zeros on a miss)."""

Rows = collections.namedtuple("Rows", "faces pairs code param points tested")
Rows.__doc__ = """The rows of a contour call sorted by (face_a, face_b): faces u32[n, 2], pairs u32[n, 2] (the IDs), code u8[n, 3],
param f64[n, 6], points f64[n, 6]; tested = the pairs that reach tri_contact."""


def terms_of(tri):
    """The six (ray, face) operand pairs of every pair: rays f64[m, 6, 7] (o, d = end - start, 1.0), faces f64[m, 6, 3, 3]."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 6, 3)
    m = t.shape[0]
    rays = np.empty((m, 6, 7))
    faces = np.empty((m, 6, 3, 3))
    for k in range(6):
        own, other = (t[:, :3], t[:, 3:]) if k < 3 else (t[:, 3:], t[:, :3])
        o, e = own[:, k % 3], own[:, (k + 1) % 3]
        with np.errstate(all="ignore"):
            rays[:, k, 0:3] = o; rays[:, k, 3:6] = e - o; rays[:, k, 6] = 1.0
        faces[:, k] = other
    return rays, faces


def tri_isect_np(tri) -> Isect:
    """tri: f64[m, 6, 3] (A's vertices, then B's)."""
    rays, faces = terms_of(tri)
    m = rays.shape[0]
    hit, t, u, v, side = ray_ref.ray_tri_np(rays.reshape(-1, 7), faces.reshape(-1, 3, 3))
    hit, t, u, v, side = (a.reshape(m, 6) for a in (hit, t, u, v, side))
    with np.errstate(all="ignore"):
        x = rays[:, :, 0:3] + t[:, :, None] * rays[:, :, 3:6]
    x = np.where(hit[:, :, None], x, 0.0)
    have = np.zeros(m, dtype=bool)
    best = np.zeros(m)
    e0 = np.full(m, TERM_NONE, dtype=np.int64)
    e1 = np.full(m, TERM_NONE, dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(6):
            for j in range(i + 1, 6):
                both = hit[:, i] & hit[:, j]
                d = x[:, i] - x[:, j]
                D = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                take = both & (~have | (D > best))
                best = np.where(take, D, best)
                e0 = np.where(take, i, e0); e1 = np.where(take, j, e1)
                have |= both
    nh = hit.sum(axis=1)
    one = nh == 1
    e0 = np.where(one, np.argmax(hit, axis=1), e0)
    n = np.minimum(nh, 2).astype(np.uint8)
    mask = (hit.astype(np.uint8) << np.arange(6, dtype=np.uint8)[None, :]).sum(axis=1).astype(np.uint8)
    code = np.empty((m, 3), dtype=np.uint8)
    param = np.zeros((m, 2, 3))
    points = np.zeros((m, 2, 3))
    r = np.arange(m)
    for s, e in enumerate((e0, e1)):
        ok = e != TERM_NONE
        k = np.where(ok, e, 0)
        code[:, s] = np.where(ok, e | (side[r, k].astype(np.int64) << 3), TERM_NONE).astype(np.uint8)
        param[:, s, 0] = np.where(ok, t[r, k], 0.0); param[:, s, 1] = np.where(ok, u[r, k], 0.0); param[:, s, 2] = np.where(ok, v[r, k], 0.0)
        points[:, s] = np.where(ok[:, None], x[r, k], 0.0)
    code[:, 2] = mask
    return Isect(n, code, param, points, hit, t, u, v, side.astype(np.uint8), x)


def endpoint_error(tri, isect) -> np.ndarray:
    """f64[m]: the largest distance of a returned endpoint from either of the two triangles (point_ref.pt_tri_np, whose own error is
    around 2^-50 M), divided by the pair's largest |coordinate| M; 0 for a pair without endpoints."""
    t = np.ascontiguousarray(tri, dtype=np.float64).reshape(-1, 6, 3)
    M = np.abs(t).max(axis=(1, 2))
    worst = np.zeros(t.shape[0])
    for s in range(2):
        ok = (isect.code[:, s] & 7) != TERM_NONE
        for tr in (t[:, :3], t[:, 3:]):
            d = point_ref.pt_tri_np(isect.points[:, s], tr)[0]
            worst = np.maximum(worst, np.where(ok, d, 0.0))
    with np.errstate(all="ignore"):
        return np.where(M > 0, worst / np.where(M > 0, M, 1.0), 0.0)


# ---------------------------------------------------------------- the queries
def _rows(fa, fb, ida, idb, tri, tested) -> Rows:
    w = tri_isect_np(tri)
    o = np.lexsort((fb, fa))
    faces = np.stack([fa, fb], axis=1).astype(np.uint32)[o]
    pairs = np.stack([ida, idb], axis=1).astype(np.uint32)[o]
    return Rows(faces, pairs, w.code[o], w.param.reshape(-1, 6)[o], w.points.reshape(-1, 6)[o], tested)


def contour_pairs(verts, vidx, ids=None, chunk=1 << 18, brute=None) -> Rows:
    """cd_find_collisions_contour: every unordered pair of faces with no shared vertex index, different IDs, strictly overlapping FP64
    boxes (these reach tri_contact: `tested`) and tri_contact with the smaller ID's triangle as P; A = the smaller ID."""
    verts = np.asarray(verts, dtype=np.float64)
    vidx = np.asarray(vidx, dtype=np.int64).reshape(-1, 3)
    n = vidx.shape[0]
    ids = br._ids(ids, n)
    tv = verts[vidx]
    lo, hi = tv.min(axis=1), tv.max(axis=1)
    if brute is None:
        brute = n <= pr.BRUTE_MAX
    if brute:
        i, j = np.triu_indices(n, 1)
        cand = np.stack([i, j], axis=1).astype(np.int64)
    else:
        w = br._pad((tv,), 0.0)
        cand = pr._candidates(lo - w, hi + w)
    fa, fb, tested = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0
    for c0 in range(0, cand.shape[0], chunk):
        i, j = cand[c0:c0 + chunk, 0], cand[c0:c0 + chunk, 1]
        keep = ~(vidx[i][:, :, None] == vidx[j][:, None, :]).any(axis=(1, 2)) & (ids[i] != ids[j])
        i, j = i[keep], j[keep]
        ov = br.strict_overlap(tv[i], tv[j])
        i, j = i[ov], j[ov]
        tested += int(i.shape[0])
        if not i.shape[0]:
            continue
        swap = ids[j] < ids[i]
        a, b = np.where(swap, j, i), np.where(swap, i, j)
        hit = oracle.tri_contact_points(np.concatenate([tv[a], tv[b]], axis=1).reshape(-1, 18)) != 0
        fa.append(a[hit]); fb.append(b[hit])
    fa, fb = np.concatenate(fa), np.concatenate(fb)
    return _rows(fa, fb, ids[fa], ids[fb], np.concatenate([tv[fa], tv[fb]], axis=1).reshape(-1, 6, 3), tested)


def contour_pairs_between(va, ia, vb, ib, ids_a=None, ids_b=None, chunk=1 << 18, brute=None) -> Rows:
    """cd_find_collisions_between_contour: between_ref.contact_pairs' definition by face pair; A = a's triangle."""
    va, vb = np.asarray(va, dtype=np.float64), np.asarray(vb, dtype=np.float64)
    ia, ib = np.asarray(ia, dtype=np.int64).reshape(-1, 3), np.asarray(ib, dtype=np.int64).reshape(-1, 3)
    ida, idb = br._ids(ids_a, ia.shape[0]), br._ids(ids_b, ib.shape[0])
    ta, tb = va[ia], vb[ib]
    w = br._pad((ta, tb), 0.0)
    ci, cj = br._cross_candidates(ta.min(axis=1) - w, ta.max(axis=1) + w, tb.min(axis=1) - w, tb.max(axis=1) + w, brute)
    fa, fb, tested = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0
    for c0 in range(0, ci.shape[0], chunk):
        i, j = ci[c0:c0 + chunk], cj[c0:c0 + chunk]
        ov = br.strict_overlap(ta[i], tb[j])
        i, j = i[ov], j[ov]
        tested += int(i.shape[0])
        if not i.shape[0]:
            continue
        hit = oracle.tri_contact_points(np.concatenate([ta[i], tb[j]], axis=1).reshape(-1, 18)) != 0
        fa.append(i[hit]); fb.append(j[hit])
    fa, fb = np.concatenate(fa), np.concatenate(fb)
    return _rows(fa, fb, ida[fa], idb[fb], np.concatenate([ta[fa], tb[fb]], axis=1).reshape(-1, 6, 3), tested)


def sort_got(faces, *arrays):
    """A call's rows in the restatement's order: sorted by (face_a, face_b)."""
    f = np.asarray(faces).reshape(-1, 2)
    o = np.lexsort((f[:, 1], f[:, 0]))
    return (f[o],) + tuple(np.asarray(a)[o] for a in arrays)


# ---------------------------------------------------------------- inputs shared by the CPU and GPU tests
GENERIC = ("unit", "small", "offset")        # sets on which every pair in contact has exactly two hits
OFFSET = 2.0 ** 20 + 0.37


def pin_sets(n, seed=7):
    """name -> f64[n, 6, 3]: random unit pairs, pairs of diameter 0.2, the same offset by 2^20 + 0.37, integer-grid pairs with
    coordinates 0..4, slivers, degenerate triangles, pairs not in contact."""
    g = np.random.default_rng(seed)
    out = {}
    out["unit"] = g.random((n, 6, 3))
    s = g.random((n, 1, 3)) * 0.8 + g.random((n, 6, 3)) * (0.2 / np.sqrt(3.0))
    out["small"] = s
    out["offset"] = s + OFFSET
    out["grid"] = g.integers(0, 5, (n, 6, 3)).astype(np.float64)
    sl = g.random((n, 6, 3))
    sl[:, 2] = sl[:, 0] + g.uniform(-0.5, 1.5, (n, 1)) * (sl[:, 1] - sl[:, 0]) + g.normal(size=(n, 3)) * 1e-9
    c = sl[:, 0] + g.random((n, 1)) * (sl[:, 1] - sl[:, 0])                   # B runs through a point of the sliver's long edge
    sl[:, 3:] = c[:, None, :] + g.normal(size=(n, 3, 3)) * 0.3
    out["sliver"] = sl
    dv, _ = br.with_degenerate(out["unit"].reshape(-1, 3), np.zeros((0, 3), np.uint32), seed + 1)
    out["degenerate"] = dv.reshape(n, 6, 3)
    a = g.random((n, 6, 3))
    on = g.random((n, 1, 3)) < 0.5
    on[np.arange(n), 0, g.integers(0, 3, n)] = True                            # apart along at least one axis
    a[:, 3:] += g.choice([-1.0, 1.0], (n, 1, 3)) * g.uniform(1.0, 2.0, (n, 1, 3)) * on
    out["apart"] = a
    return out


def pin_inputs(n, seed=7):
    """The seven sets of pin_sets as one array f64[n, 6, 3], the sets interleaved (so every n has them all)."""
    per = (n + 6) // 7
    s = pin_sets(per, seed)
    return np.ascontiguousarray(np.stack(list(s.values()), axis=1).reshape(-1, 6, 3)[:n])


# the hand-built table: name -> (A, B, n, mask)
def table():
    T = {}
    # one edge of each triangle pierces the other: A's edge 01 runs up through B's face, B's edge 20 comes back through A's
    T["one_each"] = ([[0, 0, -1], [0, 0, 1], [4, 0, 1]], [[-1, -1, 0], [1, -1, 0], [-1, 3, 0]], 2, 0b010001)
    # two edges of A through B: A's vertex 0 below B's plane, edges 01 and 20 cross it inside B
    T["two_of_a"] = ([[1, 1, -1], [1.5, 1, 1], [1, 1.5, 1]], [[0, 0, 0], [8, 0, 0], [0, 8, 0]], 2, 0b000101)
    # A's edge 01 through B's vertex 0: terms 0, 3 (B's edge 01 at t = 0) and 5 (B's edge 20 at t = 1) give the same point (0, 0, 0), term 4
    # (B's edge 12) gives (1, 1, 0).  Pairs in order: (0, 3) D = 0, (0, 4) D = 2 replaces it, (3, 4) and (4, 5) tie with it and lose
    T["through_vertex"] = ([[0, 0, -1], [0, 0, 1], [3, 3, 1]], [[0, 0, 0], [2, 0, 0], [0, 2, 0]], 2, 0b111001)
    # coplanar and overlapping: every edge is parallel to the other face
    T["coplanar"] = ([[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[1, 1, 0], [3, 1, 0], [1, 3, 0]], 0, 0)
    return {k: (np.array(a, dtype=np.float64), np.array(b, dtype=np.float64), n, m) for k, (a, b, n, m) in T.items()}


def grid_six_hits(seed=7, n=1 << 15):
    """The first pair of an integer-grid draw in which all six terms hit."""
    t = pin_sets(n, seed)["grid"]
    w = tri_isect_np(t)
    k = np.nonzero(w.code[:, 2] == 63)[0]
    return t[k[0]] if k.size else None


def grid_soup(n, seed, span=6, e=4):
    """n triangles of private vertices on the integer grid: a corner in 0..span-1, the vertices corner + 0..e."""
    g = np.random.default_rng(seed)
    c = g.integers(0, span, (n, 1, 3))
    v = (c + g.integers(0, e + 1, (n, 3, 3))).astype(np.float64)
    return np.ascontiguousarray(v.reshape(-1, 3)), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def self_meshes():
    """name -> (verts, vidx, ids): the meshes of the self call's test."""
    import mi355_synth as synth
    out = {}
    for n in (1, 2, 63, 64, 65, 513):
        v, i = br.soup(n, 0.3 if n <= 65 else 0.15, 40 + n)
        out[f"n{n}"] = (v, i, None)
    v, i = synth.soup(10_000, e=0.05, seed=3)
    out["soup10k"] = (v, i, None)
    v, i = synth.cloth_pair(70)                                                # two interpenetrating sheets, 19 600 triangles
    out["cloth70"] = (v, i, None)
    v, i = grid_soup(400, 5)
    out["grid400"] = (v, i, None)
    v, i = br.soup(600, 0.15, 77)
    v, i = br.with_degenerate(v, i, 78)
    out["degenerate"] = (v, i, None)
    v, i = br.soup(700, 0.15, 79)
    g = np.random.default_rng(80)
    out["custom_ids"] = (v, i, g.integers(0, 12, 700).astype(np.uint32) * 7 + 3)   # custom IDs, 12 values: one contact in 12 is between equal IDs
    return out


def between_cases():
    """name -> (va, ia, vb, ib, ids_a, ids_b)."""
    import mi355_synth as synth
    out = {}
    va, ia = br.soup(63, 0.3, 31)
    vb, ib = br.soup(65, 0.3, 32)
    out["soups"] = (va, ia, vb, ib, None, None)
    v, i = synth.cloth_pair(40)
    ca, cia, cb, cib = br.split(v, i, i.shape[0] // 2)
    out["cloth40"] = (ca, cia, cb, cib, None, None)
    vb1, ib1 = br.soup(1, 0.8, 33)
    out["nb1"] = (va, ia, vb1, ib1, None, None)
    sa, sia, sb, sib = br.shared_positions(300, 34)
    out["shared_positions"] = (sa, sia, sb, sib, None, None)
    ga, gia = grid_soup(150, 35)
    gb, gib = grid_soup(170, 36)
    g = np.random.default_rng(37)
    out["grid_ids"] = (ga, gia, gb, gib, g.integers(0, 50, 150).astype(np.uint32), g.integers(0, 50, 170).astype(np.uint32))
    return out


_cache = {}


def cached(key, fn):
    """fn() computed once per process and key: the references the tests share (never modified by them)."""
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]
