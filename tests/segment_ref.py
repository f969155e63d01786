"""The segment queries restated on the CPU (no test in here): seg_tri in numpy, bit for bit as csrc/cd_math.h evaluates it, from the
blocks of tests/point_ref.py (pt_face2_vw, pt_seg2_t), tests/witness_ref.py (seg_seg2_st, the edge and vertex tables) and
tests/ray_ref.py (ray_tri); cd_segments_within and cd_segments_closest as ALL pairs of items and triangles -- no box filter of any
kind; the operand sets of the predicate's tests; and the items the CPU and GPU tests share.

seg_tri (include/mi355cd.h): the segment a + s (b - a) against (p0, p1, p2), d = b - a:
    h = ray_tri(a, d, 1.0, p0, p1, p2); a hit: cross 1, dist 0, s = t, (u, v), feature 0, side, qs = a + s d, qt = bary_point(u, v)
    else B = d, T_i = p_i - a; m = largest |component|; m == 0 -> dist 0, s = u = v = 0, feature 4, end 1, side 0, qs = a, qt = p0
    m = f 2^ex (frexp, |ex| clamped at 1000); B, T_i times 2^-ex; A = O; the minimum of 14 terms, strict '<' only:
        0 face(A; T)  1..3 seg(A; edges)  4 face(B; T)  5..7 seg(B; edges)  8..10 seg(T_i; A, B)  11..13 seg_seg(A, B; edge e)
    d all-zero: terms 0..3 only (pt_tri(a) bit for bit)
    dist = sqrt(best) 2^ex; side = (O - T0) . ((T1 - T0) x (T2 - T0)) > 0; qs = a / b / a + s d; qt = bary_point(u, v) on the originals
    end = 1 when s == 0, 2 when s == 1, else 0
A row set is sorted by (item, face), the order the comparisons use (the device's order is free)."""
from __future__ import annotations

import collections
import functools

import numpy as np

import point_ref as ptr
import ray_ref as rr
import within_ref as wr
import witness_ref as wit
from point_ref import EXP_MAX, _cross, _dot, _sub

NONE = np.uint32(0xFFFFFFFF)

SegTri = collections.namedtuple("SegTri", "dist s on_seg on_tri uv feature end cross side term")
SegRows = collections.namedtuple("SegRows", "rows ids dist s on_seg on_tri uv feature end cross side")


def _cols(x):
    return tuple(x[..., k] for k in range(3))


def _frame(a, d, P):
    """The non-crossing branch's operands: (B, T0, T1, T2) scaled, m, ex.  a, d: tuples of arrays; P: three such tuples."""
    T = [_sub(p, a) for p in P]
    m = np.zeros(np.broadcast(d[0], T[0][0]).shape)
    for vec in (d, *T):
        for k in range(3):
            x = np.abs(vec[k])
            m = np.where(x > m, x, m)
    ex = np.clip(np.frexp(m)[1], -EXP_MAX, EXP_MAX)
    sc = np.ldexp(1.0, -ex)
    B, T0, T1, T2 = (tuple(vec[k] * sc for k in range(3)) for vec in (d, *T))
    return B, (T0, T1, T2), m, ex


def _terms(B, T):
    """The 14 terms in order: (squared distance, s, u, v, feature) each, on the scaled operands."""
    zero = np.zeros(np.broadcast(B[0], T[0][0]).shape)
    O = (zero, zero, zero)
    out = []
    for P, s in ((O, 0.0), (B, 1.0)):
        x, fv, fw = ptr._pt_face2_vw(P, *T)
        out.append((x, zero + s, fv, fw, np.zeros(zero.shape, dtype=np.int64)))
        for e in range(3):
            x, t = ptr._pt_seg2_t(P, T[e], T[(e + 1) % 3])
            out.append((x, zero + s, *wit._edge(e, t)))
    for i in range(3):
        x, t = ptr._pt_seg2_t(T[i], O, B)
        u, v, f = wit._vertex(i, zero)
        out.append((x, t, u, v, np.full(zero.shape, f, dtype=np.int64)))
    for e in range(3):
        x, s, t = wit._seg_seg2_st(O, B, T[e], T[(e + 1) % 3])
        out.append((x, s, *wit._edge(e, t)))
    return out


def _ray_hit(a, d, p):
    """ray_tri(a, d, 1.0, p): (hit, t, u, v, side) on [n, 3] / [n, 3, 3] arrays."""
    return rr.ray_tri_np(np.concatenate([a, d, np.ones((a.shape[0], 1))], axis=1), p)


def seg_tri_np(segs, tris) -> SegTri:
    """segs [n, 6] (a, b), tris [n, 3, 3] -> SegTri; term: the winning term 0..13 (-1: a crossing, -2: the five coincident points)."""
    sg = np.asarray(segs, dtype=np.float64).reshape(-1, 6)
    p = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    a, b = sg[:, 0:3], sg[:, 3:6]
    n = a.shape[0]
    with np.errstate(all="ignore"):
        d = b - a
        hit, ht, hu, hv, hside = _ray_hit(a, d, p)
        B, T, m, ex = _frame(_cols(a), _cols(d), [_cols(p[:, j]) for j in range(3)])
        dzero = (d == 0.0).all(axis=1)
        best = np.full(n, np.inf)
        s, u, v = np.zeros(n), np.zeros(n), np.zeros(n)
        f = np.zeros(n, dtype=np.int64)
        win = np.zeros(n, dtype=np.int64)
        for k, (x, ts, tu, tv, tf) in enumerate(_terms(B, T)):
            rep = (x < best) & ((k < 4) | ~dzero)
            best = np.where(rep, x, best)
            s, u, v, f, win = np.where(rep, ts, s), np.where(rep, tu, u), np.where(rep, tv, v), np.where(rep, tf, f), np.where(rep, k, win)
        dist = np.sqrt(best) * np.ldexp(1.0, ex)
        zero = np.zeros(n)
        O = (zero, zero, zero)
        side = _dot(_sub(O, T[0]), _cross(_sub(T[1], T[0]), _sub(T[2], T[0]))) > 0.0
        none = ~(m > 0.0)
        dist, s, u, v = (np.where(none, 0.0, x) for x in (dist, s, u, v))
        f, side, win = np.where(none, 4, f), side & ~none, np.where(none, -2, win)
        # the crossing branch replaces everything
        dist, s, u, v = np.where(hit, 0.0, dist), np.where(hit, ht, s), np.where(hit, hu, u), np.where(hit, hv, v)
        f, side, win = np.where(hit, 0, f), np.where(hit, hside != 0, side), np.where(hit, -1, win)
        end = np.where(s == 0.0, 1, np.where(s == 1.0, 2, 0))
        qs = a + s[:, None] * d
        qs = np.where((hit | (end == 0))[:, None], qs, np.where((end == 1)[:, None], a, b))
        qt = ptr.point_from_uv(u, v, p)
        qt = np.where(none[:, None] & ~hit[:, None], p[:, 0], qt)
    return SegTri(dist, s, qs, qt, np.stack([u, v], axis=1), f.astype(np.uint8), end.astype(np.uint8), hit.astype(np.uint8), side.astype(np.uint8), win)


def _dist_all(a, d, P):
    """seg_tri's dist without the crossing branch on broadcastable tuples: [items, triangles]."""
    B, T, m, ex = _frame(a, d, P)
    dzero = (d[0] == 0.0) & (d[1] == 0.0) & (d[2] == 0.0)
    zero = np.zeros(m.shape)
    O = (zero, zero, zero)
    best = np.full(m.shape, np.inf)

    def take(x, always=False):
        nonlocal best
        best = np.where((x < best) & (always | ~dzero), x, best)

    for P_, first in ((O, True), (B, False)):
        take(ptr._pt_face2_vw(P_, *T)[0], first)
        for e in range(3):
            take(ptr._pt_seg2_t(P_, T[e], T[(e + 1) % 3])[0], first)
    for i in range(3):
        take(ptr._pt_seg2_t(T[i], O, B)[0])
    for e in range(3):
        take(wit._seg_seg2_st(O, B, T[e], T[(e + 1) % 3])[0])
    return np.where(m > 0.0, np.sqrt(best) * np.ldexp(1.0, ex), 0.0)


def segments_within_ref(verts, vidx, ids, segs, pairs_per_chunk=1 << 18, threads=8) -> SegRows:
    """Every segment [n, 7] (a, b, r) against ALL triangles (chunks of segments): a row wherever seg_tri's dist <= r, with seg_tri's
    values."""
    p, ids = wr._mesh(verts, vidx, ids)
    nt = p.shape[0]
    sg = np.asarray(segs, dtype=np.float64).reshape(-1, 7)
    n = sg.shape[0]
    a, d, r = sg[:, 0:3], sg[:, 3:6] - sg[:, 0:3], sg[:, 6]
    P = [tuple(np.ascontiguousarray(p[:, j, k])[None, :] for k in range(3)) for j in range(3)]
    p0 = np.ascontiguousarray(p[:, 0])
    e1, e2 = p[:, 1] - p0, p[:, 2] - p0
    step = max(1, pairs_per_chunk // max(nt, 1))

    def work(lo):
        hi = min(n, lo + step)
        with np.errstate(all="ignore"):
            dist = _dist_all(tuple(a[lo:hi, k][:, None] for k in range(3)), tuple(d[lo:hi, k][:, None] for k in range(3)), P)
            ok = rr._stage_u(a[lo:hi, None, :], d[lo:hi, None, :], p0[None], e1[None], e2[None])[0]      # ray_tri's first exit thins the pairs out
        ri, ti = np.nonzero(ok)
        hit = _ray_hit(a[lo + ri], d[lo + ri], p[ti])[0]
        dist[ri[hit], ti[hit]] = 0.0
        ri, ti = np.nonzero(dist <= r[lo:hi, None])
        return lo + ri, ti

    k, f = wr._pairs(wr._chunks(work, n, step, threads))
    t = seg_tri_np(sg[k, 0:6], p[f])                                            # the rows again, with everything (the same bits)
    assert (t.dist <= r[k]).all()
    return SegRows(np.stack([k, f], axis=1).astype(np.uint32), ids[f], *t[:9])


def closest_of(w: SegRows, n):
    """The per-segment minimum of a row set as cd_segments_closest returns it: (face, ids, dist, s, on_seg, on_tri, uv, feature, end,
    cross, side)."""
    at, k = wr.per_item(w)
    face = np.full(n, NONE, dtype=np.uint32)
    face[k] = w.rows[at, 1]
    out = [face]
    for name, x in zip(w._fields[1:], w[1:]):
        o = np.full((n,) + x.shape[1:], np.inf if name == "dist" else 0, dtype=x.dtype)
        o[k] = x[at]
        out.append(o)
    return tuple(out)


def segments_closest_ref(verts, vidx, ids, segs):
    """cd_segments_closest over all pairs: the smallest (dist, ID, face) row of segments_within_ref per item."""
    n = np.asarray(segs).reshape(-1, 7).shape[0]
    return closest_of(segments_within_ref(verts, vidx, ids, segs), n)


def restrict(w: SegRows, segs, factor_r):
    """The rows of w (computed at a radius at least as large) with dist <= factor_r (a scalar or [n])."""
    r = np.broadcast_to(np.asarray(factor_r, dtype=np.float64), (np.asarray(segs).reshape(-1, 7).shape[0],))
    keep = w.dist <= r[w.rows[:, 0].astype(np.int64)]
    return SegRows(*(x[keep] for x in w))


# ---------------------------------------------------------------- operand sets of the predicate's tests
def _segs_of_rays(r):
    """The segment o .. o + d of a ray with a finite direction."""
    return np.concatenate([r[:, 0:3], r[:, 0:3] + r[:, 3:6]], axis=1)


def pair_classes(n, seed=0):
    """name -> (segs [n, 6], tris [n, 3, 3]): generic soups, near pairs, integer-grid ties, slivers, degenerate triangles, segments
    through edges and vertices, zero-length segments, offsets 1e6 and 2^40."""
    g = np.random.default_rng(seed)
    out = {}
    tri = lambda: g.uniform(-1.0, 1.0, (n, 3, 3))
    out["random"] = (g.uniform(-2.0, 2.0, (n, 6)), tri())
    c, p = ptr.pair_classes(n, seed + 1)["on_face"]                             # near pairs: a short segment close to the triangle
    a = c + g.normal(0.0, 0.05, (n, 3))
    out["near"] = (np.concatenate([a, a + g.normal(0.0, 0.2, (n, 3))], axis=1), p)
    out["grid"] = (g.integers(-3, 4, (n, 6)).astype(np.float64), g.integers(-3, 4, (n, 3, 3)).astype(np.float64))      # ties, exact arithmetic
    for name in ("random", "grazing", "vertex_edge", "in_plane", "degenerate", "axis", "on_triangle"):               # ray_ref's classes as segments
        r, p = rr.pair_classes(n, seed + 2)[name]
        sc = np.where(np.isfinite(r[:, 6]) & (r[:, 6] > 0), np.minimum(r[:, 6], 4.0), g.uniform(0.5, 2.0, n))        # ends before, on and behind the plane
        rs = r.copy(); rs[:, 3:6] *= sc[:, None]
        out["ray_" + name] = (_segs_of_rays(rs), p)
    for name in ("sliver", "degenerate", "on_edge", "on_vertex"):                                                    # point_ref's classes, a segment from the point
        q, p = ptr.pair_classes(n, seed + 3)[name]
        out["pt_" + name] = (np.concatenate([q, q + g.normal(0.0, 0.5, (n, 3)) * (g.random(n) < 0.8)[:, None]], axis=1), p)
    q, p = ptr.pair_classes(n, seed + 4)["random"]
    out["zero_length"] = (np.concatenate([q, q], axis=1), p)
    q, p = ptr.pair_classes(n, seed + 4)["degenerate"]
    out["zero_length_degenerate"] = (np.concatenate([q, q], axis=1), p)
    s0, p0 = out["random"]
    s1, p1 = out["near"]
    for off, tag in ((1e6, "1e6"), (2.0 ** 40, "2p40")):
        out["offset_" + tag] = (np.concatenate([s0, s1])[:n] + off, np.concatenate([p0, p1])[:n] + off)
    return out


def pin_inputs(n=512, seed=7):
    """(segs, tris) of every class, concatenated: the vectors the CPU tests use and the device's pin."""
    c = pair_classes(n, seed)
    return np.concatenate([v[0] for v in c.values()]), np.concatenate([v[1] for v in c.values()])


M_OF = lambda segs, tris: np.maximum(np.abs(np.asarray(segs).reshape(-1, 6)).max(axis=1), np.abs(np.asarray(tris).reshape(-1, 9)).max(axis=1))

# The bounds, times M (the pair's largest |coordinate|): the worst case measured on the restatement over every input the tests use
# (pin_inputs and the shared items' rows), rounded up to the next power of two (DESIGN.md section 25 records measurement and margin).
WITNESS_BOUND = 2.0 ** -50          # | |qs - qt| - dist | on cross = 0 rows (worst 2^-50.69 M)
CROSS_WITNESS_BOUND = 2.0 ** -46    # | qs - qt | on cross = 1 rows of segments that are not within rounding of the face's plane (worst 2^-46.26 M)
TRI_DISTANCE_BOUND = 2.0 ** -48     # | dist - tri_distance((a, b, b), face) | on non-crossing, non-contact pairs (worst 2^-48.13 M)


# ---------------------------------------------------------------- the items of the tests
MESHES = wr.MESHES
SMALL = wr.SMALL
SEED = 11
n_items = wr.n_items
FACTORS = (1.0, 3.0)


@functools.lru_cache(maxsize=None)
def segments(name, n=None):
    """[n, 6]: segments whose first ends are placed as within_ref.points places points, with random directions and lengths around
    2 edge (U(0.5, 3.5) edge); every 16th has zero length."""
    v, i, ids, edge = MESHES[name]
    n = n or n_items(name)
    a = ptr.mesh_points(v, i, n, seed=SEED, edge=edge)
    g = np.random.default_rng(SEED + 1)
    u = g.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    b = a + u * (edge * g.uniform(0.5, 3.5, n))[:, None]
    b[::16] = a[::16]
    return np.ascontiguousarray(np.concatenate([a, b], axis=1))


def items(name, factor, n=None):
    v, i, ids, edge = MESHES[name]
    s = segments(name, n)
    return np.ascontiguousarray(np.concatenate([s, np.full((s.shape[0], 1), factor * edge)], axis=1))


@functools.lru_cache(maxsize=None)
def want(name, factor, n=None):
    """The rows of segments(name, n) at radius factor * the mesh's edge (3 edge is computed; smaller radii are its rows within them)."""
    v, i, ids, edge = MESHES[name]
    if factor == 3.0:
        return segments_within_ref(v, i, ids, items(name, 3.0, n))
    assert factor < 3.0
    return restrict(want(name, 3.0, n), items(name, factor, n), factor * edge)


def term_groups(name, factor=3.0):
    """Rows of the set won by a crossing, by terms 0-7, 8-10, 11-13."""
    v, i, ids, edge = MESHES[name]
    w = want(name, factor)
    p = wr._mesh(v, i, ids)[0]
    t = seg_tri_np(segments(name)[w.rows[:, 0].astype(np.int64)], p[w.rows[:, 1].astype(np.int64)]).term
    return int((t == -1).sum()), int(((t >= 0) & (t < 8)).sum()), int(((t >= 8) & (t < 11)).sum()), int((t >= 11).sum())


def input_conditions(name):
    """What the tests of the row sets need of their items, per mesh, asserted on the restatement alone.  At each radius (edge, 3 edge)
    the item set has items with no row, with exactly one row and with two or more rows; rows with cross = 1 and rows with cross = 0; and
    on the meshes of at least 1000 triangles rows won by each of the term groups 0-7, 8-10 and 11-13.  Two exceptions, by geometry and
    not by seed: n1 is one triangle, so no item has two rows; and on cloth100 no item has exactly one row at either radius -- the sheets
    are tessellated at the radius' own scale, so a capsule that reaches a sheet reaches several of its triangles (seeds 1 .. 16 were
    tried: 0 of 256 every time).
    Figures with seed 11, n = 1000 (cloth100: 256), as (no row, one row, two or more) at edge, at 3 edge, and the rows at 3 edge won by
    (a crossing, terms 0-7, 8-10, 11-13):
        soup10k    (272, 67, 661) (230, 5, 765) (239, 25708, 9784, 1638)      duplicates (283, 17, 700) (209, 6, 785) (400, 55352, 22536, 4391)
        custom_ids (310, 130, 560) (239, 8, 753) (231, 12935, 4989, 859)      comb       (579, 31, 390) (549, 26, 425) (399, 482, 26, 109)
        n1         (240, 760, 0) (217, 783, 0) (238, 375, 32, 138)            n3         (456, 539, 5) (190, 241, 569) (204, 862, 309, 74)
        n65        (295, 89, 616) (197, 16, 787) (204, 11974, 5209, 1107)     cloth100   (89, 0, 167) (79, 0, 177) (295, 25694, 10500, 2617)"""
    n, nt = n_items(name), MESHES[name][1].shape[0]
    counts = [wr.rows_per_item(want(name, f), n) for f in FACTORS]
    groups = term_groups(name)
    print(name, [(int((c == 0).sum()), int((c == 1).sum()), int((c >= 2).sum())) for c in counts], groups)
    for c, f in zip(counts, FACTORS):
        w = want(name, f)
        assert (c == 0).any() and (w.cross == 1).any() and (w.cross == 0).any(), (name, f)
        assert (c == 1).any() or name == "cloth100", (name, f)
        assert (c >= 2).any() or nt == 1, (name, f)
        assert nt > 1 or c.max() <= 1
    if nt >= 1000:
        assert all(g > 0 for g in groups), (name, groups)


# ---------------------------------------------------------------- the case of the range tests (tests/test_segments_gpu.py section 10, tests/test_segment_ref.py)
SCALE_MESHES = ("cloth", "centred")         # of tests/scale_inputs.py: a cloth pair away from the origin, a soup with both signs on every axis
NSCALE = 512


@functools.lru_cache(maxsize=None)
def scale_case(name, off=0.0):
    """(verts, vidx, items [NSCALE, 7], the restatement's rows) at k = 0: segments at the mesh (a as point_ref.mesh_points places
    points, b = a + N(0, 1 edge) a coordinate), radius a quarter edge or one edge by i % 2; with `off` the mesh and both ends are
    translated by it.  Another scale takes scale_inputs.scaled() of these, never items of its own."""
    import scale_inputs as si
    v, vidx, edge = si.meshes()[name]
    vv = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    a = ptr.mesh_points(vv, vidx, NSCALE, seed=3, edge=edge)
    b = a + np.random.default_rng(21).normal(size=a.shape) * edge
    r = np.where(np.arange(NSCALE) % 2 == 0, 0.25 * edge, edge)
    items = np.ascontiguousarray(np.concatenate([a, b, r[:, None]], axis=1))
    if off:
        vv = vv + off
        items[:, 0:6] += off
    return vv, vidx, items, segments_within_ref(vv, vidx, None, items)


def scale_conditions(w: SegRows):
    """What the range tests need of the case: at least 32 items without a row, at least 32 with several, a crossing row."""
    per = wr.rows_per_item(w, NSCALE)
    assert (per == 0).sum() >= 32 and (per >= 2).sum() >= 32 and (w.cross == 1).any(), (int((per == 0).sum()), int((per >= 2).sum()), int(w.cross.sum()))
    return per


def scaled_rows(w: SegRows, k) -> SegRows:
    """The rows of the case at 2^k, from the k = 0 rows: dist and the two points times 2^k, everything else unchanged."""
    return w._replace(dist=np.ldexp(w.dist, k), on_seg=np.ldexp(w.on_seg, k), on_tri=np.ldexp(w.on_tri, k))
