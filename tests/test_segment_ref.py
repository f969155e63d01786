"""Properties of seg_tri's numpy restatement (tests/segment_ref.py), the yardstick the device is compared with bit for bit
(tests/test_segments_gpu.py): what it is by construction -- pt_tri for a point, ray_tri for a crossing -- what it agrees with within a
measured bound -- tri_distance of the degenerate triangle (a, b, b), the distance of its own two points -- its scale equivariance and
its freedom from NaN, on generic soups, near pairs, integer-grid ties, slivers, degenerate triangles, segments through edges and
vertices, zero-length segments and pairs offset by 1e6 and 2^40 (segment_ref.pair_classes).

The bounds (segment_ref.WITNESS_BOUND, CROSS_WITNESS_BOUND, TRI_DISTANCE_BOUND) are the worst case measured on the restatement over
every input the tests use -- these classes and the rows of the shared items on every mesh -- rounded up to the next power of two,
times M, the pair's largest |coordinate| (DESIGN.md section 25 has the measurements):
    | |qs - qt| - dist |, cross = 0 rows                        worst 2^-50.69 M (degenerate triangles)        asserted 2^-50 M
    | |qs - qt| |, cross = 1 rows of WELL_CONDITIONED classes   worst 2^-46.26 M (through edges and vertices)  asserted 2^-46 M
    | dist - tri_distance((a, b, b), face) |                    worst 2^-48.13 M (degenerate triangles)        asserted 2^-48 M
A crossing's two points are ray_tri's P = a + t d and the point of its (u, v): on a segment within rounding of the face's plane
(grazing, in the plane, a sliver's plane) det is rounding noise, ray_tri's gate admits the hit and the two points can be as far apart
as the triangle is large (measured 2^-0.13 M).  That is ray_tri's behaviour on such input, stated in its contract; no bound is asserted
for those classes' crossing rows."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import point_ref as ptr
import proximity_ref as pr
import ray_ref as rr
import segment_ref as sr

N = 512
CLASSES = sr.pair_classes(N, 7)
ILL_CONDITIONED_CROSSINGS = ("ray_grazing", "ray_in_plane", "ray_degenerate")
BAND = (-300, -200, -127, -64, 64, 127, 128, 200, 300)                         # 2^k within ray_tri's band (tests/test_ray_ref.py)


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    if np.asarray(b).dtype == np.float64:
        a, b = _bits(a), _bits(b)
    assert np.array_equal(a, b), what


def test_every_class_is_there_and_every_term_group_wins():
    segs, tris = sr.pin_inputs(N, 7)
    assert segs.shape == (len(CLASSES) * N, 6) and tris.shape == (len(CLASSES) * N, 3, 3)
    term = sr.seg_tri_np(segs, tris).term
    counts = np.bincount(term + 2, minlength=16)
    print("crossings, coincident, terms 0..13:", counts[1], counts[0], counts[2:].tolist())
    assert (counts > 0).all()                                                   # the five coincident points, crossings and every one of the 14 terms


@pytest.mark.parametrize("name", list(CLASSES))
def test_a_point_segment_is_pt_tri_bit_for_bit(name):
    """a == b: dist, uv, feature, side and qt are point_ref's pt_tri(a), s = 0, end = 1, cross = 0, qs = a -- on the classes' own
    zero-length segments and on every class with b moved onto a."""
    segs, tris = CLASSES[name]
    a = segs[:, 0:3]
    t = sr.seg_tri_np(np.concatenate([a, a], axis=1), tris)
    dist, q, u, v, f, side = ptr.pt_tri_np(a, tris)
    for got, want, what in ((t.dist, dist, "dist"), (t.uv[:, 0], u, "u"), (t.uv[:, 1], v, "v"), (t.feature, f, "feature"), (t.side, side, "side"), (t.on_tri, q, "qt"),
                            (t.on_seg, a, "qs")):
        _same(got, want, (name, what))
    assert (t.cross == 0).all() and (t.end == 1).all() and (t.s == 0.0).all() and ((t.term >= 0) & (t.term < 4) | (t.term == -2)).all()


@pytest.mark.parametrize("name", list(CLASSES))
def test_crossings_are_ray_tris_hits(name):
    """cross == 1 exactly where ray_ref's ray_tri(a, b - a, tmax = 1) hits, with its t, u, v and side bits; dist = 0, feature = 0."""
    segs, tris = CLASSES[name]
    t = sr.seg_tri_np(segs, tris)
    a, d = segs[:, 0:3], segs[:, 3:6] - segs[:, 0:3]
    hit, ht, hu, hv, hside = rr.ray_tri_np(np.concatenate([a, d, np.ones((N, 1))], axis=1), tris)
    assert np.array_equal(t.cross == 1, hit)
    for got, want, what in ((t.s, ht, "t"), (t.uv[:, 0], hu, "u"), (t.uv[:, 1], hv, "v"), (t.side, hside, "side")):
        _same(got[hit], want[hit], (name, what))
    assert (t.dist[hit] == 0.0).all() and (t.feature[hit] == 0).all()
    _same(t.on_seg[hit], (a + ht[:, None] * d)[hit], (name, "qs"))
    if name == "zero_length":
        assert not hit.any()                                                    # an all-zero d misses by ray_tri's own arithmetic


def _dyadic(x):
    d = x.denominator
    return d & (d - 1) == 0 and d <= 1 << 20


def _exactly_representable(seg, tri):
    """Every quotient that seg_tri or tri_distance((a, b, b), tri) forms on this integer-grid pair -- the parameter of every point
    against every segment (the segment taken in both directions: tri_distance also has it as (b, a)), the face parameters of both ends,
    the parameters of the segment against every edge -- is a dyadic rational of few bits, so every operation of both is exact."""
    F = lambda v: [Fraction(int(x)) for x in v]
    A, B, T = F(seg[0:3]), F(seg[3:6]), [F(tri[j]) for j in range(3)]
    sub = lambda a, b: [a[k] - b[k] for k in range(3)]
    dot = lambda a, b: sum(a[k] * b[k] for k in range(3))
    segments = [(A, B), (B, A)] + [(T[e], T[(e + 1) % 3]) for e in range(3)]
    for p in (A, B, *T):
        for x, y in segments:
            e = sub(y, x)
            if dot(e, e) > 0 and not _dyadic(dot(sub(p, x), e) / dot(e, e)):
                return False
    ab, ac = sub(T[1], T[0]), sub(T[2], T[0])
    d00, d01, d11 = dot(ab, ab), dot(ab, ac), dot(ac, ac)
    den = d00 * d11 - d01 * d01
    if den > 0:
        for p in (A, B):
            ap = sub(p, T[0])
            d20, d21 = dot(ap, ab), dot(ap, ac)
            if not (_dyadic((d11 * d20 - d01 * d21) / den) and _dyadic((d00 * d21 - d01 * d20) / den)):
                return False
    for x, y in segments[:2]:
        for p2, q2 in segments[2:]:
            d1, d2, r = sub(y, x), sub(q2, p2), sub(x, p2)
            a, e, b, c, f = dot(d1, d1), dot(d2, d2), dot(d1, d2), dot(d1, r), dot(d2, r)
            den = a * e - b * b
            if den > 0 and not (_dyadic((b * f - c * e) / den) and _dyadic((a * f - b * c) / den)):
                return False
    return True


def _against_tri_distance(segs, tris):
    """(seg_tri, tri_distance of (a, b, b) against the face, the pairs the comparison holds for: no crossing, no contact early-out)."""
    t = sr.seg_tri_np(segs, tris)
    pair = np.concatenate([segs[:, None, 0:3], segs[:, None, 3:6], segs[:, None, 3:6], tris], axis=1)
    return t, pr.tri_distance_np(pair), (t.cross == 0) & ~pr.in_contact(pair)


def _dyadic_grid(g, n):
    """Integer-grid pairs built so that most of them are exactly representable: right isosceles triangles in a coordinate plane with
    legs along the axes or the diagonals, of length 1, 2 or 4 (every squared edge length and the face's denominator a power of two),
    and segments along an axis or a diagonal of a coordinate plane, axes permuted and mirrored at random."""
    L = 2.0 ** g.integers(0, 3, n)
    o = g.integers(-4, 5, (n, 3)).astype(np.float64)
    diag = g.random(n) < 0.5
    sg = g.choice([-1.0, 1.0], n)
    z = np.zeros(n)
    u = np.where(diag[:, None], np.stack([L, L, z], axis=1), np.stack([L, z, z], axis=1))
    v = np.where(diag[:, None], np.stack([L, -L, z], axis=1), np.stack([z, L, z], axis=1)) * sg[:, None]
    tris = np.stack([o, o + u, o + v], axis=1)
    a = g.integers(-4, 5, (n, 3)).astype(np.float64)
    l2 = 2.0 ** g.integers(0, 3, n)
    kind = g.integers(0, 4, n)                                                  # along x, along z, a diagonal of the triangle's plane, one across it
    d = np.select([(kind == 0)[:, None], (kind == 1)[:, None], (kind == 2)[:, None]],
                  [np.stack([l2, z, z], axis=1), np.stack([z, z, l2], axis=1), np.stack([l2, -l2, z], axis=1)], np.stack([l2, z, l2], axis=1))
    d *= g.choice([-1.0, 1.0], n)[:, None]
    segs = np.concatenate([a, a + d], axis=1)
    perm = np.argsort(g.random((n, 3)), axis=1)                                 # the same permutation and mirroring for both
    flip = g.choice([-1.0, 1.0], (n, 3))
    rows = np.arange(n)[:, None]
    tris = np.stack([tris[:, j][rows, perm] * flip for j in range(3)], axis=1)
    segs = np.concatenate([segs[:, 0:3][rows, perm] * flip, segs[:, 3:6][rows, perm] * flip], axis=1)
    return segs, tris


def test_tri_distance_of_the_degenerate_triangle_exactly_on_the_integer_grid():
    """Integer-grid pairs on which every quotient of both formulas is exactly representable: the two distances are the same bits.
    (On the grid at large a quotient such as 1 / 3 is rounded, tri_distance's extra terms -- the segment taken as (b, a) -- round
    differently, and the two can differ in the last bits: that is the bound's case, below.)"""
    segs, tris = _dyadic_grid(np.random.default_rng(3), 4 * N)
    t, td, ok = _against_tri_distance(segs, tris)
    exact = np.array([bool(ok[k]) and _exactly_representable(segs[k], tris[k]) for k in range(segs.shape[0])])
    print(f"{int(exact.sum())} of {int(ok.sum())} non-crossing grid pairs are exactly representable; {int((t.dist[exact] > 0).sum())} apart; "
          f"winning terms {np.bincount(t.term[exact] + 2, minlength=16).tolist()}")
    assert exact.sum() >= N // 2 and (t.dist[exact] > 0).sum() >= N // 4
    _same(t.dist[exact], td[exact], "integer grid")


@pytest.mark.parametrize("name", list(CLASSES))
def test_tri_distance_of_the_degenerate_triangle_within_the_bound(name):
    segs, tris = CLASSES[name]
    t, td, ok = _against_tri_distance(segs, tris)
    err = np.abs(td - t.dist)[ok] / sr.M_OF(segs, tris)[ok]
    print(name, int(ok.sum()), "pairs, worst", err.max() if err.size else 0.0)
    assert ok.sum() >= N // 8 and (err <= sr.TRI_DISTANCE_BOUND).all()


@pytest.mark.parametrize("name", list(CLASSES))
def test_the_two_points_are_dist_apart_within_the_bound(name):
    segs, tris = CLASSES[name]
    t = sr.seg_tri_np(segs, tris)
    err = np.abs(np.linalg.norm(t.on_seg - t.on_tri, axis=1) - t.dist) / sr.M_OF(segs, tris)
    c = t.cross == 1
    print(name, "cross = 0 worst", err[~c].max() if (~c).any() else 0.0, "cross = 1 worst", err[c].max() if c.any() else 0.0)
    assert (err[~c] <= sr.WITNESS_BOUND).all()
    if name not in ILL_CONDITIONED_CROSSINGS:
        assert (err[c] <= sr.CROSS_WITNESS_BOUND).all()
    # both points lie where their parameters say: s in [0, 1], u, v >= 0, u + v <= 1 up to the rounding of 1 - t
    assert ((t.s >= 0.0) & (t.s <= 1.0)).all() and (t.uv >= 0.0).all() and (t.uv.sum(axis=1) <= 1.0 + 2.0 ** -52).all()
    assert np.array_equal(t.end, np.where(t.s == 0.0, 1, np.where(t.s == 1.0, 2, 0)))


@pytest.mark.parametrize("name", [n for n in CLASSES if not n.startswith("offset")])
def test_scaling_by_a_power_of_two_scales_dist_and_points_exactly(name):
    """Over ray_tri's band: dist, qs, qt times 2^k, every other output the same bits.  (The offset classes lie at 2^20 and 2^40: another
    2^300 leaves the band.)"""
    segs, tris = CLASSES[name]
    want = sr.seg_tri_np(segs, tris)
    for k in BAND:
        got = sr.seg_tri_np(np.ldexp(segs, k), np.ldexp(tris, k))
        for field in ("s", "uv", "feature", "end", "cross", "side", "term"):
            _same(getattr(got, field), getattr(want, field), (name, k, field))
        for field in ("dist", "on_seg", "on_tri"):
            _same(getattr(got, field), np.ldexp(getattr(want, field), k), (name, k, field))


@pytest.mark.parametrize("name", list(CLASSES))
def test_finite_input_gives_no_nan(name):
    segs, tris = CLASSES[name]
    for k in (0, -300, 300) if not name.startswith("offset") else (0,):
        t = sr.seg_tri_np(np.ldexp(segs, k), np.ldexp(tris, k))
        assert all(np.isfinite(x).all() for x in (t.dist, t.s, t.on_seg, t.on_tri, t.uv)), (name, k)


def test_the_shared_items_rows_keep_the_bounds_and_conditions():
    """The rows of the shared items (the inputs of the GPU tests) on the small meshes: the bounds hold there too, and the item sets are
    what the row-set tests need (segment_ref.input_conditions)."""
    import within_ref as wr
    for name in sr.SMALL:
        sr.input_conditions(name)
        v, i, ids, edge = sr.MESHES[name]
        w = sr.want(name, 3.0)
        segs, tris = sr.segments(name)[w.rows[:, 0].astype(np.int64)], wr._mesh(v, i, ids)[0][w.rows[:, 1].astype(np.int64)]
        M = sr.M_OF(segs, tris)
        err = np.abs(np.linalg.norm(w.on_seg - w.on_tri, axis=1) - w.dist) / M
        assert (err[w.cross == 0] <= sr.WITNESS_BOUND).all() and (err[w.cross == 1] <= sr.CROSS_WITNESS_BOUND).all(), name
        t, td, ok = _against_tri_distance(segs, tris)
        assert (np.abs(td - t.dist)[ok] <= sr.TRI_DISTANCE_BOUND * M[ok]).all(), name


@pytest.mark.parametrize("name", sr.SCALE_MESHES)
def test_the_row_set_of_the_range_case_is_the_same_at_both_fp32_ends(name):
    """tests/test_segments_gpu.py expects the k = 0 rows at every scale of its band.  That is the restatement's own property: on mesh,
    ends and radius scaled by 2^-149 and 2^128 segments_within_ref gives the same set of (item, face), the same IDs, s, u, v, feature,
    end, cross and side, and dist and the two points times 2^k exactly.  The case has items without a row, items with several and
    crossings (scale_conditions)."""
    import scale_inputs as si
    vv, vidx, items, want = sr.scale_case(name)
    per = sr.scale_conditions(want)
    print(f"{name}: {want.rows.shape[0]} rows, {int((per == 0).sum())} of {sr.NSCALE} items with none, {int((per >= 2).sum())} with several, {int(want.cross.sum())} crossings")
    for k in (-149, 128):
        got = sr.segments_within_ref(si.scaled(vv, k), vidx, None, si.scaled(items, k))
        sr.wr.same_rows(got, sr.scaled_rows(want, k), f"{name} 2^{k}")
    off = sr.scale_case(name, 2.0 ** 20 + 0.37)[3]
    per = sr.scale_conditions(off)
    print(f"{name} translated: {off.rows.shape[0]} rows, {int((per == 0).sum())} items with none, {int((per >= 2).sum())} with several")
