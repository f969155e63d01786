"""CPU checks of the swept-segment restatement (tests/swept_segment_ref.py).

The guarantee, with h = dist / 2, M the pair's largest |coordinate| over both ends and delta = 2^-38 M:
  1. a segment that comes closer than h - delta to the exactly, linearly moving triangle at some t* is reported with toi <= t*, and is
     never closer than h - delta before toi;
  2. a reported, resolved pair is within dist + delta at toi.
Both are checked against exact rationals: positions x + t (y - x) at dyadic t as Fractions and the exact segment-triangle distance.
Half 2 is not asserted for cross = 1 reports of the exempt classes (swept_segment_ref.EXEMPT: degenerate faces, where ray_tri's hit is
rounding noise -- an early report, never a late one); half 1 is asserted on every class."""
from __future__ import annotations

from fractions import Fraction
import math

import numpy as np
import pytest

import mi355_synth as synth
import scale_inputs as si
import segment_ref as sref
import sweep_ref as swr
import swept_segment_ref as ssr

BIG = np.array([[-10.0, -10.0, 0.0], [10.0, -10.0, 0.0], [0.0, 10.0, 0.0]])
GUARANTEE_CLASSES = tuple(k for k in ssr.CLASSES if k not in ("pt_long", "pt_unresolved", "pt_scaled_up", "pt_scaled_down", "pt_translate"))


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b)) if np.asarray(b).dtype == np.float64 else np.array_equal(a, b)


@pytest.mark.parametrize("H,v,dist", [(1.0, 2.0, 0.01), (0.5, 3.0, 0.001), (2.0, 2.5, 0.1)])
def test_falling_horizontal_segment(H, v, dist):
    it = ssr.pack([-0.5, 0.2, H], [0.6, 0.1, H], [-0.5, 0.2, H - v], [0.6, 0.1, H - v], dist)
    adv = ssr.seg_advance_np(it, np.concatenate([BIG, BIG])[None])
    assert (H - dist) / v <= adv.toi[0] <= (H - dist / 2) / v, adv
    assert adv.dist[0] <= dist and adv.cross[0] == 0 and adv.side[0] == 1 and adv.on_tri[0, 2] == 0.0


def test_edge_on_pass_is_an_edge_edge_report_no_sample_sees():
    """The case that motivates the call: a long segment parallel to a thin sheet passes through it inside the step.  Both ends and the
    midpoint stay farther than dist from the triangle throughout (they pass beside it), the segment at t = 0 and at t = 1 is farther
    than dist away, and seg_advance reports an edge-edge contact strictly inside the step."""
    tri = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    a0, b0 = np.array([0.9, -3.0, 0.5]), np.array([0.9, 5.0, 0.5])                # the line x = 0.9 cuts the corner at vertex 1: y in [0, 0.1]
    down = np.array([0.0, 0.0, -1.0])
    it = ssr.pack(a0, b0, a0 + down, b0 + down, 0.01)
    six = np.concatenate([tri, tri])[None]
    adv = ssr.seg_advance_np(it, six)
    assert 0.0 < adv.toi[0] < 1.0 and adv.dist[0] <= 0.01 and adv.cross[0] == 0 and adv.feature[0] in (1, 2, 3) and adv.end[0] == 0
    assert abs(adv.toi[0] - 0.5) < 0.011
    for p0 in (a0, b0, 0.5 * (a0 + b0)):                                       # the samples: end points and midpoint, at 3 dist
        assert np.isinf(swr.pt_advance_np(np.array([[*p0, *(p0 + down), 0.03]]), six).toi[0])
    for z in (0.0, 1.0):                                                       # the static query at both ends of the step
        assert sref.seg_tri_np(np.concatenate([a0 + z * down, b0 + z * down])[None], tri[None]).dist[0] > 0.4


def test_exact_distance_blocks():
    tri = tuple(ssr._fr(x) for x in BIG)
    F = Fraction
    assert ssr.exact_seg_tri_d2(((F(0), F(0), F(1)), (F(0), F(0), F(-1))), tri) == 0          # through the face
    assert ssr.exact_seg_tri_d2(((F(0), F(0), F(1)), (F(0), F(0), F(1, 2))), tri) == F(1, 4)   # short of it: the end's face term
    assert ssr.exact_seg_tri_d2(((F(-20), F(-10), F(3)), (F(20), F(-10), F(3))), tri) == 9     # over edge 0-1: edge against edge
    assert ssr.exact_seg_tri_d2(((F(-1), F(0), F(0)), (F(1), F(0), F(0))), tri) == 0           # in the plane, inside
    assert ssr.exact_seg_tri_d2(((F(0), F(11), F(-1)), (F(0), F(11), F(1))), tri) == 1         # beside vertex 2: the vertex against the segment
    g = np.random.default_rng(2)
    it7, t = swr.pin_class("random", 20, g)
    for k in range(20):                                                         # a zero-length segment: sweep_ref's exact point distance
        (a, b), p = ssr.exact_at(ssr.point_items(it7[k:k + 1])[0], t[k], Fraction(1, 4))
        assert a == b and ssr.exact_seg_tri_d2((a, b), p) == swr.exact_dist2(*swr.exact_at(it7[k], t[k], Fraction(1, 4)))


def test_common_translation_costs_one_evaluation():
    it, t = ssr.pin_class("pt_translate", 64, np.random.default_rng(3))
    assert np.all(ssr.rate_np(it, t) == 0.0)
    adv = ssr.seg_advance_np(it, t)
    assert np.all(adv.evals == 1) and np.all((adv.toi == 0.0) | np.isinf(adv.toi)) and (adv.toi == 0.0).any() and np.isinf(adv.toi).any()
    st = sref.seg_tri_np(it[:, 0:6], t[:, :3])
    assert _same(adv.dist, st.dist) and _same(adv.on_seg, st.on_seg)         # the one evaluation is on the start positions themselves
    assert np.array_equal(np.isfinite(adv.toi), st.dist <= it[:, 12])


def test_point_items_are_pt_advance_bit_for_bit():
    inputs = swr.pin_inputs(128, seed=4)
    it7, t = np.concatenate([v[0] for v in inputs.values()]), np.concatenate([v[1] for v in inputs.values()])
    want = swr.pt_advance_np(it7, t)
    got = ssr.seg_advance_np(ssr.point_items(it7), t)
    assert np.isfinite(want.toi).sum() > 300 and (want.evals == swr.MAX_EVALS).any()
    assert _same(got.toi, want.toi) and np.array_equal(got.evals, want.evals) and _same(got.dist, want.dist) and _same(got.uv, want.uv)
    assert np.array_equal(got.feature, want.feature) and np.array_equal(got.side, want.side) and _same(got.on_tri, want.closest)
    assert not got.cross.any() and np.all(got.end == 1) and np.all(got.s == 0.0)
    assert np.array_equal(_bits(ssr.rate_np(ssr.point_items(it7), t)), _bits(swr.rate_np(it7, t)))
    assert np.array_equal(ssr.gate_np(ssr.point_items(it7), t), swr.gate_np(it7, t))


def _case(n_tri=600, n_items=200, seed=5, dist=0.02):
    verts, vidx = synth.soup(n_tri, e=0.1, seed=seed)
    g = np.random.default_rng(seed + 1)
    x1 = verts + g.normal(size=verts.shape) * 0.03
    import point_ref as ptr
    a0 = ptr.mesh_points(verts, vidx, n_items, seed=seed, edge=0.1)
    b0 = a0 + g.normal(size=a0.shape) * 0.1
    return verts, x1, vidx, ssr.pack(a0, b0, a0 + g.normal(size=a0.shape) * 0.1, b0 + g.normal(size=a0.shape) * 0.1, dist)


def test_no_motion_is_segments_within_bit_for_bit():
    verts, x1, vidx, it = _case(dist=0.04)
    still = it.copy(); still[:, 6:12] = still[:, 0:6]
    w, (gate, evals, unres) = ssr.sweep_segment_rows_ref(verts, None, vidx, None, still, counts=True)
    want = sref.segments_within_ref(verts, vidx, None, np.concatenate([still[:, 0:6], still[:, 12:13]], axis=1))
    assert want.rows.shape[0] > 50 and np.array_equal(w.rows, want.rows) and np.all(w.toi == 0.0) and evals == gate and unres == 0
    assert (want.cross == 1).any() and (want.cross == 0).any()
    for name in want._fields[1:]:
        assert _same(getattr(w, name), getattr(want, name)), name


def test_rows_are_the_gated_pairs_the_advancement_reports_and_skip_removes_both_indices():
    verts, x1, vidx, it = _case()
    w, (tested, evals, unres) = ssr.sweep_segment_rows_ref(verts, x1, vidx, None, it, counts=True)
    n, nt = it.shape[0], vidx.shape[0]
    six = np.concatenate([verts[vidx], x1[vidx]], axis=1)
    k, f = np.divmod(np.arange(n * nt), nt)                                    # every pair, one by one
    g = ssr.gate_np(it[k], six[f])
    adv = ssr.seg_advance_np(it[k[g]], six[f[g]])
    hit = np.isfinite(adv.toi)
    assert tested == g.sum() and evals == adv.evals.sum() and w.rows.shape[0] == hit.sum() > 50
    assert np.array_equal(w.rows, np.stack([k[g][hit], f[g][hit]], axis=1)) and _same(w.toi, adv.toi[hit])
    rest = np.nonzero(~g)[0][:: max(1, (~g).sum() // 3000)]                    # a pair the gate turns away reports nothing when advanced all the same
    assert np.all(np.isinf(ssr.seg_advance_np(it[k[rest]], six[f[rest]]).toi))
    # the mesh's own edges with skip_vertices = the edge: no row's face holds either index, and the rest of the rows stay
    e = np.unique(np.sort(np.concatenate([vidx[:, [0, 1]], vidx[:, [1, 2]], vidx[:, [2, 0]]]).astype(np.int64), axis=1), axis=0)[:300]
    own = ssr.pack(verts[e[:, 0]], verts[e[:, 1]], x1[e[:, 0]], x1[e[:, 1]], 0.02)
    plain = ssr.sweep_segment_rows_ref(verts, x1, vidx, None, own)
    skipped = ssr.sweep_segment_rows_ref(verts, x1, vidx, None, own, skip=e)
    fv = vidx[plain.rows[:, 1].astype(np.int64)].astype(np.int64)
    inc = (fv[:, :, None] == e[plain.rows[:, 0].astype(np.int64)][:, None, :]).any(axis=(1, 2))
    assert inc.sum() >= e.shape[0] and np.all(plain.toi[inc] == 0.0)           # every face on the edge: a row at toi 0
    assert np.array_equal(skipped.rows, plain.rows[~inc]) and _same(skipped.toi, plain.toi[~inc])
    half = e.copy(); half[:, 1] = 0xFFFFFFFF                                   # one index and none
    w1 = ssr.sweep_segment_rows_ref(verts, x1, vidx, None, own, skip=half)
    inc1 = (fv == e[plain.rows[:, 0].astype(np.int64), 0:1]).any(axis=1)
    assert np.array_equal(w1.rows, plain.rows[~inc1])


def test_first_of_is_the_smallest_row():
    verts, x1, vidx, it = _case(dist=0.06)
    ids = np.random.default_rng(2).integers(0, 50, vidx.shape[0]).astype(np.uint32)   # repeated IDs: the face index decides
    w = ssr.sweep_segment_rows_ref(verts, x1, vidx, ids, it)
    first = ssr.first_of(w, it.shape[0])
    face, oid, toi, dist = first[:4]
    seen = 0
    for k in range(it.shape[0]):
        at = np.nonzero(w.rows[:, 0] == k)[0]
        if at.size == 0:
            assert face[k] == ssr.NONE and np.isinf(toi[k]) and all(not np.any(x[k]) for x in (oid, *first[3:]))
            continue
        best = min(at, key=lambda r: (w.toi[r], w.ids[r], w.rows[r, 1]))
        assert face[k] == w.rows[best, 1] and oid[k] == w.ids[best] and toi[k] == w.toi[best] and dist[k] == w.dist[best]
        for x, y in zip(first[4:], w[4:]):
            assert np.array_equal(x[k], y[best])
        seen += at.size > 1
    assert seen > 20


# ---------------------------------------------------------------- the guarantee
def _m(it, tri):
    return max(float(np.max(np.abs(it[:12]))), float(np.max(np.abs(tri))))


def _check_half_1(it, tri, adv, samples=16):
    checked = 0
    for k in range(it.shape[0]):
        lim = it[k, 12] * 0.5 - ssr.DELTA * _m(it[k], tri[k])
        if lim <= 0:
            continue
        lim2 = Fraction(lim) ** 2
        toi = adv.toi[k]
        end = 1.0 if np.isinf(toi) else float(toi)
        ts = [Fraction(i, samples) for i in range(samples + 1) if Fraction(i, samples) < Fraction(end)]
        if np.isfinite(toi) and toi > 0:
            ts += [Fraction(end) * (1 - Fraction(1, 2 ** e)) for e in (4, 10, 30)]
        elif np.isinf(toi):
            ts.append(Fraction(1))
        for t in ts:
            assert ssr.exact_seg_tri_d2(*ssr.exact_at(it[k], tri[k], t)) >= lim2, (k, float(t), toi, adv.dist[k], adv.evals[k], adv.cross[k])
            checked += 1
    return checked


@pytest.mark.parametrize("kind", GUARANTEE_CLASSES)
def test_guarantee_against_exact_rationals(kind):
    g = np.random.default_rng(ssr.CLASSES.index(kind) + 1)
    it, t = ssr.pin_class(kind, 24, g)
    adv = ssr.seg_advance_np(it, t)
    checked = _check_half_1(it, t, adv)                                         # half 1: on every class
    if kind not in ("pt_start_within", "cross_start"):                         # (those report at t = 0: there is no time before toi)
        assert checked > 60, checked
    rep = np.isfinite(adv.toi) & (adv.dist <= it[:, 12])
    if kind not in ("pt_near_parallel", "pt_random", "zero_length"):
        assert rep.sum() >= 5
    n2 = 0
    for k in np.nonzero(rep)[0]:                                               # half 2: a reported, resolved pair IS within dist at toi, up to delta
        if adv.cross[k] and kind in ssr.EXEMPT:
            continue
        d2 = ssr.exact_seg_tri_d2(*ssr.exact_at(it[k], t[k], Fraction(float(adv.toi[k]))))
        assert d2 <= Fraction(it[k, 12] + ssr.DELTA * _m(it[k], t[k])) ** 2, (k, adv.toi[k], adv.dist[k], adv.cross[k], math.sqrt(float(d2)))
        n2 += 1
    print(kind, "half 1 samples", checked, "half 2 pairs", n2)


@pytest.mark.parametrize("kind", ["pt_scaled_up", "pt_scaled_down"])
def test_guarantee_scaled(kind):
    it, t = ssr.pin_class(kind, 16, np.random.default_rng(9))
    adv = ssr.seg_advance_np(it, t)
    assert _check_half_1(it, t, adv, samples=8) > 60 and np.isfinite(adv.toi).sum() >= 3


def measured_seg_tri_error(count=12, seed=3):
    """max over the operands the advancement evaluates, per class, of | seg_tri.dist - exact distance | / M: the positions at t = 0, at
    toi (or the last t) and at one t between, formed as the device forms them (floats), against the exact distance of those floats."""
    worst = {}
    g = np.random.default_rng(seed)
    for kind in ssr.CLASSES:
        it, t = ssr.pin_class(kind, count, g)
        n = it.shape[0]
        adv = ssr.seg_advance_np(it, t)
        last = np.where(np.isfinite(adv.toi), adv.toi, 1.0)
        w = 0.0
        for stage, tt in ((np.zeros(n, dtype=np.int8), np.zeros(n)), (np.ones(n, dtype=np.int8), 0.5 * last), (np.where(last == 1.0, 2, 1).astype(np.int8), last)):
            X = ssr.positions(it, t, stage, tt)
            r = sref.seg_tri_np(np.concatenate([X[:, 0], X[:, 1]], axis=1), X[:, 2:])
            for k in range(n):
                if r.cross[k] and kind in ssr.EXEMPT:
                    continue
                m = Fraction(float(np.max(np.abs(X[k]))))
                ex = ssr.exact_pair_d2(X[k, :2], X[k, 2:]) / (m * m)                         # in units of M: the scaled classes lose nothing
                exact = Fraction(math.isqrt(int(ex * (1 << 400)))) / (1 << 200)            # sqrt to 2^-200
                w = max(w, float(abs(Fraction(float(r.dist[k])) / m - exact)))
        worst[kind] = w
    return worst


def test_seg_tri_error_against_the_asserted_bound():
    worst = measured_seg_tri_error()
    print({k: (round(math.log2(v), 2) if v > 0 else None) for k, v in worst.items()})
    assert max(worst.values()) <= ssr.SEG_TRI_BOUND, worst
    assert max(worst.values()) > ssr.SEG_TRI_BOUND / 2 ** 6                      # (the bound is the measurement rounded up, not a guess far above it)
    assert ssr.SEG_TRI_BOUND <= ssr.DELTA / 2 ** 10                              # delta covers it and the rounding of forming the positions


def test_equivariant_under_powers_of_two():
    """Items, triangles and dist scaled by 2^k over those of scale_inputs.SCALES inside seg_tri's band (ray_tri's: largest |coordinate|
    about 2^-300 .. 2^300): the same toi bits, evaluation counts, s, u, v, feature, end, cross and side; dist, qs and qt times 2^k."""
    g = np.random.default_rng(5)
    parts = [ssr.pin_class(k, 100, g) for k in ("pt_random", "pt_approach", "pt_end_touch", "pt_degenerate", "edge_on", "rim", "vertex", "rotating_segment",
                                                 "cross_start", "shrink", "zero_length")]
    it, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    base = ssr.seg_advance_np(it, t)
    assert np.isfinite(base.toi).sum() > 500 and len(np.unique(base.toi)) > 200 and base.cross.any()
    band = [k for k in si.SCALES if abs(k) <= 256]
    assert len(band) >= len(si.SCALES) - 1 and 256 in band and -200 in band
    for k in band:
        a = ssr.seg_advance_np(si.scaled(it, k), si.scaled(t, k))
        assert _same(a.toi, base.toi) and np.array_equal(a.evals, base.evals), k
        for name in ("dist", "on_seg", "on_tri"):
            assert _same(getattr(a, name), si.scaled(getattr(base, name), k)), (k, name)
        for name in ("s", "uv", "feature", "end", "cross", "side"):
            assert _same(getattr(a, name), getattr(base, name)), (k, name)


def test_pin_inputs_visit_every_branch():
    inputs = ssr.pin_inputs(128, seed=1)
    it, t = np.concatenate([v[0] for v in inputs.values()]), np.concatenate([v[1] for v in inputs.values()])
    adv = ssr.seg_advance_np(it, t)
    ssr.pin_conditions(it, t, adv)
    per = {k: ssr.seg_advance_np(*v) for k, v in inputs.items()}
    assert np.all(per["pt_start_within"].toi == 0.0) and np.all(per["pt_start_within"].evals == 1)
    assert np.all(per["pt_end_touch"].toi == 1.0) and np.all(per["pt_end_touch"].evals == 2)
    u = per["pt_unresolved"]
    assert np.all(u.evals == ssr.MAX_EVALS) and np.all(u.dist > inputs["pt_unresolved"][0][:, 12]) and np.all(np.isfinite(u.toi) & (u.toi < 1.0))
    assert np.all(per["pt_long"].evals >= 100) and np.all(per["pt_long"].evals < ssr.MAX_EVALS)
    c = per["cross_start"]
    assert np.all(c.cross == 1) and np.all(c.toi == 0.0) and np.all(c.dist == 0.0) and np.all(c.evals == 1)
    for kind in ("edge_on", "rim"):                                            # both ends stay outside dist: edge against edge, strictly inside the step
        a = per[kind]
        assert np.all((a.toi > 0.0) & (a.toi < 1.0)) and np.all(a.term >= 8) and np.all(a.end == 0) and np.all(a.cross == 0), kind
    assert (per["vertex"].term >= 8).all() and ((per["vertex"].term >= 8) & (per["vertex"].term < 11)).any()
    z = inputs["zero_length"][0]
    assert np.array_equal(z[:, 0:3], z[:, 3:6]) and np.array_equal(z[:, 6:9], z[:, 9:12])
    s = inputs["shrink"][0]
    assert np.array_equal(s[:, 6:9], s[:, 9:12]) and not np.array_equal(s[:, 0:3], s[:, 3:6])


def test_evaluation_bound_and_no_nan():
    g = np.random.default_rng(11)
    parts = [ssr.pin_class(k, 300, g) for k in ("pt_random", "pt_approach", "pt_near_parallel", "pt_degenerate", "pt_rotating", "rotating_segment", "rim", "edge_on")]
    parts += [ssr.pin_class(k, 30, g) for k in ("pt_long", "pt_unresolved")]
    it, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    t[:300, 3:] += g.normal(size=(300, 3, 3)) * 20.0                       # fast, tumbling vertices: many evaluations, some unresolved
    adv = ssr.seg_advance_np(it, t)
    L = ssr.rate_np(it, t)
    assert np.all(adv.evals <= 2 + 2 * L / it[:, 12] * (1 + 1e-12))
    unres = np.isfinite(adv.toi) & (adv.dist > it[:, 12])
    assert unres.any() and np.all(adv.evals[unres] == ssr.MAX_EVALS) and np.all(L[unres] > 511 * it[unres, 12] * 0.99)
    for name in ("dist", "s", "on_seg", "on_tri", "uv"):
        assert np.isfinite(getattr(adv, name)).all(), name
    assert not np.isnan(adv.toi).any()
    for kind in ("pt_scaled_up", "pt_scaled_down"):
        a = ssr.seg_advance_np(*ssr.pin_class(kind, 100, g))
        assert all(np.isfinite(getattr(a, name)).all() for name in ("dist", "s", "on_seg", "on_tri", "uv")) and not np.isnan(a.toi).any()
