"""CPU checks of the swept-point restatement (tests/sweep_ref.py).

The guarantee: a point that comes closer than h - delta (h = dist / 2, delta = 2^-38 of the pair's largest
|coordinate|) to the exactly, linearly moving triangle at some t* is reported with toi <= t*, and is never closer than h - delta before
toi.  It is checked against exact rationals: positions a + t (b - a) at dyadic t as Fractions and the exact point-triangle distance."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest

import mi355_synth as synth
import point_ref as ptr
import scale_inputs as si
import sweep_ref as sr
import within_ref as wr

DELTA_REL = 2.0 ** -38
BIG = np.array([[-10.0, -10.0, 0.0], [10.0, -10.0, 0.0], [0.0, 10.0, 0.0]])


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _one(p0, p1, dist, a, b):
    return np.array([[*p0, *p1, dist]], dtype=np.float64), np.concatenate([np.asarray(a, float), np.asarray(b, float)])[None]


@pytest.mark.parametrize("H,v,dist", [(1.0, 2.0, 0.01), (0.5, 3.0, 0.001), (2.0, 2.5, 0.1), (0.3, 0.4, 0.05)])
def test_falling_point(H, v, dist):
    adv = sr.pt_advance_np(*_one([0.1, 0.2, H], [0.1, 0.2, H - v], dist, BIG, BIG))
    assert (H - dist) / v <= adv.toi[0] <= (H - dist / 2) / v, adv
    assert adv.dist[0] <= dist and adv.feature[0] == 0 and adv.side[0] == 1
    assert np.allclose(adv.closest[0], [0.1, 0.2, 0.0]) and adv.closest[0, 2] == 0.0


def test_rising_triangle_meets_resting_point():
    """The triangle moves, the point rests: q is on the triangle as it stands at toi."""
    up = np.array([0.0, 0.0, 2.0])
    adv = sr.pt_advance_np(*_one([0.3, -0.4, 1.0], [0.3, -0.4, 1.0], 0.01, BIG, BIG + up))
    assert (1.0 - 0.01) / 2.0 <= adv.toi[0] <= (1.0 - 0.005) / 2.0
    assert abs(adv.closest[0, 2] - 2.0 * adv.toi[0]) < 1e-12 and adv.side[0] == 1


def test_exact_distance_agrees_with_point_ref():
    g = np.random.default_rng(2)
    for kind in ("random", "degenerate"):
        it, t = sr.pin_class(kind, 20, g)
        for k in range(20):
            p, tri = sr.exact_at(it[k], t[k], Fraction(0))
            assert sr.exact_dist2(p, tri) == ptr.exact_pt_tri(it[k, 0:3], t[k, :3])[0]


def test_common_translation_costs_one_evaluation():
    it, t = sr.pin_class("translate", 64, np.random.default_rng(3))
    assert np.all(sr.rate_np(it, t) == 0.0)
    adv = sr.pt_advance_np(it, t)
    assert np.all(adv.evals == 1)
    near = np.arange(64) % 4 == 0
    assert np.all(adv.toi[near] == 0.0) and np.all(np.isinf(adv.toi[~near]))
    d0 = ptr.pt_tri_np(it[:, 0:3], t[:, :3])[0]
    assert np.array_equal(_bits(adv.dist), _bits(d0))                      # the one evaluation is on p0 and x0 themselves


def _check_guarantee(it, tri, samples=24):
    adv = sr.pt_advance_np(it, tri)
    checked = 0
    for k in range(it.shape[0]):
        m = max(float(np.max(np.abs(it[k, :6]))), float(np.max(np.abs(tri[k]))))
        lim = it[k, 6] * 0.5 - DELTA_REL * m
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
            assert sr.exact_dist2(*sr.exact_at(it[k], tri[k], t)) >= lim2, (k, float(t), toi, adv.dist[k], adv.evals[k])
            checked += 1
    return adv, checked


@pytest.mark.parametrize("kind", ["random", "approach", "near_parallel", "degenerate", "rotating", "end_touch"])
def test_guarantee_against_exact_rationals(kind):
    g = np.random.default_rng(sr.CLASSES.index(kind) + 1)
    it, t = sr.pin_class(kind, 30, g)
    adv, checked = _check_guarantee(it, t)
    assert checked > (300 if kind != "near_parallel" else 100), checked
    if kind != "near_parallel":
        assert np.isfinite(adv.toi).sum() >= 5                             # many of them do come close
    rep = np.isfinite(adv.toi) & (adv.dist <= it[:, 6])
    for k in np.nonzero(rep)[0]:                                           # a reported pair IS within dist at toi, up to delta
        p, tri = sr.exact_at(it[k], t[k], Fraction(float(adv.toi[k])))
        m = max(float(np.max(np.abs(it[k, :6]))), float(np.max(np.abs(t[k]))))
        assert sr.exact_dist2(p, tri) <= Fraction(it[k, 6] + DELTA_REL * m) ** 2


@pytest.mark.parametrize("kind", ["scaled_up", "scaled_down"])
def test_guarantee_scaled(kind):
    it, t = sr.pin_class(kind, 20, np.random.default_rng(9))
    adv, checked = _check_guarantee(it, t, samples=12)
    assert checked > 100 and np.isfinite(adv.toi).sum() >= 3


def test_equivariant_under_powers_of_two():
    """Items, triangles and dist scaled by 2^k over scale_inputs.SCALES (the band of DESIGN.md section 11): the same toi bits, evaluation
    counts, u, v, feature and side, and dist and closest times 2^k exactly."""
    g = np.random.default_rng(5)
    parts = [sr.pin_class(k, 200, g) for k in ("random", "approach", "end_touch", "degenerate", "rotating", "start_within")]
    it, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    base = sr.pt_advance_np(it, t)
    assert np.isfinite(base.toi).sum() > 300 and len(np.unique(base.toi)) > 100
    for k in si.SCALES:
        a = sr.pt_advance_np(si.scaled(it, k), si.scaled(t, k))
        assert np.array_equal(_bits(a.toi), _bits(base.toi)) and np.array_equal(a.evals, base.evals), k
        assert np.array_equal(_bits(a.dist), _bits(si.scaled(base.dist, k))) and np.array_equal(_bits(a.closest), _bits(si.scaled(base.closest, k))), k
        assert np.array_equal(_bits(a.uv), _bits(base.uv)) and np.array_equal(a.feature, base.feature) and np.array_equal(a.side, base.side), k


def test_pin_inputs_visit_every_branch():
    inputs = sr.pin_inputs(256, seed=1)
    it, t = np.concatenate([v[0] for v in inputs.values()]), np.concatenate([v[1] for v in inputs.values()])
    adv = sr.pt_advance_np(it, t)
    sr.pin_conditions(it, t, adv)
    per = {k: sr.pt_advance_np(*v) for k, v in inputs.items()}
    assert np.all(per["start_within"].toi == 0.0) and np.all(per["start_within"].evals == 1)
    assert np.all(per["end_touch"].toi == 1.0) and np.all(per["end_touch"].evals == 2)
    assert np.all(per["unresolved"].evals == sr.MAX_EVALS) and np.all(per["unresolved"].dist > inputs["unresolved"][0][:, 6])
    assert np.all(np.isfinite(per["unresolved"].toi) & (per["unresolved"].toi < 1.0))
    assert np.all(per["long"].evals >= 100) and np.all(per["long"].evals < sr.MAX_EVALS)
    assert np.all(np.isfinite(per["long"].toi[1::2])) and np.all(np.isinf(per["long"].toi[0::2]))
    inside = (per["approach"].toi > 0.0) & (per["approach"].toi < 1.0)
    assert inside.sum() >= 0.9 * inside.size


def test_evaluation_bound():
    g = np.random.default_rng(11)
    parts = [sr.pin_class(k, 1000, g) for k in ("random", "approach", "near_parallel", "degenerate", "rotating")]
    parts += [sr.pin_class(k, 50, g) for k in ("long", "unresolved")]
    it, t = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    t[:1000, 3:] += g.normal(size=(1000, 3, 3)) * 20.0                     # fast, tumbling vertices: many evaluations, some unresolved
    adv = sr.pt_advance_np(it, t)
    L = sr.rate_np(it, t)
    assert np.all(adv.evals <= 2 + 2 * L / it[:, 6] * (1 + 1e-12))
    unres = np.isfinite(adv.toi) & (adv.dist > it[:, 6])
    assert unres.any() and np.all(adv.evals[unres] == sr.MAX_EVALS) and np.all(L[unres] > 511 * it[unres, 6] * 0.99)


# ---------------------------------------------------------------- the row set
def _case(n_tri=600, n_items=200, seed=5, dist=0.02):
    verts, vidx = synth.soup(n_tri, e=0.1, seed=seed)
    g = np.random.default_rng(seed + 1)
    x1 = verts + g.normal(size=verts.shape) * 0.03
    p0 = ptr.mesh_points(verts, vidx, n_items, seed=seed, edge=0.1)
    p1 = p0 + g.normal(size=p0.shape) * 0.1
    return verts, x1, vidx, np.concatenate([p0, p1, np.full((n_items, 1), dist)], axis=1)


def test_rows_are_the_gated_pairs_the_advancement_reports():
    verts, x1, vidx, it = _case()
    w, (tested, evals, unres) = sr.sweep_rows_ref(verts, x1, vidx, None, it, counts=True)
    n, nt = it.shape[0], vidx.shape[0]
    six = np.concatenate([verts[vidx], x1[vidx]], axis=1)
    k, f = np.divmod(np.arange(n * nt), nt)                                # every pair, one by one
    g = sr.gate_np(it[k], six[f])
    adv = sr.pt_advance_np(it[k[g]], six[f[g]])
    hit = np.isfinite(adv.toi)
    assert tested == g.sum() and evals == adv.evals.sum() and w.rows.shape[0] == hit.sum() > 50
    assert np.array_equal(w.rows, np.stack([k[g][hit], f[g][hit]], axis=1)) and np.array_equal(_bits(w.toi), _bits(adv.toi[hit]))
    # a pair the gate turns away is more than dist apart throughout: advancing it all the same reports nothing
    rest = np.nonzero(~g)[0][:: max(1, (~g).sum() // 5000)]
    assert np.all(np.isinf(sr.pt_advance_np(it[k[rest]], six[f[rest]]).toi))


def test_first_of_is_the_smallest_row():
    verts, x1, vidx, it = _case(dist=0.06)
    ids = np.random.default_rng(2).integers(0, 50, vidx.shape[0]).astype(np.uint32)   # repeated IDs: the face index decides
    w = sr.sweep_rows_ref(verts, x1, vidx, ids, it)
    face, oid, toi, dist, q, uv, feat, side = sr.first_of(w, it.shape[0])
    seen = 0
    for k in range(it.shape[0]):
        at = np.nonzero(w.rows[:, 0] == k)[0]
        if at.size == 0:
            assert face[k] == sr.NONE and np.isinf(toi[k]) and oid[k] == 0 and dist[k] == 0 and not q[k].any()
            continue
        best = min(at, key=lambda r: (w.toi[r], w.ids[r], w.rows[r, 1]))
        assert face[k] == w.rows[best, 1] and oid[k] == w.ids[best] and toi[k] == w.toi[best] and dist[k] == w.dist[best]
        seen += at.size > 1
    assert seen > 20


def test_no_motion_is_points_within_and_skip_removes_incident_faces():
    verts, x1, vidx, it = _case()
    still = it.copy(); still[:, 3:6] = still[:, 0:3]
    w = sr.sweep_rows_ref(verts, None, vidx, None, still)
    want = wr.points_within_ref(verts, vidx, None, still[:, 0:3], still[:, 6])
    assert want.rows.shape[0] > 20 and np.array_equal(w.rows, want.rows) and np.all(w.toi == 0.0)
    for a, b in zip((w.ids, w.dist, w.closest, w.uv, w.feature, w.side), want[1:]):
        assert np.array_equal(_bits(a), _bits(b)) if b.dtype == np.float64 else np.array_equal(a, b)
    nv = verts.shape[0]
    own = np.concatenate([verts, x1, np.full((nv, 1), 0.02)], axis=1)       # the mesh's own vertices
    plain = sr.sweep_rows_ref(verts, x1, vidx, None, own)
    skipped = sr.sweep_rows_ref(verts, x1, vidx, None, own, skip=np.arange(nv))
    inc = (vidx[plain.rows[:, 1]] == plain.rows[:, 0:1]).any(axis=1)
    assert inc.sum() == 3 * vidx.shape[0] and np.all(plain.toi[inc] == 0.0)       # every incident face: a row at toi 0
    assert np.array_equal(skipped.rows, plain.rows[~inc]) and np.array_equal(_bits(skipped.toi), _bits(plain.toi[~inc]))
