"""CPU checks of the continuous collision restatement (tests/ccd_ref.py) and of the new entry points' argument errors.

The guarantee: a pair whose exact linearly moving triangles come closer than h - delta (h = dist / 2,
delta = 2^-38 of the pair's largest |coordinate|) at some t* is reported with toi <= t*, and is never closer than h - delta before
toi.  It is checked against exact rationals: positions p0 + t (p1 - p0) at dyadic t as Fractions, the exact distance (0 where the
triangles intersect, decided by exact orientation tests)."""
from __future__ import annotations

import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import ccd_ref as cr
import mi355cd
import mi355_synth as synth
import scale_inputs as si

DELTA_REL = 2.0 ** -38


def _one(a0, b0, a1, b1):
    return np.concatenate([np.asarray(a0, float), np.asarray(b0, float), np.asarray(a1, float), np.asarray(b1, float)])[None]


BIG = np.array([[-10.0, -10.0, 0.0], [10.0, -10.0, 0.0], [0.0, 10.0, 0.0]])


@pytest.mark.parametrize("H,v,dist", [(1.0, 2.0, 0.01), (0.5, 3.0, 0.001), (2.0, 2.5, 0.1), (0.3, 0.4, 0.05)])
def test_falling_vertex(H, v, dist):
    tri = np.array([[0.0, 0.0, H], [1.0, 0.0, H + 1.0], [0.0, 1.0, H + 1.0]])
    down = np.array([0.0, 0.0, -v])
    toi, d, ev = cr.advance_np(_one(BIG, tri, BIG, tri + down), dist)
    assert (H - dist) / v <= toi[0] <= (H - dist / 2) / v, (toi, d, ev)
    assert d[0] <= dist


@pytest.mark.parametrize("H,v,dist", [(1.0, 2.0, 0.01), (0.25, 1.0, 0.002)])
def test_crossing_skew_edges(H, v, dist):
    a = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0]])
    b = np.array([[0.0, -1.0, H], [0.0, 1.0, H], [0.0, 0.0, H + 1.0]])
    down = np.array([0.0, 0.0, -v])
    toi, d, ev = cr.advance_np(_one(a, b, a, b + down), dist)
    assert (H - dist) / v <= toi[0] <= (H - dist / 2) / v, (toi, d, ev)
    assert d[0] <= dist


def test_pure_translation_one_evaluation():
    g = np.random.default_rng(3)
    a = np.round(g.uniform(-1, 1, (64, 3, 3)) * 1024) / 1024; b = np.round(g.uniform(-1, 1, (64, 3, 3)) * 1024) / 1024 + np.array([3.0, 0, 0])
    move = np.array([0.25, -0.5, 0.125]) * 8                            # dyadic positions and move: p1 - p0 and the mean are exact
    tri = np.concatenate([a, b, a + move, b + move], axis=1)
    assert np.all(cr.rate_np(tri) == 0.0)
    toi, d, ev = cr.advance_np(tri, 0.1)
    assert np.all(ev == 1) and np.all(np.isinf(toi))


def _moving_pairs(kind, n, g):
    """f64[n, 12, 3] moving pairs of one kind that come close or pass through each other inside the step."""
    if kind == "random":
        a = g.uniform(-1, 1, (n, 3, 3)); b = g.uniform(-1, 1, (n, 3, 3))
        off = g.normal(size=(n, 1, 3)); off *= 1.8 / np.linalg.norm(off, axis=2, keepdims=True)
        return np.concatenate([a, b + off, a + g.normal(size=(n, 1, 3)) * 0.1, b - off], axis=1)
    if kind == "near_parallel":
        d = g.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        e = d + g.normal(size=(n, 3)) * 1e-9
        nrm = np.cross(d, g.normal(size=(n, 3))); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        a = np.stack([np.zeros((n, 3)), d, 0.5 * d + g.normal(size=(n, 3)) * 0.3], axis=1)
        b = np.stack([0.2 * d, 0.2 * d + e, d + g.normal(size=(n, 3)) * 0.3], axis=1) + 0.3 * nrm[:, None]
        return np.concatenate([a, b, a, b - 0.6 * nrm[:, None]], axis=1)
    if kind == "degenerate":
        p = _moving_pairs("random", n, g)
        k = n // 3
        p[:k, [1, 7]] = p[:k, [0, 6]]                                        # a repeated vertex at both ends
        p[k:2 * k, 2] = p[k:2 * k, 0] + 0.37 * (p[k:2 * k, 1] - p[k:2 * k, 0])   # collinear at x0
        p[2 * k:, [4, 5]] = p[2 * k:, [3, 3]]                                  # B a point at x0 ...
        p[2 * k:, [10, 11]] = p[2 * k:, [9, 9]]                                # ... and at x1
        return p
    if kind == "rotating":
        a = g.uniform(-1, 1, (n, 3, 3)); b = g.uniform(-1, 1, (n, 3, 3)) + np.array([1.2, 0.0, 0.0])
        th = g.uniform(0.3, 1.5, n)
        c, s = np.cos(th), np.sin(th)
        R = np.zeros((n, 3, 3)); R[:, 0, 0] = c; R[:, 0, 1] = -s; R[:, 1, 0] = s; R[:, 1, 1] = c; R[:, 2, 2] = 1.0
        ctr = b.mean(axis=1, keepdims=True)
        b1 = np.einsum("nij,nkj->nki", R, b - ctr) + ctr - np.array([0.6, 0.0, 0.0])   # rigidly rotated and moved closer
        return np.concatenate([a, b, a, b1], axis=1)
    raise ValueError(kind)


def _check_guarantee(tri, dist, samples=24):
    toi, d, ev = cr.advance_np(tri, dist)
    h = dist * 0.5
    checked = 0
    for k in range(tri.shape[0]):
        m = float(np.max(np.abs(tri[k])))
        lim = h - DELTA_REL * m
        if lim <= 0:
            continue
        lim2 = Fraction(lim) ** 2
        end = 1.0 if np.isinf(toi[k]) else float(toi[k])
        ts = [Fraction(i, samples) for i in range(samples + 1) if Fraction(i, samples) < Fraction(end)]
        if np.isfinite(toi[k]) and toi[k] > 0:
            ts += [Fraction(end) * (1 - Fraction(1, 2 ** e)) for e in (4, 10, 30)]
        elif np.isinf(toi[k]):
            ts.append(Fraction(1))
        for t in ts:
            P, Q = cr.exact_at(tri[k], t)
            assert cr.exact_dist2(P, Q) >= lim2, (k, float(t), toi[k], d[k], ev[k])
            checked += 1
    return toi, d, ev, checked


@pytest.mark.parametrize("kind", ["random", "near_parallel", "degenerate", "rotating"])
def test_guarantee_against_exact_rationals(kind):
    g = np.random.default_rng({"random": 1, "near_parallel": 2, "degenerate": 3, "rotating": 4}[kind])
    tri = _moving_pairs(kind, 30, g)
    toi, d, ev, checked = _check_guarantee(tri, 0.05)
    assert checked > 300
    assert np.isfinite(toi).sum() >= 5                                     # many of them do come close


@pytest.mark.parametrize("scale", [1e100, 1e-100])
def test_guarantee_scaled(scale):
    tri = _moving_pairs("random", 20, np.random.default_rng(9)) * scale
    toi, d, ev, checked = _check_guarantee(tri, 0.05 * scale, samples=12)
    ref = cr.advance_np(tri / scale, 0.05)
    assert checked > 100 and np.isfinite(toi).sum() == np.isfinite(ref[0]).sum()


def test_evaluation_bound():
    g = np.random.default_rng(11)
    tri = np.concatenate([_moving_pairs(k, 2000, g) for k in ("random", "near_parallel", "degenerate", "rotating")])
    tri[:1000, 6:] += g.normal(size=(1000, 6, 3)) * 20.0                   # fast, tumbling vertices: many evaluations, some unresolved
    for dist in (0.05, 0.01):
        toi, d, ev = cr.advance_np(tri, dist)
        L = cr.rate_np(tri)
        assert np.all(ev <= 2 + 2 * L / dist * (1 + 1e-12))
        unres = np.isfinite(toi) & (d > dist)
        assert np.all(ev[unres] == cr.MAX_EVALS)
        assert np.all(L[unres] > 511 * dist * 0.99)
        assert np.all(ev >= 1) and np.all(ev <= cr.MAX_EVALS)


def _motion(verts, amp, seed):
    g = np.random.default_rng(seed)
    return verts + g.normal(size=verts.shape) * amp


def test_grid_matches_all_pairs():
    verts, vidx = synth.soup(1500, e=0.05, seed=5)
    x1 = _motion(verts, 0.02, 6)
    for dist in (0.01, 0.03):
        a = cr.ccd_pairs(verts, x1, vidx, None, dist, brute=True)
        b = cr.ccd_pairs(verts, x1, vidx, None, dist, brute=False)
        assert a[0].shape[0] > 0
        for u, v in zip(a, b):
            assert np.array_equal(u, v)


def test_no_motion_and_t0_equal_proximity():
    import proximity_ref as pr
    verts, vidx = synth.soup(800, e=0.05, seed=7)
    for dist in (0.005, 0.02):
        p, t, d = cr.ccd_pairs(verts, verts, vidx, None, dist)
        wp, wd = pr.proximity_pairs(verts, vidx, None, dist)
        assert np.array_equal(p, wp) and np.array_equal(d.view(np.uint64), wd.view(np.uint64)) and np.all(t == 0.0)


def test_argument_errors_without_a_device():
    lib = mi355cd.load_library()
    tri = np.zeros((1, 36))
    out = np.zeros(1); d = np.zeros(1); e = np.zeros(1, dtype=np.uint32)
    for dist in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.cd_ccd_points(tri.ctypes.data, 1, dist, out.ctypes.data, d.ctypes.data, e.ctypes.data) == mi355cd.CD_ERR_ARG
    assert lib.cd_ccd_points(None, 1, 0.1, out.ctypes.data, d.ctypes.data, e.ctypes.data) == mi355cd.CD_ERR_ARG
    n = C.c_uint64(0)
    assert lib.cd_find_ccd(None, tri.ctypes.data, 0.1, None, None, None, 0, C.byref(n), None) == mi355cd.CD_ERR_ARG
    assert lib.cd_self_ccd(None, tri.ctypes.data, 0.1, None, None, None, 0, C.byref(n), None) == mi355cd.CD_ERR_ARG


@pytest.mark.parametrize("name", list(si.meshes()))
def test_restatement_is_equivariant_under_powers_of_two(name):
    """x0, x1 and dist scaled by 2^k over scale_inputs.SCALES (past both ends of the fp32 range): the same pairs, the same toi bits,
    distances times 2^k exactly, and the same gate and evaluation counts -- what tests/test_query_scales_gpu.py compares the device
    with at every scale."""
    v, vidx, edge = si.meshes()[name]
    x1 = si.motion(v, edge)
    dist = edge / 4
    (p0, t0, d0), counts0 = cr.ccd_pairs(v, x1, vidx, None, dist, brute=False, counts=True)
    assert p0.shape[0] > vidx.shape[0] and np.all(d0 <= dist)                       # many pairs, none unresolved
    assert len(np.unique(t0)) > 100
    for k in si.SCALES:
        (pk, tk, dk), countsk = cr.ccd_pairs(si.scaled(v, k), si.scaled(x1, k), vidx, None, np.ldexp(dist, k), brute=False, counts=True)
        assert np.array_equal(pk, p0) and countsk == counts0, (k, pk.shape, p0.shape, countsk, counts0)
        assert np.array_equal(tk.view(np.uint64), t0.view(np.uint64)), k
        assert np.array_equal(dk.view(np.uint64), np.ldexp(d0, k).view(np.uint64)), k
