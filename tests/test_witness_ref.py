"""The numpy restatement of tri_witness (tests/witness_ref.py) against its own definition, on the CPU: its distance is
proximity_ref.tri_distance_np's bit for bit, both points lie on their triangles, | |qa - qb| - dist | <= 2^-48 M, contact pairs have no
witness, power-of-two scaling is exact, the hand-built table has the expected features and points, and every one of the 33 terms wins
somewhere.  Checked on the pin's vector sets and on every mesh the GPU tests (tests/test_witness_gpu.py) use."""
from __future__ import annotations

import numpy as np
import pytest

import between_ref as br
import ccd_ref as cr
import proximity_ref as pr
import scale_inputs as si
import witness_ref as wr

BOUND = 2.0 ** -48


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _check(tri, what):
    """The properties of the definition on tri f64[n, 6, 3]; returns the witness."""
    tri = np.asarray(tri, dtype=np.float64).reshape(-1, 6, 3)
    w = wr.tri_witness_np(tri)
    assert np.array_equal(_bits(w.dist), _bits(pr.tri_distance_np(tri))), what
    for x in (w.dist, w.points, w.bary):
        assert np.all(np.isfinite(x)), what
    none = pr.in_contact(tri) | (np.abs(tri - tri[:, :1]).max(axis=(1, 2)) == 0)
    assert np.array_equal(none, w.feature[:, 0] == wr.FEATURE_NONE) and np.array_equal(none, w.feature[:, 1] == wr.FEATURE_NONE), what
    assert np.all(w.dist[none] == 0) and np.all(w.points[none] == 0) and np.all(w.bary[none] == 0) and np.all(w.win[none] == -1), what
    assert np.all(w.feature[~none] <= 6) and np.all(w.win[~none] >= 0), what
    u, v = w.bary[..., 0], w.bary[..., 1]
    assert np.all(u >= 0.0) and np.all(v >= 0.0) and np.all(u + v <= 1.0 + 2.0 ** -52), what    # (1 - t) + t may round up by one ulp
    M = np.abs(tri).max(axis=(1, 2))
    gap = np.sqrt(((w.points[:, 0] - w.points[:, 1]) ** 2).sum(axis=1))
    err = np.abs(gap - w.dist)[~none]
    worst = float(np.max(err / M[~none])) if err.size else 0.0
    print(f"{what}: {tri.shape[0]} pairs, {int(none.sum())} without a witness, worst | |qa - qb| - dist | / M = 2^{np.log2(worst) if worst else -np.inf:.1f}")
    assert worst <= BOUND, (what, worst)
    # features and barycentrics agree: a vertex code has 0 / 1 weights, an edge code one zero weight
    for side in (0, 1):
        f, uu, vv = w.feature[:, side], u[:, side], v[:, side]
        ww = (1.0 - uu) - vv
        for code, (a, b) in {4: (0.0, 0.0), 5: (1.0, 0.0), 6: (0.0, 1.0)}.items():
            assert np.all((uu[f == code] == a) & (vv[f == code] == b)), (what, code)
        assert np.all(vv[f == 1] == 0) and np.all(uu[f == 3] == 0), what
        assert np.all(np.abs(ww[f == 2]) <= 2.0 ** -52), what
    return w


@pytest.fixture(scope="module")
def sets():
    return wr.pin_sets(20000)


def test_definition_on_the_vector_sets(sets):
    for name, tri in sets.items():
        w = _check(tri, name)
        if name == "contact":
            assert (w.feature[:, 0] == wr.FEATURE_NONE).sum() > tri.shape[0] // 4
        if name == "grid":                                                          # ties: the value is attained by several terms
            assert np.unique(w.win).size > 10


def test_every_term_wins_somewhere(sets):
    w = wr.tri_witness_np(sets["unit"])
    assert set(np.unique(w.win[w.win >= 0]).tolist()) == set(range(33))


@pytest.mark.parametrize("k", si.EDGES)
def test_scaling_by_a_power_of_two_is_exact(sets, k):
    for name, tri in sets.items():
        w0 = wr.tri_witness_np(tri)
        wk = wr.tri_witness_np(si.scaled(tri, k))
        assert np.array_equal(_bits(wk.dist), _bits(si.scaled(w0.dist, k))), name
        assert np.array_equal(_bits(wk.points), _bits(si.scaled(w0.points, k))), name
        assert np.array_equal(_bits(wk.bary), _bits(w0.bary)) and np.array_equal(wk.feature, w0.feature) and np.array_equal(wk.win, w0.win), name


# (A, B, winning term, features, (ua, va), (ub, vb), qa, qb, dist^2): small-integer geometry, every value exact
_B = [(0, 0, 0), (4, 0, 0), (0, 4, 0)]
TABLE = {
    "vertex-face": ([(1, 1, 1), (2, 1, 3), (1, 2, 3)], _B, 0, (4, 0), (0, 0), (0.25, 0.25), (1, 1, 1), (1, 1, 0), 1),
    "face-vertex": (_B, [(1, 1, 1), (2, 1, 3), (1, 2, 3)], 1, (0, 4), (0.25, 0.25), (0, 0), (1, 1, 0), (1, 1, 1), 1),
    "vertex-edge": ([(2, -1, 1), (1, -3, 2), (3, -3, 2)], _B, 2, (4, 1), (0, 0), (0.5, 0), (2, -1, 1), (2, 0, 0), 2),
    "edge-vertex": (_B, [(2, -1, 1), (1, -3, 2), (3, -3, 2)], 5, (1, 4), (0.5, 0), (0, 0), (2, 0, 0), (2, -1, 1), 2),
    "vertex-vertex": ([(-1, -1, 1), (-3, -1, 2), (-1, -3, 2)], _B, 2, (4, 4), (0, 0), (0, 0), (-1, -1, 1), (0, 0, 0), 3),
    "edge-edge": ([(0, -2, 1), (0, 2, 1), (0, 0, 5)], [(-2, 0, 0), (2, 0, 0), (0, 0, -4)], 8, (1, 1), (0.5, 0), (0.5, 0), (0, 0, 1), (0, 0, 0), 1),
    "edge12-edge20": ([(0, 0, 5), (0, -2, 1), (0, 2, 1)], [(2, 0, 0), (0, 0, -4), (-2, 0, 0)], 21, (2, 3), (0.5, 0.5), (0, 0.5), (0, 0, 1), (0, 0, 0), 1),
    # two parallel unit squares' triangles, one above the other: every term is at 1 and the FIRST keeps the tie -- A's vertex 0 against
    # B's face, although the point on B is B's vertex 0
    "tie": ([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 0, 1), (1, 0, 1), (0, 1, 1)], 0, (4, 0), (0, 0), (0, 0), (0, 0, 0), (0, 0, 1), 1),
    # the upper triangle moved so that only A's vertex 1 lies under it (under B's vertex 0): term 0 is +inf (A's vertex 0 projects outside
    # B), term 1 -- B's vertex 0 against A's face -- is at 1 and keeps the tie against the vertex-vertex terms: A reports its FACE at (1, 0)
    "tie-second": ([(-1, 0, 0), (0, 0, 0), (-1, 1, 0)], [(0, 0, 1), (1, 0, 1), (0, 1, 1)], 1, (0, 4), (1, 0), (0, 0), (0, 0, 0), (0, 0, 1), 1),
}


@pytest.mark.parametrize("name", list(TABLE))
def test_hand_built_table(name):
    A, B, win, feat, ba, bb, qa, qb, d2 = TABLE[name]
    tri = np.array([A + B], dtype=np.float64)
    w = _check(tri, name)
    assert int(w.win[0]) == win, (name, int(w.win[0]))
    assert tuple(w.feature[0].tolist()) == feat
    assert w.bary[0].tolist() == [list(map(float, ba)), list(map(float, bb))]
    assert w.points[0].tolist() == [list(map(float, qa)), list(map(float, qb))]
    assert w.dist[0] == np.sqrt(float(d2))
    shifted = wr.tri_witness_np(tri + 1024.0)                                       # exact: the frame translates to A's first vertex
    assert np.array_equal(shifted.feature, w.feature) and np.array_equal(shifted.win, w.win) and np.array_equal(_bits(shifted.bary), _bits(w.bary))


def _tri_of(rows, va, ia, vb, ib, va1=None, vb1=None):
    fa, fb = rows.faces[:, 0].astype(np.int64), rows.faces[:, 1].astype(np.int64)
    ia, ib = np.asarray(ia, dtype=np.int64), np.asarray(ib, dtype=np.int64)
    if rows.toi is None:
        return np.concatenate([va[ia[fa]], vb[ib[fb]]], axis=1)
    return np.concatenate([wr.positions_at(va[ia[fa]], va1[ia[fa]], rows.toi), wr.positions_at(vb[ib[fb]], vb1[ib[fb]], rows.toi)], axis=1)


_key3 = wr.sort_by_ids


@pytest.mark.parametrize("name", list(wr.self_meshes()))
def test_self_proximity_rows(name):
    verts, vidx, ids, edge = wr.self_meshes()[name]
    idv = np.arange(vidx.shape[0]) if ids is None else ids
    for d in wr.self_dists(edge):
        rows = wr.cached(("prox", name, d), lambda: wr.witness_pairs(verts, vidx, ids, d))
        want = pr.proximity_pairs(verts, vidx, ids, d)
        for g, w in zip(_key3(rows.pairs, rows.dists), _key3(*want)):
            assert np.array_equal(g, w), (name, d)
        assert np.array_equal(idv[rows.faces.astype(np.int64)], rows.pairs)
        assert np.all((rows.pairs[:, 0] < rows.pairs[:, 1]) | ((rows.pairs[:, 0] == rows.pairs[:, 1]) & (rows.faces[:, 0] < rows.faces[:, 1])))
        w = _check(_tri_of(rows, verts, vidx, verts, vidx), f"{name} d={d}")
        assert np.array_equal(_bits(w.points), _bits(rows.points)) and np.array_equal(w.feature, rows.feature)


@pytest.mark.parametrize("name", ["soup10k", "cloth100"])
def test_self_ccd_rows(name):
    verts, vidx, ids, edge = wr.self_meshes()[name]
    x1, d = wr.ccd_case(name)
    rows = wr.cached(("ccd", name, d), lambda: wr.witness_pairs(verts, vidx, ids, d, verts_end=x1))
    want = cr.ccd_pairs(verts, x1, vidx, ids, d)
    for g, w in zip(_key3(rows.pairs, rows.toi, rows.dists), _key3(*want)):
        assert np.array_equal(g, w), name
    assert (rows.toi == 0).any() and ((rows.toi > 0) & (rows.toi < 1)).any()
    _check(_tri_of(rows, verts, vidx, verts, vidx, x1, x1), f"{name} ccd")


@pytest.mark.parametrize("name", list(wr.between_cases()))
def test_between_rows(name):
    va, ia, vb, ib, d = wr.between_cases()[name]
    rows = wr.cached(("bprox", name), lambda: wr.witness_pairs_between(va, ia, vb, ib, d))
    want = br.proximity_pairs(va, ia, vb, ib, d)
    for g, w in zip(_key3(rows.pairs, rows.dists), _key3(*want)):
        assert np.array_equal(g, w), name
    assert rows.faces.shape[0] > 0
    _check(_tri_of(rows, va, ia, vb, ib), f"{name} between")
    va1 = br.motion(va, 0.3 * d, 12)
    rows = wr.cached(("bccd", name), lambda: wr.witness_pairs_between(va, ia, vb, ib, d, ccd=True, va1=va1))
    want = br.ccd_pairs(va, ia, vb, ib, d, va1=va1)
    for g, w in zip(_key3(rows.pairs, rows.toi, rows.dists), _key3(*want)):
        assert np.array_equal(g, w), name
    _check(_tri_of(rows, va, ia, vb, ib, va1, vb), f"{name} between ccd")
