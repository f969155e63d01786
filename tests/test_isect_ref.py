"""tri_isect's numpy restatement (tests/isect_ref.py) against its stated properties (include/mi355cd.h): the swap
law, exact scaling, no NaN, both endpoints on both triangles within 2^-42 M, the hand-built table, and the conditions on the inputs the
GPU tests rely on.  CPU only.

The bound.  ENDPOINT_BOUND = 2^-42 M comes from the restatement, not from the device code: the worst endpoint_error over every input
the tests use -- the seven sets of pin_sets(PIN_ROWS) and the rows of every mesh of self_meshes() and between_cases() -- was measured
at 2^-44.58 M (a pair of the sliver set; 2^-44.63 M on the unit set), and two bits of margin were added."""
from __future__ import annotations

import numpy as np
import pytest

import isect_ref as ir
import proximity_ref as pr

ENDPOINT_BOUND = 2.0 ** -42
PIN_ROWS = 28672                    # rows a set: 7 x 28672 = 200 704, the large pin of tests/test_contour_gpu.py


def _bits(d):
    return np.ascontiguousarray(d, dtype=np.float64).view(np.uint64)


def _sets():
    return ir.cached(("sets", PIN_ROWS), lambda: ir.pin_sets(PIN_ROWS))


def _isect(name):
    return ir.cached(("isect", name), lambda: ir.tri_isect_np(_sets()[name]))


SETS = ("unit", "small", "offset", "grid", "sliver", "degenerate", "apart")


def test_the_sets_are_the_seven():
    assert tuple(_sets()) == SETS


@pytest.mark.parametrize("name", SETS)
def test_no_nan_and_the_coding(name):
    w = _isect(name)
    assert not np.isnan(w.param).any() and not np.isnan(w.points).any()
    nh = w.hit.sum(axis=1)
    assert np.array_equal(w.n, np.minimum(nh, 2))
    term = w.code[:, :2] & 7
    assert np.array_equal(term[:, 0] != ir.TERM_NONE, nh >= 1) and np.array_equal(term[:, 1] != ir.TERM_NONE, nh >= 2)
    gone = term == ir.TERM_NONE
    assert np.all(w.code[:, :2][gone] == ir.TERM_NONE)                          # a missing endpoint: 7, side 0, zeros
    assert not w.param[gone].any() and not w.points[gone].any()
    r = np.arange(w.n.shape[0])
    for s in range(2):                                                          # an endpoint is one of the terms that hit
        ok = ~gone[:, s]
        assert np.all(w.hit[r[ok], term[ok, s]])
        assert np.all((w.param[ok, s, 0] >= 0.0) & (w.param[ok, s, 0] <= 1.0))
        assert np.all((w.param[ok, s, 1] >= 0.0) & (w.param[ok, s, 2] >= 0.0) & (w.param[ok, s, 1] + w.param[ok, s, 2] <= 1.0))
    two = nh == 2                                                               # exactly two hits: the two hits in term order
    first = np.argmax(w.hit, axis=1)
    last = 5 - np.argmax(w.hit[:, ::-1], axis=1)
    assert np.array_equal(term[two, 0], first[two]) and np.array_equal(term[two, 1], last[two])
    assert np.all(term[nh >= 2, 0] < term[nh >= 2, 1])


@pytest.mark.parametrize("name", SETS)
def test_swap_law(name):
    t = _sets()[name]
    w = _isect(name)
    s = ir.tri_isect_np(np.concatenate([t[:, 3:], t[:, :3]], axis=1))
    k = (np.arange(6) + 3) % 6
    assert np.array_equal(s.hit, w.hit[:, k])                                   # exactly the terms (k + 3) mod 6 ...
    for a, b in ((s.t, w.t), (s.u, w.u), (s.v, w.v), (s.x, w.x)):               # ... with bit-identical t, u, v, side, x
        assert np.array_equal(_bits(a), _bits(b[:, k]))
    assert np.array_equal(s.side, w.side[:, k])
    assert np.array_equal(s.n, w.n)
    # the endpoints: the same farthest distance; with exactly two hits the same two terms, possibly in the other order
    two = w.hit.sum(axis=1) == 2
    st, wt = np.sort((s.code[two, :2] & 7).astype(np.int64), axis=1), np.sort(((w.code[two, :2] & 7).astype(np.int64) + 3) % 6, axis=1)
    assert np.array_equal(st, wt)
    D = lambda q: ((q.points[:, 0] - q.points[:, 1]) ** 2).sum(axis=1)
    many = w.n == 2
    assert np.array_equal(_bits(D(s)[many]), _bits(D(w)[many]))


@pytest.mark.parametrize("k", [0, 128, -149])
@pytest.mark.parametrize("name", SETS)
def test_scaling_by_a_power_of_two(name, k):
    t = _sets()[name][:4096]
    w = ir.tri_isect_np(t)
    s = ir.tri_isect_np(np.ldexp(t, k))
    assert np.array_equal(s.code, w.code)
    assert np.array_equal(_bits(s.param), _bits(w.param))
    assert np.array_equal(_bits(s.points), _bits(np.ldexp(w.points, k)))


@pytest.mark.parametrize("name", SETS)
def test_endpoints_lie_on_both_triangles(name):
    err = ir.endpoint_error(_sets()[name], _isect(name))
    print(f"{name}: worst endpoint error 2^{np.log2(err.max()) if err.max() > 0 else -np.inf:.2f} M")
    assert err.max() <= ENDPOINT_BOUND


def _mesh_rows():
    out = {}
    for name, (v, i, ids) in ir.self_meshes().items():
        r = ir.cached(("self", name), lambda: ir.contour_pairs(v, i, ids))
        tv = v[np.asarray(i, dtype=np.int64)]
        out["self " + name] = (r, np.concatenate([tv[r.faces[:, 0]], tv[r.faces[:, 1]]], axis=1))
    for name, (va, ia, vb, ib, ida, idb) in ir.between_cases().items():
        r = ir.cached(("between", name), lambda: ir.contour_pairs_between(va, ia, vb, ib, ida, idb))
        out["between " + name] = (r, np.concatenate([va[np.asarray(ia, dtype=np.int64)][r.faces[:, 0]], vb[np.asarray(ib, dtype=np.int64)][r.faces[:, 1]]], axis=1))
    return out


def test_the_meshes_rows():
    """The rows of every mesh the GPU tests use: the bound, no NaN, and what the meshes are there for."""
    rows = _mesh_rows()
    nhits = {}
    for name, (r, tri) in rows.items():
        w = ir.tri_isect_np(tri)
        assert np.array_equal(w.code, r.code) and np.array_equal(_bits(w.param.reshape(-1, 6)), _bits(r.param)), name
        assert not np.isnan(r.param).any() and not np.isnan(r.points).any(), name
        err = ir.endpoint_error(tri, w)
        assert err.size == 0 or err.max() <= ENDPOINT_BOUND, (name, err.max())
        nhits[name] = np.bincount(w.hit.sum(axis=1), minlength=7)
    for name in ("self n1", "self n2"):
        assert rows[name][0].faces.shape[0] == 0
    for name in ("self n63", "self n64", "self n65", "self n513", "self soup10k", "self cloth70", "self degenerate", "self custom_ids",
                 "between soups", "between cloth40", "between nb1"):
        assert rows[name][0].faces.shape[0] > 0, name
    assert rows["self cloth70"][0].faces.shape[0] > 2000
    for name in ("self grid400", "between grid_ids"):                           # ties and multi-hit rows
        assert np.all(nhits[name][[0, 2, 3, 4, 5, 6]] > 0), (name, nhits[name])
    assert nhits["between shared_positions"][1] > 0                             # rows with one endpoint
    # custom_ids: repeated IDs, and pairs the ID rule removes
    v, i, ids = ir.self_meshes()["custom_ids"]
    assert np.unique(ids).shape[0] < ids.shape[0]
    r = rows["self custom_ids"][0]
    assert np.all(r.pairs[:, 0] < r.pairs[:, 1])
    assert ir.contour_pairs(v, i, None).faces.shape[0] > r.faces.shape[0]


def test_conditions_on_the_inputs():
    """On the three generic sets every pair in contact has exactly two hits; the grid set has pairs with 0, 3, 4, 5 and 6 hits; the
    pairs of 'apart' are not in contact."""
    for name in ir.GENERIC:
        c = pr.in_contact(_sets()[name])
        nh = _isect(name).hit.sum(axis=1)
        assert c.sum() > PIN_ROWS // 5 and np.all(nh[c] == 2), (name, np.bincount(nh[c]))
    g = _isect("grid").hit.sum(axis=1)
    gc = pr.in_contact(_sets()["grid"])
    hist = np.bincount(g[gc], minlength=7)
    assert np.all(hist[[0, 2, 3, 4, 5, 6]] > 0), hist
    assert not pr.in_contact(_sets()["apart"]).any()
    assert pr.in_contact(_sets()["sliver"]).sum() > PIN_ROWS // 10
    assert pr.in_contact(_sets()["degenerate"]).sum() > PIN_ROWS // 10


def test_hand_built_table():
    for name, (a, b, n, mask) in ir.table().items():
        w = ir.tri_isect_np(np.concatenate([a, b])[None])
        assert w.n[0] == n and w.code[0, 2] == mask, (name, w.n, w.code)
    T = ir.table()
    one = lambda k: ir.tri_isect_np(np.concatenate(T[k][:2])[None])
    w = one("one_each")                                                         # A's edge 01 up through B, B's edge 12 through A
    assert w.code[0].tolist() == [0, 4, 0b010001]
    assert w.param[0, 0].tolist() == [0.5, 0.5, 0.25] and w.points[0].tolist() == [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]
    w = one("two_of_a")                                                         # edges 01 and 20 of A, from below and from above
    assert (w.code[0, :2] & 7).tolist() == [0, 2] and (w.code[0, :2] >> 3).tolist() == [0, 1]
    assert w.points[0].tolist() == [[1.25, 1.0, 0.0], [1.0, 1.25, 0.0]] and w.param[0, :, 0].tolist() == [0.5, 0.5]
    w = one("through_vertex")                                                   # the duplicate point: (0, 4) beats (0, 3), and keeps the ties with (3, 4), (4, 5)
    assert (w.code[0, :2] & 7).tolist() == [0, 4]
    assert w.points[0].tolist() == [[0.0, 0.0, 0.0], [1.0, 1.0, 0.0]]
    for k in (3, 5):
        assert np.array_equal(w.x[0, k], w.x[0, 0])
    w = one("coplanar")
    assert w.code[0].tolist() == [7, 7, 0] and not w.param.any() and not w.points.any()
    six = ir.grid_six_hits()
    assert six is not None
    w = ir.tri_isect_np(six[None])
    assert w.code[0, 2] == 63 and w.n[0] == 2
    # the kept pair is the first, in lexicographic order, that attains the largest D
    x = w.x[0]
    D = {(i, j): float(((x[i] - x[j]) ** 2).sum()) for i in range(6) for j in range(i + 1, 6)}
    best = max(D.values())
    assert tuple((w.code[0, :2] & 7).tolist()) == min(p for p, d in D.items() if d == best)
